"""What FlatIPIndex hands to the C ABI for each storage, argument for argument, without a GPU.

`_search_call` (every enqueue of the search ladder ends in it) and the C call of `score_rows_tensors` are driven on indexes
built without the constructor, over small CPU tensors; `_lib.lib()`, `_lib.check` and `_lib.stream_ptr` are recorders.  A trace
is the list of (entry name, arguments) with every pointer replaced by the name of the buffer it points to (None for NULL, "new"
for a tensor the call allocated itself); integers and floats stand as they are.

The expectations in tests/golden/store_calls.json were RECORDED from the commit before the store descriptions of
convdr_amd/stores.py, whose host code branched on the storage in both functions (`python tests/test_store_calls_cpu.py --record`
with that version of convdr_amd first on the path, CONVDR_STORE_CALLS_PACKAGE_ROOT), not from the code under test."""
import contextlib
import ctypes
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.environ.get("CONVDR_STORE_CALLS_PACKAGE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from convdr_amd import _lib
from convdr_amd import search as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "store_calls.json")
D_, NQ, N, K_SHALLOW, K_DEEP = 128, 3, 40, 5, 5000
# (storage, precision, scan kind, dtype of the scan operand, scale of the scan copy)
STORAGES = {"fp32-bf16": ("fp32", "bf16", "bf16", torch.bfloat16, 1.0), "fp32-fp16": ("fp32", "fp16", "f16", torch.float16, 4.0),
            "fp16": ("fp16", "auto", "f16", torch.float16, 8.0), "sq8": ("sq8", "auto", "i8", torch.int8, 1.0)}


def make_index(which, n):
    """(index, {data pointer: buffer name}): a FlatIPIndex of `n` rows as the constructor and add() would leave its fields"""
    storage, precision, kind, dtype, scale = STORAGES[which]
    idx = object.__new__(S.FlatIPIndex)
    idx.storage, idx.precision, idx.kind, idx.device = storage, precision, kind, torch.device("cpu")
    if hasattr(S, "STORES"):
        idx._store = S.STORES[storage]
    else:                   # (the recorded commit kept two flags)
        idx._half, idx._sq8 = storage == "fp16", storage == "sq8"
    idx.d = idx.d_in = D_
    idx._n, idx._scale = n, scale
    idx._s32 = torch.zeros((N, D_), dtype=torch.float32) if storage == "fp32" and n else None
    idx._s16 = torch.zeros((N, D_), dtype=dtype) if n else None
    idx._slo = None
    idx._max_norm = torch.ones(1, dtype=torch.float32)
    idx._centre = None if storage == "fp16" or not n else torch.zeros(D_, dtype=torch.float32)
    if storage == "sq8":
        idx._step = torch.ones(D_, dtype=torch.float32) if n else None
    names = {t.data_ptr(): name for name, t in (("s32", idx._s32), ("s16", idx._s16), ("max_norm", idx._max_norm),
                                                ("centre", idx._centre), ("step", getattr(idx, "_step", None))) if t is not None}
    return idx, names


class Recorder:
    """stands for the loaded library: every entry is a recorder that returns 0"""

    def __init__(self, names):
        self.names, self.calls = names, []

    def _arg(self, a):
        if isinstance(a, ctypes.c_void_p):
            return None if a.value is None else self.names.get(a.value, "new")
        assert a is None or isinstance(a, (int, float, str)), a
        return a

    def __getattr__(self, entry):
        def call(*args):
            self.calls.append([entry, [self._arg(a) for a in args]])
            return 0
        return call


@contextlib.contextmanager
def recording(names):
    rec = Recorder(names)
    saved = _lib.lib, _lib.check, _lib.stream_ptr, torch.cuda.device
    _lib.lib, _lib.stream_ptr, torch.cuda.device = (lambda: rec), (lambda: "stream"), (lambda dev: contextlib.nullcontext())
    _lib.check = lambda rc, what: rec.calls[-1].append(what)
    try:
        yield rec
    finally:
        _lib.lib, _lib.check, _lib.stream_ptr, torch.cuda.device = saved


def search_case(which, deep, filtered, split, empty):
    idx, names = make_index(which, 0 if empty else N)
    k = K_DEEP if deep else K_SHALLOW
    t = {"q": torch.zeros((NQ, D_)), "tau_in": torch.zeros(NQ), "ws": torch.zeros(64, dtype=torch.uint8), "D": torch.zeros((NQ, k)),
         "I": torch.zeros((NQ, k), dtype=torch.int64), "status": torch.zeros(NQ, dtype=torch.int32), "tau_retry": torch.zeros(NQ),
         "bits": torch.zeros(8, dtype=torch.int32)}
    plo = None
    if split and idx.storage == "fp32" and not empty:          # (the half store's split scan has no third operand)
        idx._slo = t["slo"] = torch.zeros((N, D_), dtype=idx._s16.dtype)
        plo = idx._plo
    names.update({v.data_ptr(): name for name, v in t.items()})
    # an empty index is enqueued with the queries in the rows' place: never dereferenced (FlatIPIndex._enqueue)
    p32, p16 = (t["q"], t["q"]) if empty else (idx._rows, idx._pbf)
    allowed = S.RowFilter(t["bits"], idx._n, 7) if filtered else None
    with recording(names) as rec:
        idx._search_call(t["q"], NQ, p32, p16, plo, idx._n, k, t["tau_in"], 16384 if deep else 4096, 0, t["ws"], t["D"], t["I"],
                         t["status"], t["tau_retry"], split, deep, allowed)
    return rec.calls


def score_case(which, empty):
    idx, names = make_index(which, 0 if empty else N)
    q, rows = torch.zeros((NQ, D_)), torch.full((NQ, 2), -1, dtype=torch.int64)
    names.update({q.data_ptr(): "q", rows.data_ptr(): "rows"})
    with recording(names) as rec:
        D, X = idx.score_rows_tensors(q, rows)
    assert tuple(D.shape) == tuple(X.shape) == (NQ, 2) and D.dtype == torch.float32 and X.dtype == torch.float64
    return rec.calls


def _cases():
    out = {}
    for which, (storage, _, _, _, _) in STORAGES.items():
        splits = (False,) if storage == "sq8" else (False, True)      # (the 8-bit store has one rung)
        for deep in (False, True):
            for filtered in (False, True):
                for split in splits:
                    for empty in (False, True):
                        name = "%s-search-%s-%s-%s-%s" % (which, "deep" if deep else "shallow", "filter" if filtered else "all",
                                                          "split" if split else "single", "n0" if empty else "rows")
                        out[name] = (search_case, (which, deep, filtered, split, empty))
        for empty in (False, True):
            out["%s-score_rows-%s" % (which, "n0" if empty else "rows")] = (score_case, (which, empty))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_every_case(golden):
    assert sorted(golden) == sorted(CASES) and len(CASES) == 3 * 16 + 8 + 4 * 2


@pytest.mark.parametrize("case", sorted(CASES))
def test_call_trace(golden, case):
    fn, args = CASES[case]
    got = json.loads(json.dumps(fn(*args)))
    assert len(got) == 1 and got[0][0] == got[0][2]            # one C call, checked under its own name
    assert got == golden[case]


def test_the_recorded_traces_name_the_buffers_they_should(golden):
    """The record itself: a trace that named no buffer would pin nothing."""
    for case, calls in golden.items():
        entry, args, _ = calls[0]
        assert "new" not in args or "score_rows" in case, case     # (score_rows_tensors allocates its outputs)
        assert ("_q8" in entry) == case.startswith("sq8") and ("filtered" in entry) == ("-filter-" in case), case
        if "-search-" in case:
            assert ("_deep" in entry or args[0 if "_q8" in entry else 1] == 1) == ("-deep-" in case), case
            assert [a for a in args if a in ("D", "I", "status", "tau_retry", "stream")] == ["D", "I", "status", "tau_retry", "stream"]
        if case.endswith("-rows"):
            assert "s16" in args and ("s32" in args) == case.startswith("fp32") and ("slo" in args) == ("fp32" in case and "-split-" in case)
            assert ("step" in args and "centre" in args) == case.startswith("sq8"), case
    assert golden["fp16-search-shallow-all-split-rows"][0][0] == "convdr_ip_search_h16"
    assert golden["fp32-fp16-search-deep-all-single-rows"][0][0] == "convdr_ip_search_deep_f16"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_store_calls_cpu.py --record    (writes %s)" % GOLDEN)
    print("recording from", S.__file__)
    with open(GOLDEN, "w") as f:
        json.dump({case: fn(*args) for case, (fn, args) in sorted(CASES.items())}, f, indent=1)
        f.write("\n")
