"""The certification ladder of FlatIPIndex.search_begin / search_finish, rung by rung, without a GPU.

The ladder is host code: which queries are re-run, with which capacity, threshold and scan, and what `stats` says afterwards.
`LadderStub` replaces the device calls (search_device, search_deep_device, last_counts, _rebuild_scaled, _search_exhaustive,
_search_large_k) by recorders whose `status` vectors come from a script; every call is logged and fills the D / I it returns
with its serial number, so the final D shows which call each query's row came from.

The expectations in tests/golden/search_ladder_traces.json were RECORDED from the two-ladder code this file's ladder replaced
(`python tests/test_search_ladder_cpu.py --record` with that version of convdr_amd first on the path), not from the code
under test."""
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.environ.get("CONVDR_LADDER_PACKAGE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from convdr_amd import search as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_ladder_traces.json")
OK, OVERFLOW, TOO_FEW, UNCERTAIN, RANGE = 0, 1, 2, 3, 4
SHALLOW_K, DEEP_K = 10, 5000


class LadderStub(S.FlatIPIndex):
    """FlatIPIndex with the attributes the ladder reads and scripted recorders where it calls the device."""

    def __init__(self, precision="auto", half=False, cap=4096, n=100000, script=(), default=OK, counts=None):
        self.device = torch.device("cpu")
        self.precision, self.kind = precision, S._KINDS[precision]
        self._store = S.STORES["fp16" if half else "fp32"]
        self.cap, self._n = int(cap), int(n)
        self.d = self.d_in = 64
        self.stats = {}
        self._x3_first = False
        self.script, self.default, self.counts = list(script), default, counts
        self.trace, self.serial = [], 0

    def _record(self, route, q, k, tau_in, cap, x3):
        nq = int(q.shape[0])
        self.serial += 1
        self.trace.append([route, nq, int(k), int(cap), tau_in is None, x3])
        if tau_in is not None:
            assert tuple(tau_in.shape) == (nq,)
        st = self.script.pop(0) if self.script else self.default
        st = [st] * nq if isinstance(st, int) else list(st)
        assert len(st) == nq, "script entry %r for a call with %d queries (call %d)" % (st, nq, self.serial)
        return (torch.full((nq, k), float(self.serial), dtype=torch.float32), torch.full((nq, k), self.serial, dtype=torch.int64),
                torch.tensor(st, dtype=torch.int32), torch.zeros(nq, dtype=torch.float32))

    def search_device(self, q, k, tau_in=None, cap=None, x3=None):
        return self._record("shallow", q, k, tau_in, cap or self.cap, x3)

    def search_deep_device(self, q, k, tau_in=None, cap=None, x3=False):
        return self._record("deep", q, k, tau_in, cap or self._deep_cap(k), x3)

    def last_counts(self, nq, k, cap=None):
        self.trace.append(["last_counts", nq, int(k), cap])
        emitted, band = self.counts
        assert len(emitted) == nq
        return torch.tensor(emitted, dtype=torch.int32), torch.tensor(band, dtype=torch.int32)

    def _rebuild_scaled(self):
        self.trace.append(["rebuild"])

    def _last_rung(self, route, q, k):
        nq = int(q.shape[0])
        self.serial += 1
        self.trace.append([route, nq, int(k)])
        return torch.full((nq, k), float(self.serial), dtype=torch.float32), torch.full((nq, k), self.serial, dtype=torch.int64)

    def _search_exhaustive(self, q, k):
        return self._last_rung("exhaustive", q, k)

    def _search_large_k(self, q, k):
        return self._last_rung("large_k", q, k)


# One entry per rung: constructor arguments of the stub, the number of queries and how many searches are made in a row.  A script
# entry is the status vector of one enqueue, in call order (an int stands for every query of that call); `default` answers the
# calls after the script's end.
NQ = 6
RUNGS = {
    "all_ok": dict(),
    "range_first_pass": dict(script=[[RANGE, OK, OK, RANGE, OK, OK], [OK, OK, UNCERTAIN, OK, OK, OK], [OK]]),
    # queries 0 and 3: band >= emitted > 0 and UNCERTAIN -> straight to the split scan (shallow); 1 and 4 are retried -- 4 has a
    # saturated band but is not UNCERTAIN; 1 clears in its second retry, 4 never does and joins the split scan, which leaves
    # one of the three for a retry of its own
    "saturated_band_beside_retries": dict(
        script=[[UNCERTAIN, UNCERTAIN, OK, UNCERTAIN, TOO_FEW, OK]],
        counts=([50, 50, 50, 4096, 7, 0], [50, 20, 0, 5000, 9, 0])),
    "overflow_to_the_capacity_limit": dict(cap=1024, default=OVERFLOW),
    "never_clears": dict(default=UNCERTAIN),
    "pinned_fp16x3": dict(precision="fp16x3", script=[[OK, UNCERTAIN, OK, TOO_FEW, OK, OK], [UNCERTAIN, OK], [OK]]),
    "pinned_fp16x3_never_clears": dict(precision="fp16x3", default=TOO_FEW),
    "x3_first_on_the_second_search": dict(
        searches=2,
        # search 1: first pass leaves 4 of 6 open, six retry rounds change nothing, the split scan certifies them (4 > 6 // 2);
        # search 2 starts on the split scan: one query open, one retry
        script=[[UNCERTAIN, UNCERTAIN, OK, UNCERTAIN, UNCERTAIN, OK]] + [UNCERTAIN] * 6 + [OK]
               + [[OK, OK, OK, OK, OVERFLOW, OK], [OK]]),
    "half_store_x2": dict(half=True,
                          script=[[RANGE, UNCERTAIN, OK, OK, OK, OK], [OK, UNCERTAIN, UNCERTAIN, OK, OK, OK]] + [UNCERTAIN] * 6
                                 + [[OK, TOO_FEW], [OK]]),
    # (recorded when no bf16 kernel could report RANGE and the ladder retried it like any status; since the bf16 kinds refuse norms
    #  below their floor a RANGE from them is final: the search raises after this one pass -- test_ladder_trace holds the case to
    #  the first call of the recorded trace and to the error)
    "bf16_ignores_range": dict(precision="bf16", script=[[RANGE, OK, OK, OK, OK, OK]]),
}
# saturated_band_beside_retries continues differently per depth (the deep ladder has no shortcut), so its tail is per depth
TAILS = {
    ("saturated_band_beside_retries", SHALLOW_K): [[UNCERTAIN, TOO_FEW], [OK, TOO_FEW]] + [[TOO_FEW]] * 4 + [[OK, UNCERTAIN, OK], [OK]],
    ("saturated_band_beside_retries", DEEP_K): [[OK, UNCERTAIN, OK, TOO_FEW], [OK, TOO_FEW]] + [[TOO_FEW]] * 4 + [[OK]],
}
CASES = [("%s-k%d" % (name, k), name, k) for name in RUNGS for k in (SHALLOW_K, DEEP_K)] + \
        [("empty_index-k%d" % DEEP_K, "empty", DEEP_K), ("beyond_deep_max_k", "beyond", S.FlatIPIndex.DEEP_MAX_K + 1)]


def run_case(name, k):
    """What the ladder did: per search the stats, _x3_first and the serial-number image of (D, I); the call trace of all."""
    if name == "empty":
        spec = dict(n=0)
    elif name == "beyond":
        spec = dict(n=70000)
    else:
        spec = dict({"counts": ([50] * NQ, [20] * NQ)}, **RUNGS[name])      # (bands well inside the lists unless the rung says otherwise)
        spec["script"] = list(spec.get("script", ())) + TAILS.get((name, k), [])
    searches = spec.pop("searches", 1)
    idx = LadderStub(**spec)
    q = torch.zeros((NQ, idx.d), dtype=torch.float32)
    out = {"searches": []}
    for _ in range(searches):
        try:
            D, I = idx.search_finish(idx.search_begin(q, k))
        except S._lib.ConvdrError as e:
            out["raised"] = str(e)
            break
        assert tuple(D.shape) == (NQ, k) and tuple(I.shape) == (NQ, k) and D.dtype == torch.float32 and I.dtype == torch.int64
        assert bool((D == D[:, :1]).all()) and bool((I == I[:, :1]).all())       # a row comes from ONE call
        out["searches"].append({"stats": idx.stats, "x3_first": bool(idx._x3_first),
                                "D": D[:, 0].double().tolist(), "I": I[:, 0].tolist()})
    assert not idx.script, "unused script entries: %r" % (idx.script,)
    out["trace"] = idx.trace
    return json.loads(json.dumps(out, default=lambda v: v.item()))         # (numpy scalars in stats; tuples become lists)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_every_case(golden):
    assert sorted(golden) == sorted(c[0] for c in CASES)


@pytest.mark.parametrize("case,name,k", CASES, ids=[c[0] for c in CASES])
def test_ladder_trace(golden, case, name, k):
    got, want = run_case(name, k), golden[case]
    if name == "bf16_ignores_range":
        # a bf16 scan has no scale to rebuild: RANGE ends the search loudly, with the cause and the remedy, after ONE pass
        assert got["trace"] == want["trace"][:1] and got["searches"] == []
        assert "CONVDR_IP_RANGE" in got["raised"] and "2^-60" in got["raised"] and 'precision="auto"' in got["raised"]
        return
    assert "raised" not in got
    assert got["trace"] == want["trace"]
    assert len(got["searches"]) == len(want["searches"])
    for g, w in zip(got["searches"], want["searches"]):
        assert g["stats"] == w["stats"]
        assert {k_: type(v) for k_, v in g["stats"].items()} == {k_: type(v) for k_, v in w["stats"].items()}
        assert g["x3_first"] == w["x3_first"]
        assert g["D"] == w["D"] and g["I"] == w["I"]


def test_the_cases_reach_the_rungs_they_are_named_for(golden):
    """The recorded traces themselves: a script that missed its rung would pin nothing."""
    def routes(case):
        return [t[0] for t in golden[case]["trace"]]

    def stats(case, i=0):
        return golden[case]["searches"][i]["stats"]
    assert routes("all_ok-k10") == ["shallow"] and routes("all_ok-k5000") == ["deep"]
    for k in (SHALLOW_K, DEEP_K):
        assert routes("range_first_pass-k%d" % k)[1] == "rebuild" and stats("range_first_pass-k%d" % k)["rescaled"] == 1
        assert "rebuild" not in routes("bf16_ignores_range-k%d" % k)
        assert stats("half_store_x2-k%d" % k)["x2_queries"] == 2 and stats("half_store_x2-k%d" % k)["x3_queries"] == 0
        assert golden["x3_first_on_the_second_search-k%d" % k]["searches"][0]["x3_first"]
        assert stats("x3_first_on_the_second_search-k%d" % k, 1)["x3_first"]
        assert not any(t[0] in ("shallow", "deep") and t[5] is False for t in golden["pinned_fp16x3-k%d" % k]["trace"])
    sat = golden["saturated_band_beside_retries-k10"]
    assert sat["trace"][1][0] == "last_counts" and sat["trace"][2][:2] == ["shallow", 2]     # 0 and 3 skip the retries
    assert "last_counts" not in routes("saturated_band_beside_retries-k5000")
    caps = [t[3] for t in golden["overflow_to_the_capacity_limit-k10"]["trace"] if t[0] == "shallow"]
    assert max(caps) == 8192 and routes("overflow_to_the_capacity_limit-k10")[-1] == "exhaustive"
    caps = [t[3] for t in golden["overflow_to_the_capacity_limit-k5000"]["trace"] if t[0] == "deep"]
    assert max(caps) == S.FlatIPIndex.DEEP_MAX_CAP and stats("overflow_to_the_capacity_limit-k5000")["deep_cap"] == max(caps)
    assert routes("never_clears-k10").count("shallow") == 1 + 6 + 1 + 6 and routes("never_clears-k10")[-1] == "exhaustive"
    assert routes("never_clears-k5000").count("deep") == 1 + 6 + 1 + 6 and routes("never_clears-k5000")[-1] == "large_k"
    assert stats("never_clears-k10")["exhaustive_queries"] == NQ and stats("never_clears-k5000")["chunked_queries"] == NQ
    assert routes("empty_index-k5000") == [] and routes("beyond_deep_max_k") == ["large_k"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_search_ladder_cpu.py --record    (writes %s)" % GOLDEN)
    print("recording from", S.__file__)
    with open(GOLDEN, "w") as f:
        json.dump({case: run_case(name, k) for case, name, k in CASES}, f, indent=1, sort_keys=False)
        f.write("\n")
