"""Range search, the parts that need no GPU: every refusal of convdr_ip_range_search / convdr_ip_range_pack / the workspace
function (argument validation happens before anything touches a device), and the host ladder of FlatIPIndex.range_search
against a scripted pass."""
import os
import re

import numpy as np
import pytest
import torch

from convdr_amd import _lib
from convdr_amd import search as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, OVERFLOW, RANGE = 0, 1, 4


def _call(L, store=1, nq=5, scale=4.0, centre=None, n=100000, d=768, cap=4096, count_only=0, bits=None, words=0):
    """Every pointer but the centre and the bitmap (neither is dereferenced on the host) is NULL and the workspace has 0 bytes:
    a call that got past validation could not return these messages."""
    return L.convdr_ip_range_search(store, None, nq, None, None, scale, centre, n, d, None, None, cap, count_only, bits, words,
                                    None, 0, None, None, None, None)


@pytest.mark.parametrize("store", [0, 1, 2])
def test_every_refusal_of_the_search_entry_is_a_negative_code_with_a_message(store):
    L = _lib.lib()
    words = (100000 + 255) // 256 * 8
    cases = [
        ({"store": 3}, b"store must be"),
        ({"store": -1}, b"store must be"),
        ({"cap": 5000}, b"cap must be a power of two"),
        ({"cap": 512}, b"cap must be a power of two"),
        ({"cap": 262144}, b"cap must be a power of two"),
        ({"cap": 0}, b"cap must be a power of two"),
        ({"d": 70}, b"d % 64"),
        ({"d": 0}, b"d % 64"),
        ({"d": 4160}, b"d <= 4096"),
        ({"n": 1 << 31}, b"bad block size"),
        ({"n": -1}, b"bad block size"),
        ({"nq": 0}, b"bad sizes"),
        ({"nq": -3}, b"bad sizes"),
        ({"count_only": 2}, b"count_only"),
        ({"bits": (1 << 20) + 4, "words": words}, b"16-byte aligned"),
        ({"bits": 1 << 20, "words": words - 8}, b"the bitmap holds"),          # one tile short
        ({"bits": 1 << 20, "words": 0}, b"the bitmap holds"),
        ({"bits": None, "words": 8}, b"row_bits is NULL"),
    ]
    if store != 0:
        cases += [({"scale": 0.75}, b"power of two"), ({"scale": 0.0}, b"power of two"), ({"scale": float("inf")}, b"power of two")]
    if store == 2:
        cases += [({"scale": 0.5}, b"power of two >= 1"), ({"centre": 1 << 20}, b"no centre")]
    for kw, msg in cases:
        rc = _call(L, **{"store": store, **kw})
        assert rc < 0 and msg in L.convdr_last_error(), (kw, rc, L.convdr_last_error())
    # the first check past all of them, with and without a bitmap, in both modes, at both ends of cap
    for kw in ({}, {"bits": 1 << 20, "words": words}, {"count_only": 1}, {"cap": 1024}, {"cap": 131072}, {"n": 0}):
        assert _call(L, store=store, **kw) < 0 and b"workspace too small" in L.convdr_last_error(), kw
    if store == 0:          # the bf16 copy has no scale: whatever is passed is not read
        assert _call(L, store=0, scale=0.75) < 0 and b"workspace too small" in L.convdr_last_error()
    if store != 2:
        assert _call(L, store=store, centre=1 << 20) < 0 and b"workspace too small" in L.convdr_last_error()


def test_every_refusal_of_the_pack_entry():
    L = _lib.lib()
    for kw in ({"nq": 0}, {"n": 1 << 31}, {"n": -1}, {"d": 70}, {"d": 8192}, {"cap": 5000}, {"cap": 512}, {"cap": 262144}):
        a = dict(nq=5, n=1000, d=64, cap=4096)
        a.update(kw)
        rc = L.convdr_ip_range_pack(None, a["nq"], a["n"], a["d"], a["cap"], None, None, None, None, None)
        assert rc < 0 and b"outside the contract" in L.convdr_last_error(), (kw, L.convdr_last_error())
    assert L.convdr_ip_range_pack(None, 5, 1000, 64, 4096, None, None, None, None, None) < 0
    assert b"NULL argument" in L.convdr_last_error()


def test_workspace_bytes_is_monotone_and_zero_outside_the_contract():
    ws = _lib.lib().convdr_ip_range_workspace_bytes
    caps = [1 << e for e in range(10, 18)]
    for nq in (1, 37, 128, 129, 1000):
        sizes = [ws(nq, 100000, 768, cap) for cap in caps]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes), sizes
        assert sizes[0] >= nq * 1024 * 24                    # id + scan score + two fp64 scores per list entry
    for cap in (1024, 131072):
        sizes = [ws(nq, 100000, 768, cap) for nq in (1, 2, 100, 128, 129, 256, 1000, 5000)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), sizes
    assert ws(5, 0, 64, 1024) > 0                           # an empty block is inside the contract
    for args in ((0, 100, 64, 4096), (-1, 100, 64, 4096), (5, -1, 64, 4096), (5, 1 << 31, 64, 4096), (5, 100, 70, 4096),
                 (5, 100, 0, 4096), (5, 100, 4160, 4096), (5, 100, 64, 512), (5, 100, 64, 5000), (5, 100, 64, 262144)):
        assert ws(*args) == 0, args


def test_header_ctypes_and_exports_agree_on_the_entries():
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "convdr_hip.h")).read(), flags=re.S)
    for name in ("convdr_ip_range_workspace_bytes", "convdr_ip_range_search", "convdr_ip_range_pack"):
        assert name in _lib.exported_symbols() and hasattr(L, name)
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(params.split(",")) == len(_lib._SIGNATURES[name][1]), name


# ---- the host ladder against a scripted pass ---------------------------------------------------------------------------
class RangeStub(S.FlatIPIndex):
    """FlatIPIndex with the attributes the range ladder reads; _range_pass and _range_chunked are recorders.  `hits[j]` is what
    the scan reports for query j: a pass at `cap` answers OK with that many results when hits[j] <= cap, OVERFLOW with the hit
    count otherwise.  A result row of query j carries D = j and I = 1000 j + position."""

    def __init__(self, hits, cap=4096, kind="f16", n=1000000, range_first=0):
        self.device = torch.device("cpu")
        self.kind, self._store = kind, S.STORES["fp32"]
        self.cap, self._n = int(cap), int(n)
        self.d = self.d_in = 64
        self.stats = {}
        self.hits = np.asarray(hits, np.int64)
        self.trace, self.range_first = [], range_first

    def _ids(self, q):
        return q[:, 0].long().numpy()           # the test's queries carry their number in column 0

    def _result(self, js, lens):
        lims = torch.as_tensor(np.concatenate([[0], np.cumsum(lens)]))
        D = torch.cat([torch.full((int(n),), float(j)) for j, n in zip(js, lens)] + [torch.zeros(0)])
        I = torch.cat([1000 * int(j) + torch.arange(int(n)) for j, n in zip(js, lens)] + [torch.zeros(0, dtype=torch.int64)])
        return lims, D, I

    def _range_pass(self, q, rad, cap, count_only, allowed=None, rows=None, want_x=False):
        js = self._ids(q)
        assert tuple(rad.shape) == (len(js),) and rad.dtype == torch.float32 and rows is None
        self.trace.append(["pass", js.tolist(), int(cap), bool(count_only)])
        h = self.hits[js]
        if self.range_first:
            self.range_first -= 1
            return h, np.full(len(js), RANGE, np.int32), None, None, None, None
        st = np.where(h > cap, OVERFLOW, OK).astype(np.int32)
        if count_only:
            return h, st, None, None, None, None
        return (h, st) + self._result(js, np.where(st == OK, h, 0)) + (None,)

    def _range_chunked(self, q, rad, allowed, count_only):
        js = self._ids(q)
        self.trace.append(["chunked", js.tolist(), bool(count_only)])
        h = self.hits[js]
        if count_only:
            return h, None, None, None
        return (h,) + self._result(js, h)

    def _rebuild_scaled(self):
        self.trace.append(["rebuild"])


def _queries(nq):
    q = torch.zeros((nq, 64), dtype=torch.float32)
    q[:, 0] = torch.arange(nq)
    return q


def _check_result(idx, hits, lims, D, I):
    np.testing.assert_array_equal(lims.numpy(), np.concatenate([[0], np.cumsum(hits)]))
    for j, h in enumerate(hits):
        a = int(lims[j])
        assert (D[a:a + h] == float(j)).all() and I[a:a + h].tolist() == list(range(1000 * j, 1000 * j + h)), j
    assert D.dtype == torch.float32 and I.dtype == torch.int64 and lims.dtype == torch.int64
    assert idx.stats["range_results"] == int(np.sum(hits))


def test_ladder_picks_the_cap_from_the_reported_count():
    # 4096: first pass; 4097 -> 8192; 8192 -> 8192 (exactly full is no overflow); 20000 -> 32768; 131072 -> the largest list;
    # 131073 -> the last rung; 0: an empty run
    hits = [4096, 4097, 8192, 20000, 131072, 131073, 0, 5]
    idx = RangeStub(hits)
    lims, D, I = idx.range_search_tensors(_queries(8), 0.5)
    assert idx.trace == [["pass", list(range(8)), 4096, False], ["pass", [1, 2], 8192, False], ["pass", [3], 32768, False],
                         ["pass", [4], 131072, False], ["chunked", [5], False]], idx.trace
    _check_result(idx, hits, lims, D, I)
    assert idx.stats["range_rounds"] == 4 and idx.stats["range_cap"] == 131072 and idx.stats["range_chunked_queries"] == 1
    # one query far above the first list: ONE more pass, not three doublings
    idx = RangeStub([20000])
    lims, D, I = idx.range_search_tensors(_queries(1), torch.tensor([0.25]))
    assert [t[2] for t in idx.trace] == [4096, 32768] and idx.stats["range_rounds"] == 2 and idx.stats["range_cap"] == 32768
    _check_result(idx, [20000], lims, D, I)
    # nothing overflows: the pass's own tensors are the result
    idx = RangeStub([3, 0, 7])
    lims, D, I = idx.range_search_tensors(_queries(3), np.float32(1.0))
    assert len(idx.trace) == 1 and idx.stats["range_rounds"] == 1 and idx.stats["range_chunked_queries"] == 0
    _check_result(idx, [3, 0, 7], lims, D, I)


def test_ladder_hands_over_to_the_last_rung_above_range_max_cap_and_counts():
    hits = [100, 3000, 2049, 2048, 1500]
    idx = RangeStub(hits, cap=1024)
    idx.RANGE_MAX_CAP = 2048
    lims, D, I = idx.range_search_tensors(_queries(5), 0.0)
    assert idx.trace == [["pass", [0, 1, 2, 3, 4], 1024, False], ["pass", [3, 4], 2048, False], ["chunked", [1, 2], False]]
    _check_result(idx, hits, lims, D, I)
    assert idx.stats["range_chunked_queries"] == 2 and idx.stats["range_cap"] == 2048
    # a first cap above the limit is cut to it
    idx = RangeStub([5000], cap=4096)
    idx.RANGE_MAX_CAP = 2048
    idx.range_search_tensors(_queries(1), 0.0)
    assert idx.trace == [["pass", [0], 2048, False], ["chunked", [0], False]]
    # range_count walks the same ladder in count-only mode
    idx = RangeStub(hits, cap=1024)
    idx.RANGE_MAX_CAP = 2048
    got = idx.range_count(_queries(5), 0.0)
    assert got.dtype == np.int64 and got.tolist() == hits
    assert idx.trace == [["pass", [0, 1, 2, 3, 4], 1024, True], ["pass", [3, 4], 2048, True], ["chunked", [1, 2], True]]


def test_ladder_rebuilds_once_on_range():
    idx = RangeStub([10, 5000], range_first=1)
    lims, D, I = idx.range_search_tensors(_queries(2), 0.0)
    assert [t[0] for t in idx.trace] == ["pass", "rebuild", "pass", "pass"] and idx.stats["rescaled"] == 1
    _check_result(idx, [10, 5000], lims, D, I)
    with pytest.raises(_lib.ConvdrError):
        RangeStub([10], range_first=2).range_search_tensors(_queries(1), 0.0)
    with pytest.raises(_lib.ConvdrError):
        RangeStub([10], kind="bf16", range_first=1).range_search_tensors(_queries(1), 0.0)


def test_empty_index_and_empty_filter_enqueue_nothing():
    for idx, allowed in ((RangeStub([1, 2], n=0), None),
                         (RangeStub([1, 2], n=512), S.RowFilter(torch.zeros(16, dtype=torch.int32), 512, 0))):
        lims, D, I = idx.range_search_tensors(_queries(2), 0.0, allowed=allowed)
        assert idx.trace == [] and lims.tolist() == [0, 0, 0] and D.numel() == 0 and I.numel() == 0
        assert idx.range_count(_queries(2), 0.0, allowed=allowed).tolist() == [0, 0]
    with pytest.raises(ValueError):         # a stale filter
        RangeStub([1], n=512).range_search_tensors(_queries(1), 0.0, allowed=S.RowFilter(torch.zeros(16, dtype=torch.int32), 511, 3))


def test_radius_forms_and_refusals():
    idx = RangeStub([1, 2, 3])
    q = _queries(3)
    for radius in (0.5, np.float32(0.5), np.full(3, 0.5, np.float32), torch.full((3,), 0.5), np.full(3, 0.5, np.float64),
                   float("inf"), -float("inf"), np.array([-np.inf, 0.0, np.inf], np.float32)):
        r = idx._range_radius(radius, 3)
        assert r.dtype == torch.float32 and tuple(r.shape) == (3,) and r.is_contiguous()
    assert idx._range_radius(0.1, 3).tolist() == [float(np.float32(0.1))] * 3
    for bad in (np.zeros(2, np.float32), np.zeros(4, np.float32), torch.zeros(0), np.zeros((3, 1), np.float32)):
        with pytest.raises(ValueError):
            idx.range_search_tensors(q, bad)
        with pytest.raises(ValueError):
            idx.range_count(q, bad)
    for bad in (float("nan"), np.array([0.0, np.nan, 1.0], np.float32), torch.tensor([float("nan")] * 3)):
        with pytest.raises(ValueError):
            idx.range_search_tensors(q, bad)
        with pytest.raises(ValueError):
            idx.range_count(q, bad)
    assert idx.trace == []


N_ROWS = 1000000
# the four workspace planners behind split_under, as ws(L, items per call, size): the list capacity, or for the distinct cut the
# length of the ranked lists; then a size where 1,000 items fit DEEP_WS_BYTES, the largest size, a count that does not fit at
# that size, and a size outside the contract
PLANNERS = {
    "range": (lambda L, c, cap: L.convdr_ip_range_workspace_bytes(c, N_ROWS, 768, cap), 4096, 131072, 4000, 5000),
    "rank": (lambda L, c, cap: L.convdr_ip_rank_workspace_bytes(c, N_ROWS, 768, cap), 4096, 131072, 4000, 5000),
    "deep_topk": (lambda L, c, cap: L.convdr_ip_deep_workspace_bytes(c, N_ROWS, 768, 5000, cap), 16384, 131072, 4000, 5000),
    "deep_distinct": (lambda L, c, n: L.convdr_topk_distinct_deep_workspace_bytes(c, n), 5000, 65536, 8000, 65537),
}


@pytest.mark.parametrize("planner", sorted(PLANNERS))
def test_queries_are_split_under_the_workspace_limit(planner):
    """split_under with the library's own workspace functions: one call never asks for more than DEEP_WS_BYTES, and the split
    is not finer than halving needs."""
    fn, small, large, many, bad = PLANNERS[planner]
    L = _lib.lib()

    def ws(c, size):
        return fn(L, c, size)

    def step(count, size, budget):
        got, need = S.split_under(lambda c: ws(c, size), count, budget)
        assert need == ws(got, size)
        return got
    budget = S.FlatIPIndex.DEEP_WS_BYTES
    assert step(1000, small, budget) == 1000 and ws(1000, small) <= budget
    got = step(many, large, budget)                   # range: 4000 x 131072 x 24 bytes = 12.6 GB in one call
    assert 1 <= got < many and ws(got, large) <= budget < ws(min(many, 2 * got), large)
    got = step(100, large, 64 << 20)
    assert 1 <= got < 100 and ws(got, large) <= (64 << 20) < ws(2 * got, large)
    assert step(100, small, 1) == 1                   # a single query is never split
    assert step(many, large, None) == many            # no budget: never split
    assert S.split_under(lambda c: ws(c, bad), 5, budget) == (5, 0)


def test_every_pass_refuses_sizes_outside_the_contract_in_its_own_words():
    """0 bytes from the workspace function: each user of split_under raises ConvdrError under its entry's name, before it
    touches the device (the passes are the real ones, called on the stub)."""
    idx = RangeStub([0])
    q, z = _queries(5), torch.zeros((10, 64))
    with pytest.raises(_lib.ConvdrError, match="convdr_ip_range_search: sizes outside the contract"):
        S.FlatIPIndex._range_pass(idx, q, torch.zeros(5), 5000, False, rows=(z, z))
    with pytest.raises(_lib.ConvdrError, match="convdr_ip_rank_rows: sizes outside the contract"):
        S.FlatIPIndex._rank_pass(idx, q, torch.zeros(5, dtype=torch.int64), 5000)
    with pytest.raises(_lib.ConvdrError, match="convdr_ip_search_deep: sizes outside the contract"):
        idx._enqueue(q, 5000, None, 5000, False, deep=True, rows=(z, z))


def test_a_status_that_is_neither_ok_nor_overflow_raises_after_one_pass():
    """STATUS_TOO_FEW belongs to the top-k entries: from a range pass it is a broken contract, not a rung of the ladder."""
    idx = RangeStub([10, 20])

    def too_few(q, rad, cap, count_only, allowed=None, rows=None, want_x=False):
        idx.trace.append(["pass", idx._ids(q).tolist(), int(cap), bool(count_only)])
        return idx.hits, np.asarray([OK, S.STATUS_TOO_FEW], np.int32), None, None, None, None
    idx._range_pass = too_few
    with pytest.raises(_lib.ConvdrError, match="convdr_ip_range_search: unexpected status"):
        idx.range_search_tensors(_queries(2), 0.0)
    assert idx.trace == [["pass", [0, 1], 4096, False]]
