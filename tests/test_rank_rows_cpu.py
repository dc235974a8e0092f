"""Score and rank of given rows, the parts that need no GPU: the entries are declared and exported, every refusal of
convdr_ip_score_rows / convdr_ip_rank_rows / the workspace function (argument validation happens before anything touches a
device), the workspace layout against tests/golden/ip_rank_workspace_layout.json and against the documented region order, and
the argument checks and the host ladder of FlatIPIndex.rank_rows against a scripted pass."""
import json
import os

import numpy as np
import pytest
import torch

from convdr_amd import _lib
from convdr_amd import search as S
from tests import capi_decl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, OVERFLOW, RANGE = 0, 1, 4
ENTRIES = ("convdr_ip_score_rows", "convdr_ip_rank_workspace_bytes", "convdr_ip_rank_rows")


def test_header_ctypes_and_exports_agree_on_the_entries():
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.exported_symbols() and hasattr(L, name)
        assert len(capi_decl.params(name).split(",")) == len(_lib._SIGNATURES[name][1]), name


def _rank(L, store=1, np_=5, scale=4.0, centre=None, n=100000, d=768, cap=4096, bits=None, words=0, n_allowed=0):
    """Every pointer but the centre and the bitmap (neither is dereferenced on the host) is NULL and the workspace has 0 bytes:
    a call that got past validation could not return these messages."""
    return L.convdr_ip_rank_rows(store, None, np_, None, None, None, scale, centre, n, d, None, bits, words, n_allowed, cap, None, 0,
                                 None, None, None, None, None, None)


@pytest.mark.parametrize("store", [0, 1, 2])
def test_every_refusal_of_the_rank_entry_is_a_negative_code_with_a_message(store):
    L = _lib.lib()
    words = (100000 + 255) // 256 * 8
    cases = [
        ({"store": 3}, b"store must be"),
        ({"store": -1}, b"store must be"),
        ({"cap": 5000}, b"cap must be a power of two"),
        ({"cap": 512}, b"cap must be a power of two"),
        ({"cap": 262144}, b"cap must be a power of two"),
        ({"d": 70}, b"d % 64"),
        ({"d": 4160}, b"d <= 4096"),
        ({"n": 1 << 31}, b"bad block size"),
        ({"n": -1}, b"bad block size"),
        ({"np_": 0}, b"bad sizes"),
        ({"bits": (1 << 20) + 4, "words": words}, b"16-byte aligned"),
        ({"bits": 1 << 20, "words": words - 8}, b"the bitmap holds"),
        ({"bits": None, "words": 8}, b"row_bits is NULL"),
        ({"bits": 1 << 20, "words": words, "n_allowed": 100001}, b"n_allowed"),
        ({"bits": 1 << 20, "words": words, "n_allowed": -1}, b"n_allowed"),
    ]
    if store != 0:
        cases += [({"scale": 0.75}, b"power of two"), ({"scale": float("inf")}, b"power of two")]
    if store == 2:
        cases += [({"scale": 0.5}, b"power of two >= 1"), ({"centre": 1 << 20}, b"no centre")]
    for kw, msg in cases:
        rc = _rank(L, **{"store": store, **kw})
        assert rc < 0 and msg in L.convdr_last_error(), (kw, rc, L.convdr_last_error())
        assert b"convdr_ip_rank_rows" in L.convdr_last_error()
    # the first check past all of them
    for kw in ({}, {"bits": 1 << 20, "words": words, "n_allowed": 7}, {"cap": 1024}, {"cap": 131072}, {"n": 0}):
        assert _rank(L, store=store, **kw) < 0 and b"workspace too small" in L.convdr_last_error(), kw


def test_every_refusal_of_the_score_entry():
    L = _lib.lib()

    def call(store=0, nq=3, scale=1.0, n=1000, d=64, m=2, ld=2, q=None, rows=None):
        return L.convdr_ip_score_rows(store, q, nq, None, None, scale, n, d, rows, m, ld, None, None, None)
    for kw, msg in (({"store": 3}, b"store must be"), ({"nq": -1}, b"bad sizes"), ({"m": -1}, b"bad sizes"), ({"ld": 1}, b"ld >= m"),
                    ({"n": 1 << 31}, b"bad block size"), ({"n": -1}, b"bad block size"), ({"d": 70}, b"d % 64"),
                    ({"d": 8192}, b"d <= 4096"), ({"store": 2, "scale": 0.5}, b"power of two >= 1"),
                    ({"store": 1, "scale": 3.0}, b"power of two"), ({}, b"NULL argument"),
                    ({"q": 1 << 20, "rows": 1 << 20}, b"NULL block pointer"), ({"store": 2, "q": 1 << 20, "rows": 1 << 20}, b"NULL block pointer")):
        rc = call(**kw)
        assert rc < 0 and msg in L.convdr_last_error() and b"convdr_ip_score_rows" in L.convdr_last_error(), (kw, L.convdr_last_error())
    assert call(nq=0) == 0 and call(m=0, ld=0) == 0                     # nothing to do: no pointer is looked at
    assert call(n=0, q=1 << 20, rows=1 << 20) == 0                      # both outputs NULL: nothing to do either


def _plan_total(np_, n, d, cap):
    """the documented region order (include/convdr_hip.h), every region rounded up to 256 bytes"""
    tl = 256 if np_ > 128 else 128
    nq_pad = (np_ + tl - 1) // tl * tl
    regions = [nq_pad * d * 2, nq_pad * 4, nq_pad * 4, nq_pad * 4, nq_pad * 32 * 4, nq_pad * 32 * 4, nq_pad * 4, nq_pad * 4,
               np_ * cap * 4, np_ * cap * 4, np_ * cap * 8]
    return sum((r + 255) // 256 * 256 for r in regions)


def test_workspace_bytes_zero_outside_the_contract_and_the_recorded_layout():
    L = _lib.lib()
    ws = L.convdr_ip_rank_workspace_bytes
    for args, msg in (((0, 100, 64, 4096), b"bad sizes"), ((-1, 100, 64, 4096), b"bad sizes"), ((5, -1, 64, 4096), b"bad block size"),
                      ((5, 1 << 31, 64, 4096), b"bad block size"), ((5, 100, 70, 4096), b"d % 64"), ((5, 100, 0, 4096), b"d % 64"),
                      ((5, 100, 4160, 4096), b"d <= 4096"), ((5, 100, 64, 512), b"cap must be"), ((5, 100, 64, 5000), b"cap must be"),
                      ((5, 100, 64, 262144), b"cap must be")):
        assert ws(*args) == 0 and msg in L.convdr_last_error() and b"convdr_ip_rank_rows" in L.convdr_last_error(), args
    assert ws(5, 0, 64, 1024) > 0                           # an empty block is inside the contract
    with open(os.path.join(ROOT, "tests", "golden", "ip_rank_workspace_layout.json")) as f:
        rec = json.load(f)["convdr_ip_rank_workspace_bytes"]
    assert len(rec) > 300 and any(r[-1] == 0 for r in rec) and any(r[-1] > 0 for r in rec)
    for *args, want in rec:
        assert ws(*args) == want, (args, want)
        if want:
            assert want == _plan_total(*args), args


# ---- the Python argument checks and the host ladder against a scripted pass ----------------------------------------------
class RankStub(S.FlatIPIndex):
    """FlatIPIndex with the attributes rank_rows / score_rows read before any device work; _rank_pass is a recorder.
    `band[t]` is the band count the scan reports for target t: a pass at `cap` answers OK with rank 10 t when band[t] <= cap,
    OVERFLOW with the count otherwise."""

    def __init__(self, band, cap=4096, kind="f16", n=1000, range_first=0):
        self.device = torch.device("cpu")
        self.kind, self._store = kind, S.STORES["fp32"]
        self.cap, self._n = int(cap), int(n)
        self.d = self.d_in = 64
        self.stats = {}
        self.band = np.asarray(band, np.int64)
        self.trace, self.range_first = [], range_first

    def _rank_pass(self, qp, tp, cap, allowed=None):
        t = tp.numpy()
        assert qp.shape == (len(t), 64) and tp.dtype == torch.int64
        assert (qp[:, 0].long().numpy()[t >= 0] == t[t >= 0] // 100).all()          # every pair carries its own query
        self.trace.append(["pass", t.tolist(), int(cap)])
        X = torch.zeros(len(t), dtype=torch.float64)
        if self.range_first:
            self.range_first -= 1
            return np.full(len(t), -1), np.zeros(len(t), np.int64), np.zeros(len(t), np.int64), np.full(len(t), RANGE, np.int32), X
        valid = t >= 0
        h = np.where(valid, self.band[np.maximum(t, 0)], 0)
        st = np.where(h > cap, OVERFLOW, OK).astype(np.int32)
        rank = np.where(valid & (st == OK), 10 * t, -1)
        return rank, h, np.where(valid, 7, 0), st, X

    def _rebuild_scaled(self):
        self.trace.append(["rebuild"])


def _queries(nq):
    q = torch.zeros((nq, 64), dtype=torch.float32)
    q[:, 0] = torch.arange(nq)
    return q


def test_argument_checks_raise_value_error_before_any_device_work():
    idx = RankStub(np.zeros(1000, np.int64))
    q = _queries(3)
    for call in (idx.rank_rows, idx.rank_rows_tensors, idx.score_rows, idx.score_rows_tensors):
        for bad in (np.zeros(2, np.int64), np.zeros((4, 2), np.int64), np.zeros((3, 2, 2), np.int64), np.int64(5),
                    np.zeros(3, np.float32), np.zeros(3, bool)):
            with pytest.raises(ValueError):
                call(q, bad)
        for bad in (np.array([0, 1000, 5]), np.array([[0, 1], [2, 3], [4, 1 << 40]]), torch.tensor([999, 1000, -1])):
            with pytest.raises(ValueError, match="ntotal"):
                call(q, bad)
        with pytest.raises(ValueError):
            call(torch.zeros((3, 65)), np.zeros(3, np.int64))
    for call in (idx.rank_rows, idx.rank_rows_tensors):
        with pytest.raises(ValueError, match="stale"):
            call(q, np.zeros(3, np.int64), allowed=S.RowFilter(torch.zeros(32, dtype=torch.int32), 999, 5))
        with pytest.raises(ValueError):
            call(q, np.zeros(3, np.int64), allowed=np.ones(999, bool))
    assert idx.trace == []


def test_pairs_are_expanded_and_the_ladder_jumps_to_the_reported_count():
    band = np.zeros(1000, np.int64)
    band[[105, 201, 202, 203]] = [4097, 8192, 20000, 131073]
    idx = RankStub(band)
    rows = np.array([[3, -1], [105, 199], [201, 202]])      # the test's targets carry their query number in the hundreds
    rows[0, 0] = 3
    got = idx.rank_rows(_queries(3), rows)
    assert got.dtype == np.int64 and got.shape == (3, 2)
    assert idx.trace == [["pass", [3, -1, 105, 199, 201, 202], 4096], ["pass", [105, 201], 8192], ["pass", [202], 32768]], idx.trace
    np.testing.assert_array_equal(got, np.where(rows >= 0, 10 * rows, -1))
    assert idx.stats["rank_rounds"] == 3 and idx.stats["rank_cap"] == 32768 and idx.stats["rank_fallback_pairs"] == 0
    assert idx.stats["rank_band_rows"] == (4096 + 4096 + 4096) + (4097 + 8192) + 20000      # every entry re-scored, all passes
    assert idx.stats["rank_above"] == 7 * 5
    # 1-D rows: one target per query, no pass beyond the first when nothing overflows
    idx = RankStub(band)
    got = idx.rank_rows_tensors(_queries(3), torch.tensor([7, 150, 299]))
    assert got.tolist() == [70, 1500, 2990] and len(idx.trace) == 1 and idx.stats["rank_rounds"] == 1
    # an empty index: nothing enqueued, every rank -1
    idx = RankStub(band, n=0)
    assert idx.rank_rows(_queries(2), np.array([-1, -1])).tolist() == [-1, -1] and idx.trace == []


def test_ladder_rebuilds_once_on_range():
    idx = RankStub(np.zeros(1000, np.int64), range_first=1)
    assert idx.rank_rows(_queries(2), np.array([5, 150])).tolist() == [50, 1500]
    assert [t[0] for t in idx.trace] == ["pass", "rebuild", "pass"] and idx.stats["rescaled"] == 1
    with pytest.raises(_lib.ConvdrError):
        RankStub(np.zeros(1000, np.int64), range_first=2).rank_rows(_queries(1), np.array([5]))
    with pytest.raises(_lib.ConvdrError):
        RankStub(np.zeros(1000, np.int64), kind="bf16", range_first=1).rank_rows(_queries(1), np.array([5]))


def test_a_status_that_is_neither_ok_nor_overflow_raises_after_one_pass():
    idx = RankStub(np.zeros(1000, np.int64))

    def too_few(qp, tp, cap, allowed=None):
        idx.trace.append(["pass", tp.tolist(), int(cap)])
        z = np.zeros(len(tp), np.int64)
        return z - 1, z, z, np.asarray([OK, S.STATUS_TOO_FEW], np.int32), torch.zeros(len(tp), dtype=torch.float64)
    idx._rank_pass = too_few
    with pytest.raises(_lib.ConvdrError, match="convdr_ip_rank_rows: unexpected status"):
        idx.rank_rows(_queries(2), np.array([5, 150]))
    assert idx.trace == [["pass", [5, 150], 4096]]


@pytest.mark.parametrize("x", [0.1, 0.7, 0.0, -3.0])       # float32(x) above x, below x, and equal to x twice
def test_a_band_beyond_range_max_cap_is_handed_to_the_fallback(x):
    """One target whose band holds 131,073 rows: no list holds it, so the pair goes to range_search_tensors just below the
    target's score and the rows that come back are compared by their canonical scores.  Both are recorders here."""
    t = 50
    band = np.zeros(1000, np.int64)
    band[t] = 131073
    idx = RankStub(band)
    ranked = idx._rank_pass
    calls = []

    def rank_pass(qp, tp, cap, allowed=None):
        return ranked(qp, tp, cap, allowed)[:4] + (torch.full((len(tp),), x, dtype=torch.float64),)

    def range_search_tensors(q, radius, allowed=None):
        calls.append(["range", q[:, 0].tolist(), radius, allowed])
        idx.stats = {"range_results": 4, "range_rounds": 1, "range_cap": 4096, "range_chunked_queries": 0, "rescaled": 0}
        return torch.tensor([0, 4]), torch.zeros(4), torch.tensor([3, t, 70, 900])

    def score_rows_tensors(q, rows):
        calls.append(["score", q[:, 0].tolist(), rows.tolist()])
        X = torch.tensor([[x, x, x, x + 1.0]], dtype=torch.float64)     # row 3 ties below the target, 70 above it; 900 beats it
        return X.float(), X
    idx._rank_pass, idx.range_search_tensors, idx.score_rows_tensors = rank_pass, range_search_tensors, score_rows_tensors
    got = idx.rank_rows_tensors(_queries(1), np.array([t]))
    assert got.tolist() == [2]
    assert idx.trace == [["pass", [t], 4096]]
    assert [c[0] for c in calls] == ["range", "score"] and calls[1] == ["score", [0.0], [[3, t, 70, 900]]]
    _, qs, r, allowed = calls[0]
    assert qs == [0.0] and allowed is None
    assert isinstance(r, np.float32) and np.float64(r) < x <= np.float64(np.nextafter(r, np.float32(np.inf)))
    assert idx.stats == {"rank_rounds": 1, "rank_cap": 4096, "rank_band_rows": 4096, "rank_above": 0, "rank_fallback_pairs": 1,
                         "rescaled": 0}
    assert not [k for k in idx.stats if k.startswith("range_")]
