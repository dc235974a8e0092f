"""Document rank, the parts that need no GPU: the entries are declared and exported, every refusal of convdr_ip_rank_docs /
convdr_doc_ordinals / the two workspace functions (argument validation happens before anything touches a device), the
workspace totals against tests/golden/ip_rank_docs_workspace_layout.json and against the documented region order, the argument
checks and the host ladder of FlatIPIndex.rank_ids against a scripted pass, and the oracle against its brute restatement."""
import json
import os

import numpy as np
import pytest
import torch

from convdr_amd import _lib
from convdr_amd import search as S
from tests import capi_decl
from tests import doc_cases as DC
from tests import doc_rank_cases as RC
from tests import key_cases as K
from tests.golden.make_golden import synth_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, OVERFLOW, RANGE = 0, 1, 4
ENTRIES = ("convdr_doc_ordinals_workspace_bytes", "convdr_doc_ordinals", "convdr_ip_rank_docs_workspace_bytes", "convdr_ip_rank_docs")
FAKE = 1 << 20          # a pointer that is never dereferenced on the host


def test_header_ctypes_and_exports_agree_on_the_entries():
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.exported_symbols() and hasattr(L, name)
        assert len(capi_decl.params(name).split(",")) == len(_lib._SIGNATURES[name][1]), name


def _rank(L, store=1, np_=5, scale=4.0, centre=None, n=100000, d=768, cap=4096, bits=None, words=0, n_allowed=0, ord_=None, ndocs=1000,
          ws=None, ws_bytes=0, ptrs=None):
    """Every pointer but those named is NULL and the workspace has 0 bytes: a call that got past validation could not return
    these messages."""
    return L.convdr_ip_rank_docs(store, ptrs, np_, ptrs, None, None, scale, centre, n, d, None, bits, words, n_allowed, ord_, ndocs, cap,
                                 ws, ws_bytes, ptrs, ptrs, ptrs, ptrs, ptrs, None)


@pytest.mark.parametrize("store", [0, 1, 2])
def test_every_refusal_of_the_rank_docs_entry_is_a_negative_code_with_a_message(store):
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
        ({"ndocs": -1}, b"ndocs=-1 outside"),
        ({"ndocs": 100001}, b"ndocs=100001 outside"),
        ({"n": 0, "ndocs": 1}, b"ndocs=1 outside"),
    ]
    if store != 0:
        cases += [({"scale": 0.75}, b"power of two"), ({"scale": float("inf")}, b"power of two")]
    if store == 2:
        cases += [({"scale": 0.5}, b"power of two >= 1"), ({"centre": 1 << 20}, b"no centre")]
    for kw, msg in cases:
        rc = _rank(L, **{"store": store, **kw})
        assert rc < 0 and msg in L.convdr_last_error(), (kw, rc, L.convdr_last_error())
        assert b"convdr_ip_rank_docs" in L.convdr_last_error()
    # the first check past all of them
    for kw in ({}, {"bits": 1 << 20, "words": words, "n_allowed": 7}, {"cap": 1024}, {"cap": 131072}, {"n": 0, "ndocs": 0},
               {"ndocs": 0}, {"ndocs": 100000}):
        assert _rank(L, store=store, **kw) < 0 and b"workspace too small" in L.convdr_last_error(), kw
        assert b"convdr_ip_rank_docs" in L.convdr_last_error()
    # with a workspace that is large enough: the NULL arguments, then ord -- which only an empty block may leave out
    need = L.convdr_ip_rank_docs_workspace_bytes(5, 100000, 768, 4096, 1000)
    assert _rank(L, store=store, ws=FAKE, ws_bytes=need) < 0 and b"NULL argument" in L.convdr_last_error()
    assert _rank(L, store=store, ws=FAKE, ws_bytes=need, ptrs=FAKE) < 0 and b"ord is NULL" in L.convdr_last_error()
    assert b"convdr_ip_rank_docs" in L.convdr_last_error()
    assert _rank(L, store=store, ws=FAKE, ws_bytes=need, ptrs=FAKE, ord_=FAKE) < 0 and b"NULL block pointer" in L.convdr_last_error()


def test_every_refusal_of_the_ordinals_entry():
    L = _lib.lib()

    def call(n=1000, col=FAKE, ws=FAKE, ws_bytes=1 << 40, ord_=FAKE, ndocs=FAKE):
        return L.convdr_doc_ordinals(col, n, ws, ws_bytes, ord_, ndocs, None)
    for kw, msg in (({"n": -1}, b"bad list length"), ({"n": (1 << 27) + 1}, b"bad list length"), ({"col": None}, b"NULL argument"),
                    ({"ord_": None}, b"NULL argument"), ({"ws": None}, b"NULL argument"), ({"ndocs": None}, b"NULL argument"),
                    ({"n": 0, "ws": None}, b"NULL argument"), ({"n": 0, "ndocs": None}, b"NULL argument"),
                    ({"ws_bytes": L.convdr_doc_ordinals_workspace_bytes(1000) - 1}, b"workspace too small"),
                    ({"n": 0, "col": None, "ord_": None, "ws_bytes": 0}, b"workspace too small")):
        rc = call(**kw)
        assert rc < 0 and msg in L.convdr_last_error() and b"convdr_doc_ordinals" in L.convdr_last_error(), (kw, L.convdr_last_error())


def _rank_total(np_, n, d, cap):
    """the rank plan's documented region order (tests/test_rank_rows_cpu.py), every region rounded up to 256 bytes"""
    tl = 256 if np_ > 128 else 128
    nq_pad = (np_ + tl - 1) // tl * tl
    regions = [nq_pad * d * 2, nq_pad * 4, nq_pad * 4, nq_pad * 4, nq_pad * 32 * 4, nq_pad * 32 * 4, nq_pad * 4, nq_pad * 4,
               np_ * cap * 4, np_ * cap * 4, np_ * cap * 8]
    return sum((r + 255) // 256 * 256 for r in regions)


def _docs_total(np_, n, d, cap, ndocs):
    """... followed by the bitmap: np x mark_words words, mark_words = ceil(ndocs / 32) rounded up to 32"""
    mark_words = ((ndocs + 31) // 32 + 31) // 32 * 32
    return _rank_total(np_, n, d, cap) + (np_ * mark_words * 4 + 255) // 256 * 256


def _ordinals_total(n):
    """key set (256 + 20 S) | head 256 | document number per slot u32 [S] | block sums u32 [ceil(n / 256)]"""
    slots = 64
    while slots < 2 * n:
        slots *= 2
    return sum((r + 255) // 256 * 256 for r in (256 + 20 * slots, 256, 4 * slots, 4 * ((n + 255) // 256)))


def test_workspace_bytes_zero_outside_the_contract_and_the_recorded_layout():
    L = _lib.lib()
    ws = L.convdr_ip_rank_docs_workspace_bytes
    for args, msg in (((0, 100, 64, 4096, 10), b"bad sizes"), ((-1, 100, 64, 4096, 10), b"bad sizes"), ((5, -1, 64, 4096, 0), b"bad block size"),
                      ((5, 1 << 31, 64, 4096, 10), b"bad block size"), ((5, 100, 70, 4096, 10), b"d % 64"), ((5, 100, 0, 4096, 10), b"d % 64"),
                      ((5, 100, 4160, 4096, 10), b"d <= 4096"), ((5, 100, 64, 512, 10), b"cap must be"), ((5, 100, 64, 5000, 10), b"cap must be"),
                      ((5, 100, 64, 262144, 10), b"cap must be"), ((5, 100, 64, 4096, -1), b"ndocs"), ((5, 100, 64, 4096, 101), b"ndocs"),
                      ((5, 0, 64, 4096, 1), b"ndocs")):
        assert ws(*args) == 0 and msg in L.convdr_last_error() and b"convdr_ip_rank_docs" in L.convdr_last_error(), args
    assert ws(5, 0, 64, 1024, 0) == L.convdr_ip_rank_workspace_bytes(5, 0, 64, 1024) > 0          # an empty block is inside the contract
    wo = L.convdr_doc_ordinals_workspace_bytes
    for n in (-1, (1 << 27) + 1):
        assert wo(n) == 0 and b"convdr_doc_ordinals" in L.convdr_last_error(), n
    with open(os.path.join(ROOT, "tests", "golden", "ip_rank_docs_workspace_layout.json")) as f:
        rec = json.load(f)
    docs, ords = rec["convdr_ip_rank_docs_workspace_bytes"], rec["convdr_doc_ordinals_workspace_bytes"]
    assert len(docs) > 300 and any(r[-1] == 0 for r in docs) and any(r[-1] > 0 for r in docs)
    for *args, want in docs:
        assert ws(*args) == want, (args, want)
        if want:
            assert want == _docs_total(*args), args
    assert len(ords) > 20 and any(r[-1] == 0 for r in ords)
    for n, want in ords:
        assert wo(n) == want, (n, want)
        if want:
            assert want == _ordinals_total(n), n


# ---- the Python argument checks and the host ladder against a scripted pass ----------------------------------------------
class DocRankStub(S.FlatIPIndex):
    """FlatIPIndex with the attributes rank_ids reads before any device work; score_ids_tensors, doc_ordinals and
    _rank_docs_pass are recorders.  The id of row r is 3 r unless `col` says otherwise; `band[t]` is the band count the scan
    reports for target row t: a pass at `cap` answers OK with rank 10 t when band[t] <= cap, OVERFLOW with the count otherwise."""

    def __init__(self, band, cap=4096, kind="f16", n=1000, range_first=0, col=None):
        self.device = torch.device("cpu")
        self.kind, self._store = kind, S.STORES["fp32"]
        self.cap, self._n = int(cap), int(n)
        self.d = self.d_in = 64
        self.stats = {}
        self.band = np.asarray(band, np.int64)
        self.trace, self.range_first = [], range_first
        self.col = np.arange(n, dtype=np.int64) * 3 if col is None else col
        self._sid = torch.from_numpy(self.col.copy())

    def score_ids_tensors(self, q, ids):
        it = torch.as_tensor(ids)
        R = np.asarray([next((r for r, c in enumerate(self.col) if c == k), -1) for k in it.reshape(-1).tolist()], np.int64)
        self.trace.append(["score_ids", R.tolist()])
        return torch.zeros(tuple(it.shape)), torch.from_numpy(R).reshape(tuple(it.shape))

    def doc_ordinals(self):
        self.trace.append(["ordinals"])
        return S.DocOrdinals(torch.zeros(self._n, dtype=torch.int32), len(np.unique(self.col)), self._n)

    def _rank_docs_pass(self, qp, tp, cap, ordinals, allowed=None):
        t = tp.numpy()
        assert qp.shape == (len(t), 64) and tp.dtype == torch.int64 and isinstance(ordinals, S.DocOrdinals) and ordinals.n == self._n
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
    idx = DocRankStub(np.zeros(1000, np.int64))
    q = _queries(3)
    ids = np.zeros(3, np.int64)
    for call in (idx.rank_ids, idx.rank_ids_tensors):
        for bad in (np.zeros(2, np.int64), np.zeros((4, 2), np.int64), np.zeros((3, 2, 2), np.int64), np.int64(5),
                    np.zeros(3, np.float32), np.zeros(3, bool), np.zeros(3, np.int32)):
            with pytest.raises(ValueError, match="rank_ids"):
                call(q, bad)
        with pytest.raises(ValueError, match="rank_ids"):
            call(torch.zeros((3, 65)), ids)
        with pytest.raises(ValueError, match="stale RowFilter"):
            call(q, ids, allowed=S.RowFilter(torch.zeros(32, dtype=torch.int32), 999, 5))
        with pytest.raises(ValueError):
            call(q, ids, allowed=np.ones(999, bool))
        with pytest.raises(ValueError, match="stale DocOrdinals"):
            call(q, ids, ordinals=S.DocOrdinals(torch.zeros(999, dtype=torch.int32), 10, 999))
        with pytest.raises(ValueError, match="DocOrdinals"):
            call(q, ids, ordinals=torch.zeros(1000, dtype=torch.int32))
    assert idx.trace == []
    idx._sid = None
    with pytest.raises(ValueError, match="no row ids"):
        idx.rank_ids(q, ids)
    with pytest.raises(ValueError, match="no row ids"):
        S.FlatIPIndex.doc_ordinals(idx)
    assert idx.trace == []


def test_pairs_are_expanded_and_the_ladder_jumps_to_the_reported_count():
    band = np.zeros(1000, np.int64)
    band[[105, 201, 202, 203]] = [4097, 8192, 20000, 131073]
    idx = DocRankStub(band)
    rows = np.array([[3, -1], [105, 199], [201, 202]])      # the test's target rows carry their query number in the hundreds
    ids = np.where(rows >= 0, 3 * rows, 7)                  # (7 is the id of no row)
    got = idx.rank_ids(_queries(3), ids)
    assert got.dtype == np.int64 and got.shape == (3, 2)
    assert idx.trace == [["score_ids", [3, -1, 105, 199, 201, 202]], ["ordinals"], ["pass", [3, -1, 105, 199, 201, 202], 4096],
                         ["pass", [105, 201], 8192], ["pass", [202], 32768]], idx.trace
    np.testing.assert_array_equal(got, np.where(rows >= 0, 10 * rows, -1))
    assert idx.stats["rank_rounds"] == 3 and idx.stats["rank_cap"] == 32768 and idx.stats["rank_fallback_pairs"] == 0
    assert idx.stats["rank_band_rows"] == (4096 + 4096 + 4096) + (4097 + 8192) + 20000      # every entry re-scored, all passes
    assert idx.stats["rank_above"] == 7 * 5 and idx.stats["ndocs"] == 1000 and idx.stats["rescaled"] == 0
    # 1-D ids and given ordinals: one target per query, no ordinals pass, no pass beyond the first when nothing overflows
    idx = DocRankStub(band)
    o = S.DocOrdinals(torch.zeros(1000, dtype=torch.int32), 321, 1000)
    rank, D, R = idx.rank_ids_tensors(_queries(3), torch.tensor([21, 450, 897]), ordinals=o)
    assert rank.tolist() == [70, 1500, 2990] and R.tolist() == [7, 150, 299] and tuple(D.shape) == (3,)
    assert [t[0] for t in idx.trace] == ["score_ids", "pass"] and idx.stats["rank_rounds"] == 1 and idx.stats["ndocs"] == 321
    # an empty index: no pass, every rank -1
    idx = DocRankStub(band, n=0)
    assert idx.rank_ids(_queries(2), np.array([5, 6])).tolist() == [-1, -1] and not [t for t in idx.trace if t[0] == "pass"]


def test_ladder_rebuilds_once_on_range():
    idx = DocRankStub(np.zeros(1000, np.int64), range_first=1)
    assert idx.rank_ids(_queries(2), np.array([15, 450])).tolist() == [50, 1500]
    assert [t[0] for t in idx.trace] == ["score_ids", "ordinals", "pass", "rebuild", "pass"] and idx.stats["rescaled"] == 1
    with pytest.raises(_lib.ConvdrError, match="convdr_ip_rank_docs"):
        DocRankStub(np.zeros(1000, np.int64), range_first=2).rank_ids(_queries(1), np.array([15]))
    with pytest.raises(_lib.ConvdrError, match="convdr_ip_rank_docs"):
        DocRankStub(np.zeros(1000, np.int64), kind="bf16", range_first=1).rank_ids(_queries(1), np.array([15]))


@pytest.mark.parametrize("x", [0.1, 0.7, 0.0, -3.0])       # float32(x) above x, below x, and equal to x twice
def test_a_band_beyond_range_max_cap_takes_the_fallback_which_drops_the_targets_own_id(x):
    """One target whose band holds 131,073 rows: the pair goes to range_search_tensors just below the target's score; of the
    rows that come back, those that precede the target give their ids, the target's own id is dropped, the rest is counted
    once per id.  Both device calls are recorders here."""
    t = 50
    band = np.zeros(1000, np.int64)
    band[t] = 131073
    col = np.arange(1000, dtype=np.int64) * 3
    col[900] = col[3]           # two rows of one document precede the target: counted once
    col[71] = col[t]            # a row of the target's own document that beats its ... recorded best row: dropped
    idx = DocRankStub(band, col=col)
    ranked = idx._rank_docs_pass
    calls = []

    def rank_pass(qp, tp, cap, ordinals, allowed=None):
        return ranked(qp, tp, cap, ordinals, allowed)[:4] + (torch.full((len(tp),), x, dtype=torch.float64),)

    def range_search_tensors(q, radius, allowed=None):
        calls.append(["range", q[:, 0].tolist(), radius, allowed])
        idx.stats = {"range_results": 6, "range_rounds": 1, "range_cap": 4096, "range_chunked_queries": 0, "rescaled": 0}
        return torch.tensor([0, 6]), torch.zeros(6), torch.tensor([3, t, 70, 900, 71, 40])

    def score_rows_tensors(q, rows):
        calls.append(["score", q[:, 0].tolist(), rows.tolist()])
        # row 3 ties below the target, 70 ties above it; 900 and 71 beat it; 40 ties below it: a second document
        X = torch.tensor([[x, x, x, x + 1.0, x + 2.0, x]], dtype=torch.float64)
        return X.float(), X
    idx._rank_docs_pass, idx.range_search_tensors, idx.score_rows_tensors = rank_pass, range_search_tensors, score_rows_tensors
    got, _, R = idx.rank_ids_tensors(_queries(1), np.array([col[t]]))
    assert got.tolist() == [2] and R.tolist() == [t]
    assert [c[0] for c in idx.trace] == ["score_ids", "ordinals", "pass"]
    assert [c[0] for c in calls] == ["range", "score"] and calls[1] == ["score", [0.0], [[3, t, 70, 900, 71, 40]]]
    _, qs, r, allowed = calls[0]
    assert qs == [0.0] and allowed is None
    assert isinstance(r, np.float32) and np.float64(r) < x <= np.float64(np.nextafter(r, np.float32(np.inf)))
    assert idx.stats == {"rank_rounds": 1, "rank_cap": 4096, "rank_band_rows": 4096, "rank_above": 0, "rank_fallback_pairs": 1,
                         "rescaled": 0, "ndocs": 998}


# ---- the oracle against its brute restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("column", ["chunked_ids", "interleaved"])
def test_the_oracle_equals_the_walk_over_the_canonical_order(column):
    n, nq = 400, 3
    col = DC.chunked_ids(n) if column == "chunked_ids" else np.array(DC.interleaved(n))
    P = synth_corpus(41, n, 64).astype(np.float16).astype(np.float32)
    P[[10, 20, 390]] = P[200]                   # exact ties across documents
    Q = synth_corpus(42, nq, 64)
    Q[2] = 0                                    # every score ties
    from oracle import search as OS
    Sx = OS.canonical_scores(Q, P)
    rs = np.random.RandomState(5)
    mask = rs.rand(n) < 0.5
    keys = list(np.unique(col)[::7]) + [int(col[200]), int(col[10]), int(col[390]), 123_456_789, K.I64_MIN]
    if column == "interleaved":
        keys.append(DC.BIG_ID)
    for j in range(nq):
        for m in (None, mask):
            for k in keys:
                assert RC.rank(Sx[j], col, int(k), m) == RC.brute_rank(Sx[j], col, int(k), m), (j, k, m is None)
    assert RC.rank(Sx[0], col, 123_456_789) == -1 and RC.rank(Sx[0], col, K.I64_MIN) == -1
    want, ndocs = RC.ordinals(col)
    seen = {}
    for r, k in enumerate(col.tolist()):
        seen.setdefault(k, len(seen))
        assert want[r] == seen[k]
    assert ndocs == len(seen) and want.dtype == np.uint32
    # the zero query without a mask: the rank of a document is its ordinal
    for k in keys[:20]:
        assert RC.rank(Sx[2], col, int(k)) == want[np.flatnonzero(col == k)[0]]
