"""Documents by id, the parts that need no GPU: the four entries are declared and exported, the size function against the
documented regions, every refusal (argument validation happens before anything touches a device), the id checks of the new
FlatIPIndex methods against a scripted index, and the oracle of tests/doc_cases.py against brute force."""

import numpy as np
import pytest
import torch

from convdr_amd import _lib
from convdr_amd import search as S
from tests import capi_decl
from tests import doc_cases as DC
from tests import key_cases as K

ENTRIES = ("convdr_keys_rows_workspace_bytes", "convdr_keys_rows_count", "convdr_keys_rows_fill", "convdr_ip_score_docs")
METHODS = ("rows_all", "score_ids", "score_ids_tensors", "search_docs", "reconstruct_docs", "upsert_docs")
P = 1 << 20                     # a pointer that is never dereferenced on the host (16-byte aligned)
N = 100000
BIG = 1 << 40                   # a workspace size that fits every call


def test_header_ctypes_and_exports_agree_on_the_entries():
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.exported_symbols() and hasattr(L, name)
        assert len(capi_decl.params(name).split(",")) == len(_lib._SIGNATURES[name][1]), name


def _slots(m):
    s = 64
    while s < 2 * m:
        s *= 2
    return s


def _up(b):
    return (b + 255) // 256 * 256


def _total(m, rows_cap):
    """the documented region order (include/convdr_hip.h, "Documents by id": workspace): the key set's regions | head |
    segment starts | cursors | block sums | list A | list B, each on a 256-byte boundary"""
    s = _slots(m)
    return (256 + 20 * s) + 256 + 4 * s + 4 * s + _up(4 * ((m + 255) // 256)) + _up(8 * rows_cap) + _up(8 * rows_cap)


def test_workspace_bytes_follow_the_documented_regions_and_are_zero_outside_the_contract():
    L = _lib.lib()
    ws = L.convdr_keys_rows_workspace_bytes
    for m in (0, 1, 32, 33, 256, 257, 5000, 100000, 1 << 27):
        for cap in (0, 1, 31, 32, 33, 5000, 1 << 20, (1 << 31) - 1):
            assert ws(m, cap) == _total(m, cap), (m, cap)
        assert ws(m, 0) >= L.convdr_keyset_workspace_bytes(m) == 256 + 20 * _slots(m)       # (the set's size is what it was)
    for m in (-1, (1 << 27) + 1, 1 << 40):
        assert ws(m, 10) == 0 and b"bad list length" in L.convdr_last_error(), m
    for cap in (-1, 1 << 31, 1 << 40):
        assert ws(10, cap) == 0 and b"bad list capacity" in L.convdr_last_error(), cap


def _refused(L, name, rc, msg):
    err = L.convdr_last_error()
    assert rc < 0 and msg in err and name in err, (name, rc, msg, err)


def test_every_refusal_of_the_count_entry_is_a_negative_code_with_a_message():
    L = _lib.lib()
    name = b"convdr_keys_rows_count"

    def count(row_keys=P, n=N, ws=P, ws_bytes=BIG, keys=P, m=1000, start=P, cnt=P, dup=P, total=P):
        return L.convdr_keys_rows_count(row_keys, n, ws, ws_bytes, keys, m, start, cnt, dup, total, None)
    _refused(L, name, count(m=-1), b"bad list length")
    _refused(L, name, count(m=(1 << 27) + 1), b"bad list length")
    _refused(L, name, count(n=-1), b"bad block size")
    _refused(L, name, count(n=1 << 31), b"bad block size")
    for kw in ({"row_keys": None}, {"ws": None}, {"keys": None}, {"start": None}, {"cnt": None}, {"total": None},
               {"m": 0, "n": 0, "ws": None}, {"m": 0, "n": 0, "total": None}):
        _refused(L, name, count(**kw), b"NULL argument")
    for m in (0, 1, 33, 5000):
        _refused(L, name, count(m=m, ws_bytes=_total(m, 0) - 1), b"workspace too small")
    _refused(L, name, count(m=1000, dup=None, ws_bytes=_total(1000, 0) - 1), b"workspace too small")     # (dup_of is nullable)
    _refused(L, name, count(m=5000, ws_bytes=L.convdr_keyset_workspace_bytes(5000)), b"workspace too small")   # (the set alone)


def test_every_refusal_of_the_fill_entry_is_a_negative_code_with_a_message():
    L = _lib.lib()
    name = b"convdr_keys_rows_fill"

    def fill(row_keys=P, n=N, ws=P, ws_bytes=BIG, m=1000, rows=P, cap=5000):
        return L.convdr_keys_rows_fill(row_keys, n, ws, ws_bytes, m, rows, cap, None)
    _refused(L, name, fill(m=-1), b"bad list length")
    _refused(L, name, fill(m=(1 << 27) + 1), b"bad list length")
    _refused(L, name, fill(n=-1), b"bad block size")
    _refused(L, name, fill(n=1 << 31), b"bad block size")
    _refused(L, name, fill(cap=-1), b"bad list capacity")
    _refused(L, name, fill(cap=1 << 31), b"bad list capacity")
    for kw in ({"row_keys": None}, {"ws": None}, {"rows": None}, {"n": 0, "cap": 0, "ws": None}):
        _refused(L, name, fill(**kw), b"NULL argument")
    for m, cap in ((0, 0), (1, 1), (33, 5000), (5000, 33)):
        _refused(L, name, fill(m=m, cap=cap, ws_bytes=_total(m, cap) - 1), b"workspace too small")
    _refused(L, name, fill(m=1000, cap=5000, ws_bytes=_total(1000, 0)), b"workspace too small")          # (the count's size)


def test_every_refusal_of_the_score_entry_is_a_negative_code_with_a_message():
    L = _lib.lib()
    name = b"convdr_ip_score_docs"

    def score(store=1, q=P, nq=3, p32=P, p16=P, scale=1.0, n=N, d=768, rows=P, rows_len=5000, start=P, count=P, m=7, ld=7, X=P,
              D=P, R=P):
        return L.convdr_ip_score_docs(store, q, nq, p32, p16, scale, n, d, rows, rows_len, start, count, m, ld, X, D, R, None)
    for store in (-1, 3):
        _refused(L, name, score(store=store), b"store must be")
    _refused(L, name, score(nq=-1), b"bad sizes")
    _refused(L, name, score(m=-1), b"bad sizes")
    _refused(L, name, score(ld=6), b"bad sizes")
    _refused(L, name, score(n=-1), b"bad block size")
    _refused(L, name, score(n=1 << 31), b"bad block size")
    for d in (0, 70, 4160):
        _refused(L, name, score(d=d), b"d % 64")
    _refused(L, name, score(rows_len=-1), b"bad list length")
    _refused(L, name, score(scale=3.0), b"power of two")
    _refused(L, name, score(store=2, scale=0.5), b"power of two")
    for kw in ({"q": None}, {"start": None}, {"count": None}, {"rows": None}):
        _refused(L, name, score(**kw), b"NULL argument")
    _refused(L, name, score(p32=None), b"NULL block pointer")
    _refused(L, name, score(store=2, p16=None), b"NULL block pointer")
    # nothing to do: no pair, or no output asked for -- and no launch
    assert score(nq=0, q=None, start=None, count=None, rows=None) == 0
    assert score(m=0, ld=0, q=None, start=None, count=None, rows=None) == 0
    assert score(X=None, D=None, R=None) == 0


# ---- the Python argument checks against a scripted index -------------------------------------------------------------------
class KeyedStub(S.FlatIPIndex):
    """FlatIPIndex with what add(ids=) and the id methods read before any device work, on the CPU"""

    def __init__(self, d=8):
        self.device = torch.device("cpu")
        self._store, self.d_in, self.d = S.STORES["fp32"], d, d
        self._n, self.stats = 0, {}
        self._s32 = self._s16 = self._slo = self._sid = self._sid_spare = None

    def _add_rows(self, x, chunk_bytes=None):
        x = torch.as_tensor(x)
        self._s16 = x.clone() if self._s16 is None else torch.cat([self._s16[:self._n], x])
        self._n += int(x.shape[0])


def _calls(idx, ids, q):
    return (lambda: idx.rows_all(ids), lambda: idx.score_ids(q, ids), lambda: idx.score_ids_tensors(q, ids),
            lambda: idx.search_docs(q, 2), lambda: idx.reconstruct_docs(ids),
            lambda: idx.upsert_docs(ids, np.ones(len(ids), np.int64), torch.zeros(len(ids), 8)))


def test_every_document_method_raises_on_an_index_without_ids():
    idx = KeyedStub()
    idx.add(np.zeros((4, 8), np.float32))
    for call in _calls(idx, np.array([1]), np.zeros((1, 8), np.float32)):
        with pytest.raises(ValueError, match="carries no row ids"):
            call()
    assert idx.ntotal == 4


def test_the_lists_are_checked_before_any_device_work():
    idx = KeyedStub()
    idx.add(np.zeros((3, 8), np.float32), ids=np.array([1, 2, 2]))
    q = np.zeros((2, 8), np.float32)
    for bad in (np.array([1.0]), np.array([1], np.int32), np.array([[1]]), np.array([K.I64_MIN])):
        for call in (idx.rows_all, idx.reconstruct_docs, lambda v: idx.upsert_docs(v, np.ones(1, np.int64), torch.zeros(1, 8))):
            with pytest.raises(ValueError):
                call(bad)
    for bad_ids in (np.array([1.0, 2.0]), np.array([1, 2], np.int32), np.array([1, 2, 3]), np.zeros((2, 2, 2), np.int64)):
        with pytest.raises(ValueError, match="ids must be int64"):
            idx.score_ids_tensors(q, bad_ids)
    with pytest.raises(ValueError, match="queries must be"):
        idx.score_ids_tensors(np.zeros((2, 5), np.float32), np.array([1, 2]))
    ids = np.array([1, 7])
    for counts, emb in ((np.array([1]), torch.zeros(1, 8)), (np.array([1, 0]), torch.zeros(1, 8)), (np.array([1.0, 2.0]), torch.zeros(3, 8)),
                        (np.array([[1, 2]]), torch.zeros(3, 8)), (np.array([1, 2]), torch.zeros(2, 8)),
                        (np.array([1, 2]), torch.zeros(3, 7)), (np.array([1, 2]), torch.zeros(3, 8, dtype=torch.float64)),
                        (np.array([1, 2]), np.zeros((3, 8), np.float32))):
        with pytest.raises(ValueError, match="upsert_docs"):
            idx.upsert_docs(ids, counts, emb)
    assert idx.ntotal == 3 and idx.ids.tolist() == [1, 2, 2]
    assert idx.upsert_docs(np.zeros(0, np.int64), np.zeros(0, np.int64), torch.zeros(0, 8)) == (0, 0, 0)      # an empty list: no device work


def test_without_a_gpu_the_index_and_with_it_the_new_methods_raise_convdr_error():
    for name in METHODS:
        assert callable(getattr(S.FlatIPIndex, name)), name
    if not torch.cuda.is_available():
        with pytest.raises(_lib.ConvdrError, match="no CPU fallback"):
            S.FlatIPIndex(64).rows_all(np.array([1]))


# ---- the oracle against brute force ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", DC.FAMILIES)
def test_the_rows_oracle_agrees_with_brute_force(family):
    for n, m in ((0, 0), (0, 5), (7, 0), (1, 1), (40, 33), (120, 64), (400, 50)):
        col, lst = DC.case(family, n, m)
        assert col.dtype == np.int64 and lst.dtype == np.int64 and col.shape == (n,) and lst.shape == (m,)
        start, count, rows, dup = DC.rows_all(col, lst)
        bs, bc, br = DC.brute_rows_all(col.tolist(), lst.tolist())
        assert np.array_equal(start, bs) and np.array_equal(count, bc) and np.array_equal(rows, br), (family, n, m)
        assert np.array_equal(count, K.locate(col, lst)[1]) and np.array_equal(dup, K.locate(col, lst)[2]), (family, n, m)
        assert len(rows) == sum(int((col == k).sum()) for k in set(lst.tolist()))
        for j in range(m):
            seg = rows[start[j]:start[j] + count[j]]
            assert np.array_equal(seg, np.nonzero(col == lst[j])[0]) and (np.diff(seg) > 0).all()
    # the reserved id is on no row and stands for itself
    col, lst = np.array([5, 6, 5], np.int64), np.array([5, K.I64_MIN, 5, K.I64_MIN], np.int64)
    start, count, rows, dup = DC.rows_all(col, lst)
    assert start.tolist() == [0, 0, 0, 0] and count.tolist() == [2, 0, 2, 0] and rows.tolist() == [0, 2] and dup.tolist() == [0, 1, 0, 3]
    assert [a.tolist() for a in DC.brute_rows_all(col.tolist(), lst.tolist())] == [[0, 0, 0, 0], [2, 0, 2, 0], [0, 2]]


def test_the_interleaved_column_holds_what_it_is_named_for():
    col = DC.interleaved(20000)
    assert int((col == DC.BIG_ID).sum()) == 5000 and not (col == K.I64_MIN).any()
    ids, reps = np.unique(col, return_counts=True)
    triples = ids[reps == 3]
    assert len(triples) > 1000 and sorted(set(reps.tolist())) == [1, 3, 5000]
    r = np.nonzero(col == triples[5])[0]
    assert (r - r[0]).tolist() == [0, 7, 300] and len(set(col[r[0]:r[2]].tolist())) > 100       # other documents lie in between
    assert all(k in col for k in K.EDGE_KEYS)
    col, lst = DC.case("interleaved", 20000, 1000)
    _, count, rows, dup = DC.rows_all(col, lst)
    assert DC.BIG_ID in lst and (count == 0).any() and (count == 3).any() and (dup != np.arange(1000)).any()
    assert any(k in lst for k in K.EDGE_KEYS) and len(rows) > 5000


def test_the_maxp_oracle_agrees_with_brute_force_and_takes_the_lowest_row_on_a_tie():
    rs = np.random.RandomState(3)
    for L in (1, 2, 7, 300):
        rows = np.sort(rs.choice(10000, size=L, replace=False))
        for scores in (rs.randn(L), -np.abs(rs.randn(L)) - 1.0, np.round(rs.randn(L)), np.full(L, -2.5)):
            assert DC.maxp(scores, rows) == DC.brute_maxp(scores.tolist(), rows.tolist())
    assert DC.maxp(np.array([-3.0, -1.0, -1.0]), np.array([4, 9, 11])) == (-1.0, 9)
    assert DC.maxp(np.zeros(0), np.zeros(0, np.int64)) == (None, -1) == DC.brute_maxp([], [])
    ids = DC.chunked_ids(3000)
    reps = np.unique(ids, return_counts=True)[1]
    assert reps.min() >= 1 and reps.max() == 6 and ids.shape == (3000,)
