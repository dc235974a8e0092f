"""Row ids, the parts that need no GPU: the five entries are declared and exported, every refusal (argument validation happens
before anything touches a device), the workspace size against the documented regions, the argument checks of
FlatIPIndex.add(ids=) and of the id methods against a scripted index, and the oracle of tests/key_cases.py against brute force."""

import numpy as np
import pytest
import torch

from convdr_amd import _lib
from convdr_amd import search as S
from tests import capi_decl
from tests import key_cases as K

ENTRIES = ("convdr_keyset_workspace_bytes", "convdr_keyset_build", "convdr_keys_member", "convdr_keys_locate", "convdr_ip_compact_ids")
P = 1 << 20                     # a pointer that is never dereferenced on the host (16-byte aligned)
N = 100000
WORDS = (N + 255) // 256 * 8
BIG = 1 << 40                   # a workspace size that fits every set


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


def _total(m):
    """the documented region order (include/convdr_hip.h, "Row ids": workspace): head | keys | positions | rows | counts"""
    s = _slots(m)
    return 256 + 8 * s + 4 * s + 4 * s + 4 * s


def test_workspace_bytes_follow_the_documented_regions_and_are_zero_outside_the_contract():
    L = _lib.lib()
    ws = L.convdr_keyset_workspace_bytes
    assert [_slots(m) for m in (0, 1, 32, 33, 5000, 1 << 27)] == [64, 64, 64, 128, 16384, 1 << 28]
    for m in (0, 1, 32, 33, 5000, 1 << 27):
        assert ws(m) == _total(m), m
    for m in (-1, (1 << 27) + 1, 1 << 40):
        assert ws(m) == 0 and b"bad list length" in L.convdr_last_error() and b"convdr_keyset_build" in L.convdr_last_error(), m


def _refused(L, name, rc, msg):
    err = L.convdr_last_error()
    assert rc < 0 and msg in err and name in err, (name, rc, msg, err)


def test_every_refusal_of_the_build_entry_is_a_negative_code_with_a_message():
    L = _lib.lib()
    name = b"convdr_keyset_build"
    build = L.convdr_keyset_build
    _refused(L, name, build(P, -1, P, BIG, P, None), b"bad list length")
    _refused(L, name, build(P, (1 << 27) + 1, P, BIG, P, None), b"bad list length")
    _refused(L, name, build(None, 5, P, BIG, P, None), b"NULL argument")
    _refused(L, name, build(P, 5, None, BIG, P, None), b"NULL argument")
    _refused(L, name, build(P, 5, P, BIG, None, None), b"NULL argument")
    _refused(L, name, build(None, 0, None, BIG, P, None), b"NULL argument")        # (m == 0: keys may be NULL, the rest not)
    for m in (0, 1, 33, 5000, 1 << 27):
        _refused(L, name, build(P, m, P, _total(m) - 1, P, None), b"workspace too small")


def test_every_refusal_of_the_member_entry_is_a_negative_code_with_a_message():
    L = _lib.lib()
    name = b"convdr_keys_member"

    def member(row_keys=P, n=N, ws=P, ws_bytes=BIG, bits=P, words=WORDS, counts=P):
        return L.convdr_keys_member(row_keys, n, ws, ws_bytes, 0, bits, words, counts, None)
    _refused(L, name, member(n=-1), b"bad block size")
    _refused(L, name, member(n=1 << 31), b"bad block size")
    for kw in ({"row_keys": None}, {"ws": None}, {"bits": None}, {"counts": None}, {"n": 0, "counts": None}, {"n": 0, "ws": None}):
        _refused(L, name, member(**kw), b"NULL argument")
    _refused(L, name, member(bits=P + 4), b"16-byte aligned")
    _refused(L, name, member(bits=P + 8), b"16-byte aligned")
    _refused(L, name, member(words=WORDS - 1), b"the bitmap holds")
    _refused(L, name, member(n=257, words=8), b"the bitmap holds")
    for kw in ({}, {"n": 0, "row_keys": None, "bits": None, "words": 0}, {"n": 256, "words": 8}, {"n": (1 << 31) - 1, "words": 1 << 26}):
        _refused(L, name, member(ws_bytes=_total(0) - 1, **kw), b"workspace too small")


def test_every_refusal_of_the_locate_entry_is_a_negative_code_with_a_message():
    L = _lib.lib()
    name = b"convdr_keys_locate"

    def locate(row_keys=P, n=N, ws=P, ws_bytes=BIG, keys=P, m=1000, first=P, count=P, dup=P):
        return L.convdr_keys_locate(row_keys, n, ws, ws_bytes, keys, m, first, count, dup, None)
    _refused(L, name, locate(m=-1), b"bad list length")
    _refused(L, name, locate(m=(1 << 27) + 1), b"bad list length")
    _refused(L, name, locate(n=-1), b"bad block size")
    _refused(L, name, locate(n=1 << 31), b"bad block size")
    for kw in ({"row_keys": None}, {"ws": None}, {"keys": None}, {"first": None}, {"count": None}, {"m": 0, "n": 0, "ws": None}):
        _refused(L, name, locate(**kw), b"NULL argument")
    for m in (0, 1, 33, 5000):
        _refused(L, name, locate(m=m, ws_bytes=_total(m) - 1), b"workspace too small")
    _refused(L, name, locate(m=1000, dup=None, ws_bytes=_total(1000) - 1), b"workspace too small")       # (dup_of is nullable)


def test_every_refusal_of_the_compact_ids_entry_is_a_negative_code_with_a_message():
    L = _lib.lib()
    name = b"convdr_ip_compact_ids"
    plan_bytes = L.convdr_ip_compact_workspace_bytes(N, 16, 256) - 256 * 16        # the plan's regions: all but the bounce buffer

    def ids(src=P, dst=2 * P, n=N, bits=P, words=WORDS, ws=P, ws_bytes=BIG):
        return L.convdr_ip_compact_ids(src, dst, n, bits, words, ws, ws_bytes, None)
    _refused(L, name, ids(n=-1), b"bad block size")
    _refused(L, name, ids(n=1 << 31), b"bad block size")
    _refused(L, name, ids(bits=P + 4), b"16-byte aligned")
    _refused(L, name, ids(words=WORDS - 8), b"the bitmap holds")
    _refused(L, name, ids(bits=None, words=8), b"keep_bits is NULL")
    _refused(L, name, ids(ws_bytes=plan_bytes - 1), b"workspace too small")
    for kw in ({"src": None}, {"dst": None}, {"ws": None}):
        _refused(L, name, ids(ws_bytes=plan_bytes, **kw), b"NULL argument")
    _refused(L, name, ids(dst=P), b"out of place")
    assert ids(n=0, src=None, dst=None, bits=None, words=0, ws=None) == 0            # an empty column: nothing to move


# ---- the Python argument checks against a scripted index ---------------------------------------------------------------
class KeyedStub(S.FlatIPIndex):
    """FlatIPIndex with what add(ids=) and the id methods read before any device work, on the CPU: _add_rows appends to a
    host block (refuse=True: it raises, as a half store's add does for a row it cannot hold)."""

    def __init__(self, d=8):
        self.device = torch.device("cpu")
        self._store, self.d_in, self.d = S.STORES["fp32"], d, d
        self._n, self.stats = 0, {}
        self._s32 = self._s16 = self._slo = self._sid = self._sid_spare = None
        self.refuse = False

    def _add_rows(self, x, chunk_bytes=None):
        if self.refuse:
            raise _lib.ConvdrError("the index is unchanged")
        x = torch.as_tensor(x)
        self._s16 = x.clone() if self._s16 is None else torch.cat([self._s16[:self._n], x])
        self._n += int(x.shape[0])


def _x(m, d=8):
    return np.zeros((m, d), np.float32)


def test_add_keeps_the_id_column_in_step_and_refuses_mixed_adds():
    idx = KeyedStub()
    assert idx.ids is None
    idx.add(_x(3), ids=np.array([7, -1, 7]))
    idx.add(_x(2), ids=torch.tensor([K.I64_MAX, K.I64_MIN + 1]))
    idx.add(_x(0), ids=np.zeros(0, np.int64))
    assert idx.ntotal == 5 and idx.ids.dtype == torch.int64 and idx.ids.tolist() == [7, -1, 7, K.I64_MAX, K.I64_MIN + 1]
    with pytest.raises(ValueError, match="carries row ids"):
        idx.add(_x(2))
    plain = KeyedStub()
    plain.add(_x(2))
    with pytest.raises(ValueError, match="without ids"):
        plain.add(_x(2), ids=np.array([1, 2]))
    assert plain.ntotal == 2 and plain.ids is None and idx.ntotal == 5 and idx.ids.tolist()[:2] == [7, -1]


def test_add_refuses_ids_of_the_wrong_length_dtype_or_value_and_leaves_the_index_unchanged():
    idx = KeyedStub()
    idx.add(_x(2), ids=np.array([10, 11]))
    for bad in (np.array([1, 2, 3]), np.array([1]), np.zeros(0, np.int64), np.array([1, 2], np.int32), np.array([1.0, 2.0]),
                np.array([[1, 2]]), torch.tensor([1, 2], dtype=torch.int32), np.array([1, K.I64_MIN]), torch.tensor([K.I64_MIN, 4])):
        with pytest.raises(ValueError):
            idx.add(_x(2), ids=bad)
        assert idx.ntotal == 2 and idx.ids.tolist() == [10, 11]
    # an add the index itself refuses: the column is as it was
    idx.refuse = True
    with pytest.raises(_lib.ConvdrError):
        idx.add(_x(2), ids=np.array([12, 13]))
    assert idx.ntotal == 2 and idx.ids.tolist() == [10, 11] and idx._sid.shape[0] == 2


def test_every_id_method_raises_on_an_index_without_ids():
    idx = KeyedStub()
    idx.add(_x(4))
    q, ids = np.zeros((1, 8), np.float32), np.array([1, 2])
    calls = (lambda: idx.search_ids(q, 2), lambda: idx.search_ids_tensors(q, 2), lambda: idx.remove_ids(ids),
             lambda: idx.id_filter(ids), lambda: idx.id_filter(ids, invert=True), lambda: idx.rows_of(ids),
             lambda: idx.reconstruct_ids(ids), lambda: idx.upsert(ids, torch.zeros(2, 8)))
    for call in calls:
        with pytest.raises(ValueError, match="carries no row ids"):
            call()
    assert idx.ntotal == 4
    # with ids: the list itself is checked before any device work
    idx = KeyedStub()
    idx.add(_x(2), ids=np.array([1, 2]))
    for bad in (np.array([1.0]), np.array([1], np.int32), np.array([[1]]), np.array([K.I64_MIN])):
        for call in (idx.remove_ids, idx.id_filter, idx.rows_of, idx.reconstruct_ids, lambda v: idx.upsert(v, torch.zeros(1, 8))):
            with pytest.raises(ValueError):
                call(bad)
    assert idx.ntotal == 2 and idx.ids.tolist() == [1, 2]


def test_reset_drops_the_column_and_reserve_keeps_it():
    idx = KeyedStub()
    idx.add(_x(3), ids=np.array([5, 6, 7]))
    idx._reserve_ids(10)
    assert idx._sid.shape[0] == 10 and idx.ids.tolist() == [5, 6, 7]
    idx._reserve_ids(4)
    assert idx._sid.shape[0] == 10


# ---- the oracle against brute force ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", K.FAMILIES)
def test_the_oracle_agrees_with_brute_force(family):
    for n, m in ((0, 0), (0, 5), (7, 0), (1, 1), (40, 33), (120, 64)):
        col, lst = K.case(family, n, m)
        assert col.dtype == np.int64 and lst.dtype == np.int64 and col.shape == (n,) and lst.shape == (m,)
        assert not (col == K.I64_MIN).any() and not (lst == K.I64_MIN).any()
        assert np.array_equal(K.member(col, lst), K.brute_member(col, lst)), (family, n, m)
        for got, want in zip(K.locate(col, lst), K.brute_locate(col, lst)):
            assert got.dtype == want.dtype and np.array_equal(got, want), (family, n, m)
        assert K.missing(col, lst) == len({k for k in lst.tolist() if k not in set(col.tolist())})


def test_the_families_hold_what_they_are_named_for():
    col, lst = K.case("random", 1000, 1000)
    assert all(k in col or k in lst for k in K.EDGE_KEYS[:4]) and (col < 0).any() and (lst < 0).any()
    col, lst = K.case("triple", 1000, 999)
    assert not (np.unique(lst, return_counts=True)[1] % 3).any() and K.member(col, lst).any()
    col, lst = K.case("chunks", 1000, 100)
    reps = np.unique(col, return_counts=True)[1]
    assert reps.min() >= 1 and reps.max() == 7 and (K.locate(col, lst)[1] > 1).any()
    col, lst = K.case("absent", 1000, 100)
    assert not K.member(col, lst).any() and K.missing(col, lst) == len(np.unique(lst))
    col, lst = K.case("shift20", 1000, 100)
    assert not (col & ((1 << 20) - 1)).any() and not (lst & ((1 << 20) - 1)).any()
    for family in K.FAMILIES:
        if family != "absent":
            col, lst = K.case(family, 1000, 1000)
            hit = K.member(col, lst)
            assert hit.any() and not hit.all() and K.missing(col, lst) > 0, family
