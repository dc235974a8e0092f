"""Per-query exclusions, the parts that need no GPU: pack_exclusions, the numpy oracle against brute force, the ExcludedSearch view of every
exact entry, and every refusal of the new C entries (argument validation happens before anything touches a device)."""
import inspect

import numpy as np
import pytest
import torch

from convdr_amd import _lib
from convdr_amd.index_store import EXCLUDE_MAX, QueryExclusions, pack_exclusions
from tests import exclude_cases as X


# ---- pack_exclusions ---------------------------------------------------------------------------------------------------------
def test_pack_exclusions_pads_ragged_lists_and_keeps_arrays():
    out = pack_exclusions([[5, 1, 5], [], (7,), np.array([2, -1, 9, 3])], 4)
    assert out.dtype == np.int64
    np.testing.assert_array_equal(out, [[5, 1, 5, -1], [-1, -1, -1, -1], [7, -1, -1, -1], [2, -1, 9, 3]])
    a = np.array([[3, -1, 3], [0, 1, 2]], np.int32)
    np.testing.assert_array_equal(pack_exclusions(a, 2), a.astype(np.int64))
    assert pack_exclusions(a, 2).dtype == np.int64
    t = torch.tensor([[4, 4], [-1, 0]], dtype=torch.int32)
    got = pack_exclusions(t, 2)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int64 and got.tolist() == [[4, 4], [-1, 0]]
    assert pack_exclusions([], 0).shape == (0, 0)
    assert pack_exclusions([[], []], 2).shape == (2, 0)
    assert pack_exclusions(np.zeros((3, 0), np.int64), 3).shape == (3, 0)
    np.testing.assert_array_equal(pack_exclusions([torch.tensor([1, 2]), [3]], 2), [[1, 2], [3, -1]])


@pytest.mark.parametrize("rows,nq", [
    (np.zeros((2, 3), np.float32), 2),              # not integers
    (np.zeros((2, 3), bool), 2),
    (torch.zeros(2, 3), 2),
    (torch.zeros(2, 3, dtype=torch.bool), 2),
    (np.zeros((3, 3), np.int64), 2),                # another number of queries
    (np.zeros(6, np.int64), 2),                     # not [nq, e]
    (torch.zeros(2, 3, 1, dtype=torch.int64), 2),
    ([[1], [2], [3]], 2),
    ([[1.5], [2]], 2),
    ([[[1]], [2]], 2),
    (5, 1),
])
def test_pack_exclusions_refuses(rows, nq):
    with pytest.raises(ValueError):
        pack_exclusions(rows, nq)


def test_pack_exclusions_limit():
    assert EXCLUDE_MAX == 16384
    assert pack_exclusions(np.zeros((1, EXCLUDE_MAX), np.int64), 1).shape == (1, EXCLUDE_MAX)
    assert pack_exclusions([list(range(EXCLUDE_MAX))], 1).shape == (1, EXCLUDE_MAX)
    for too_long in (np.zeros((1, EXCLUDE_MAX + 1), np.int64), torch.zeros(1, EXCLUDE_MAX + 1, dtype=torch.int64),
                     [[0] * (EXCLUDE_MAX + 1)]):
        with pytest.raises(ValueError, match="at most 16384"):
            pack_exclusions(too_long, 1)


def test_query_exclusions_select_needs_no_device():
    rows = torch.tensor([[1, 2, -1, -1], [-1, -1, -1, -1], [0, 5, 9, -1]], dtype=torch.int32)
    ex = QueryExclusions(rows, torch.tensor([2, 0, 3], dtype=torch.int32), [2, 0, 3], 100)
    assert (ex.nq, ex.n, ex.e_max) == (3, 100, 3)
    sub = ex.select([1, 0])
    assert (sub.nq, sub.n, sub.e_max) == (2, 100, 2) and sub.rows.tolist() == [[-1] * 4, [1, 2, -1, -1]] and sub.count.tolist() == [0, 2]
    assert ex.select(torch.tensor([2])).e_max == 3 and ex.select(np.zeros(0, np.int64)).e_max == 0


def test_the_view_offers_every_exact_entry_with_the_index_s_own_arguments():
    from convdr_amd import search as S
    for name in ("search", "search_tensors", "search_begin", "search_ids", "search_ids_tensors", "search_docs", "range_search",
                 "range_search_tensors", "range_count", "rank_rows", "rank_rows_tensors"):
        assert inspect.signature(getattr(S.ExcludedSearch, name)) == inspect.signature(getattr(S.FlatIPIndex, name)), name
    for name in ("rank_ids", "rank_ids_tensors", "search_device", "search_deep_device", "search_distinct"):        # out of scope
        assert not hasattr(S.ExcludedSearch, name), name
    index = type("Named", (str,), {})("index")          # a plain string that carries the one attribute excluding() asks
    index._store = S.STORES["fp32"]
    view = S.FlatIPIndex.excluding(index, "lists")
    assert isinstance(view, S.ExcludedSearch) and (view.index, view.exclude) == ("index", "lists")
    assert S._Pending(1, 2, 3, 4, 5, 6).allowed is None and S._PendingExcluded(1, 2, 3).k == 3
    assert callable(S.FlatIPIndex.exclude_rows) and callable(S.FlatIPIndex.exclude_ids) and S.QueryExclusions is QueryExclusions


# ---- the oracle against brute force ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_matches_brute_force_on_tiny_inputs(seed):
    rs = np.random.RandomState(seed)
    n = 23
    s = rs.randint(0, 6, n).astype(np.float64)              # many exact ties
    allowed = None if seed == 0 else rs.rand(n) < 0.7
    excluded = np.array([3, 3, -1, 7, 11, 22, 0][:7 - seed], np.int64)
    got = X.order(s, allowed, excluded)
    assert got.tolist() == X.brute_order(s, allowed, [x for x in excluded if x >= 0])
    D, I = X.topk(s[None, :], 30, allowed, [excluded])
    assert I[0, :len(got)].tolist() == got.tolist() and (I[0, len(got):] == -1).all() and (D[0, len(got):] == X.PAD_SCORE).all()
    for t in range(n):
        assert X.rank(s, t, allowed, excluded) == X.brute_rank(s, t, allowed, [x for x in excluded if x >= 0]), t
        if t in got:
            assert X.rank(s, t, allowed, excluded) == got.tolist().index(t)
    assert X.in_range(s, 2.5, allowed, excluded).tolist() == [r for r in got if s[r] > 2.5]
    col = np.arange(n) // 4
    Dd, Kd, Rd = X.docs(s, col, 3, allowed, excluded)
    first = []
    for r in got:
        if col[r] not in [col[x] for x in first]:
            first.append(r)
    assert Rd[:len(first[:3])].tolist() == first[:3] and Kd[:len(first[:3])].tolist() == [col[r] for r in first[:3]]


def test_recipes_bite():
    rs = np.random.RandomState(5)
    S = rs.randn(9, 300)
    for k in (1, 10, 100):
        for name in X.RECIPES:
            lists = X.recipe(name, S, k)
            assert X.bites(S, k, lists) == (name != "none"), (name, k)
        whole = X.recipe("whole_topk", S, k)
        np.testing.assert_array_equal(X.topk(S, k, None, whole)[1], X.topk(S, 2 * k)[1][:, k:])
    un = X.recipe("uneven", rs.randn(9, 500), 10)             # (e_q = 37 j mod 301: 0 and more than one 256-entry chunk)
    assert [len(e) for e in un[:3]] == [0, 37, 74] and len(un[8]) == 296
    near = X.recipe("nearly_all", S, 10)
    assert len(X.order(S[0], None, near[0])) == 4 and len(near[1]) == 0
    assert X.padded(un).shape == (9, 296) and X.e_max(X.recipe("scattered", S, 10), 300) == 12


# ---- the C entries refuse bad arguments before anything touches a device -------------------------------------------------------
P, A = 1 << 20, (1 << 20) + 4          # a pointer that is never dereferenced on the host (16-byte aligned; and one that is not)


def _refused(rc, msg, name):
    err = _lib.lib().convdr_last_error()
    assert rc < 0 and msg in err and name.encode() in err, (rc, err)


def test_build_rows_refusals():
    L, name = _lib.lib(), "convdr_excl_build_rows"
    call = lambda rows=P, nq=2, e=8, ld=8, n=1000, ex=P, ex_ld=8, cnt=P, st=P: L.convdr_excl_build_rows(rows, nq, e, ld, n, ex, ex_ld,
                                                                                                        cnt, st, None)
    _refused(call(e=16385, ld=16385, ex_ld=16384), b"at most 16384", name)
    _refused(call(ld=7), b"ld >= e", name)
    _refused(call(nq=-1), b"bad sizes", name)
    _refused(call(n=1 << 31), b"bad block size", name)
    _refused(call(n=-1), b"bad block size", name)
    _refused(call(ex=None), b"NULL", name)
    _refused(call(cnt=None), b"NULL", name)
    _refused(call(st=None), b"status is NULL", name)
    _refused(call(ex_ld=6), b"multiple of 4", name)
    _refused(call(ex_ld=0), b"multiple of 4", name)
    _refused(call(ex_ld=16388), b"multiple of 4", name)
    _refused(call(ex_ld=4), b"cannot hold", name)
    _refused(call(rows=None), b"rows is NULL", name)


def test_build_docs_refusals():
    L, name = _lib.lib(), "convdr_excl_build_docs"
    call = lambda csr=P, rows_len=100, start=P, count=P, nq=2, m=8, ld=8, n=1000, ex=P, ex_ld=8, cnt=P, st=P: \
        L.convdr_excl_build_docs(csr, rows_len, start, count, nq, m, ld, n, ex, ex_ld, cnt, st, None)
    _refused(call(m=16385, ld=16385), b"at most 16384", name)
    _refused(call(ld=7), b"ld >= m", name)
    _refused(call(rows_len=-1), b"rows_len", name)
    _refused(call(rows_len=1 << 31), b"rows_len", name)
    _refused(call(n=1 << 31), b"bad block size", name)
    _refused(call(ex=None), b"NULL", name)
    _refused(call(cnt=None), b"NULL", name)
    _refused(call(st=None), b"status is NULL", name)
    _refused(call(ex_ld=10), b"multiple of 4", name)
    _refused(call(start=None), b"NULL", name)
    _refused(call(csr=None), b"csr_rows is NULL", name)


def test_drop_topk_refusals():
    L, name = _lib.lib(), "convdr_excl_drop_topk"
    call = lambda D=P, I=P, nq=2, m=10, ld=10, ex=P, ex_ld=8, cnt=P, k=5, Do=P, Io=P, kept=P: \
        L.convdr_excl_drop_topk(D, I, nq, m, ld, ex, ex_ld, cnt, k, Do, Io, kept, None)
    _refused(call(k=0), b"k=0", name)
    _refused(call(k=-3), b"k=-3", name)
    _refused(call(ld=9), b"ld >= m", name)
    _refused(call(m=0, ld=0), b"bad sizes", name)
    _refused(call(ex_ld=16388), b"at most 16384", name)
    _refused(call(ex=None), b"NULL", name)
    for out in ("Do", "Io", "kept", "D", "I"):
        _refused(call(**{out: None}), b"NULL", name)


def test_ragged_refusals():
    L = _lib.lib()
    name = "convdr_excl_count_ragged"
    call = lambda lims=P, I=P, total=10, nq=2, ex=P, ex_ld=8, cnt=P, kept=P: L.convdr_excl_count_ragged(lims, I, total, nq, ex, ex_ld,
                                                                                                        cnt, kept, None)
    _refused(call(total=-1), b"bad sizes", name)
    _refused(call(kept=None), b"NULL", name)
    _refused(call(lims=None), b"NULL", name)
    _refused(call(I=None), b"NULL", name)
    _refused(call(ex_ld=16388), b"at most 16384", name)
    _refused(call(cnt=None), b"NULL", name)
    name = "convdr_excl_pack_ragged"
    call = lambda lims=P, D=P, I=P, total=10, nq=2, ex=P, ex_ld=8, cnt=P, lo=P, Do=P, Io=P, to=5: \
        L.convdr_excl_pack_ragged(lims, D, I, total, nq, ex, ex_ld, cnt, lo, Do, Io, to, None)
    _refused(call(to=11), b"total_out <= total", name)
    _refused(call(to=-1), b"bad sizes", name)
    _refused(call(ex_ld=3), b"multiple of 4", name)
    for out in ("Do", "Io", "lo", "lims", "D", "I"):
        _refused(call(**{out: None}), b"NULL", name)


def test_count_ahead_refusals():
    L, name = _lib.lib(), "convdr_ip_excl_count_ahead"
    call = lambda store=1, q=P, nq=2, p32=P, p16=P, scale=4.0, n=1000, d=768, bits=None, words=0, ex=P, ex_ld=8, cnt=P, np_=3, pairq=P, \
        x=P, r=P, ahead=P: L.convdr_ip_excl_count_ahead(store, q, nq, p32, p16, scale, n, d, bits, words, ex, ex_ld, cnt, np_, pairq, x, r,
                                                        ahead, None)
    _refused(call(store=3), b"store must be", name)
    _refused(call(n=1 << 31), b"bad block size", name)
    _refused(call(d=70), b"d % 64", name)
    _refused(call(scale=0.75), b"power of two", name)
    _refused(call(store=2, scale=0.5), b"power of two >= 1", name)
    _refused(call(bits=None, words=8), b"row_bits is NULL", name)
    _refused(call(bits=A, words=32), b"16-byte aligned", name)
    _refused(call(bits=P, words=24), b"the bitmap holds", name)
    _refused(call(ex_ld=16388), b"at most 16384", name)
    _refused(call(ex=None), b"NULL", name)
    _refused(call(ahead=None), b"ahead is NULL", name)
    _refused(call(np_=-1), b"bad sizes", name)
    _refused(call(pairq=None), b"NULL", name)
    _refused(call(x=None), b"NULL", name)
    _refused(call(store=0, p32=None), b"NULL block pointer", name)
    _refused(call(store=2, p16=None), b"NULL block pointer", name)
