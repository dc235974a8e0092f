"""Per-query exclusions on the GPU: FlatIPIndex.excluding(ex).search / search_ids / search_docs / range_search / range_count /
rank_rows, the QueryExclusions operand, and the new C entries through ctypes.

Expected value everywhere, no tolerances: tests/exclude_cases.py -- per query the canonical order of the allowed rows with the
query's excluded rows removed, over oracle.search.canonical_scores; D is that score rounded to fp32.  Every comparison is
assert_array_equal."""
import numpy as np
import pytest

from tests import exclude_cases as X
from tests import index_cases as C
from tests.golden.make_golden import synth_corpus
from tests.index_cases import torch_cuda      # noqa: F401 (the fixture, by name)

pytestmark = pytest.mark.gpu

SHAPES = [(300, 3, 64, False), (257, 1, 100, False), (5000, 37, 768, False), (5000, 37, 768, True), (33000, 130, 128, False)]
BIG = (33000, 130, 128, False)          # searched with its first 8 queries
I64_MIN = -(1 << 63)
PAD = 0xffffffff


def _case(shape):
    """(Q, S) of a shape: all queries, or the first 8 of the large one"""
    (P, Q), S = C.corpus(shape), C.scores(shape)
    return (Q[:8], S[:8]) if shape == BIG else (Q, S)


def _equal(got, want, what):
    D, I = (t.cpu().numpy() if hasattr(t, "cpu") else t for t in got)
    np.testing.assert_array_equal(I, want[1], err_msg=str(what))
    np.testing.assert_array_equal(D, want[0], err_msg=str(what))


# ---- search ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,precision", C.CONFIGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_search_with_exclusions_equals_the_oracle(torch_cuda, shape, storage, precision):
    idx = C.index(shape, storage, precision)
    Q, S = _case(shape)
    n = shape[0]
    for k in (1, 10, 100):
        plain = idx.search_tensors(Q, k)
        for name in X.RECIPES + (("nearly_all",) if n == 300 else ()):
            lists = X.recipe(name, S, k)
            bite = name != "none" and not (name == "uneven" and len(Q) == 1)         # (uneven: query 0 excludes nothing)
            assert X.bites(S, k, lists) == bite, (name, k)
            want = X.topk(S, k, None, lists)
            got = idx.excluding(X.padded(lists)).search_tensors(Q, k)
            _equal(got, want, (shape, name, k))
            assert idx.stats["exclude_depth"] == min(k + X.e_max(lists, n), max(k, n)), (name, k, idx.stats)
            assert (idx.stats["excluded_dropped"] > 0) == bite, (name, k, idx.stats)
            if name == "none":
                assert torch_cuda.equal(got[0], plain[0]) and torch_cuda.equal(got[1], plain[1])
            if name == "whole_topk":
                _equal(got, tuple(t[:, k:] for t in X.topk(S, 2 * k)), (shape, name, k))
            if name == "nearly_all":
                assert (k + X.e_max(lists, n) > n) == (k >= 10) and (want[1][0, :min(k, 4)] >= 0).all() and (want[1][0, 4:] == -1).all()
    # a list of lists, numpy in / numpy out, and the handle pair
    lists = X.recipe("scattered", S, 10)
    want = X.topk(S, 10, None, lists)
    _equal(idx.excluding([e.tolist() for e in lists]).search(Q, 10), want, "lists")
    _equal(idx.search_finish(idx.excluding(torch_cuda.as_tensor(X.padded(lists)).to(idx.device)).search_begin(Q, 10)), want, "handle")


@pytest.mark.parametrize("storage,precision", C.CONFIGS)
@pytest.mark.parametrize("mask", ["half", "word_edges"])
@pytest.mark.parametrize("shape", [(300, 3, 64, False), (5000, 37, 768, True)])
def test_search_with_exclusions_and_a_row_filter(torch_cuda, shape, mask, storage, precision):
    idx = C.index(shape, storage, precision)
    Q, S = _case(shape)
    n = shape[0]
    allowed = C.mask(n, mask)
    f = idx.row_filter(allowed)
    banned = np.flatnonzero(~allowed)[:2]                   # excluded rows that are not allowed: they change nothing
    for k in (1, 10, 100):
        for name in ("top1", "scattered", "uneven"):
            lists = [np.concatenate([e, banned]) for e in X.recipe(name, S, k, allowed)]
            assert X.bites(S, k, lists, allowed)
            want = X.topk(S, k, allowed, lists)
            _equal(idx.excluding(X.padded(lists)).search_tensors(Q, k, allowed=f), want, (shape, mask, name, k))
            assert idx.stats["exclude_depth"] == min(k + X.e_max(lists, n), max(k, int(allowed.sum())))
    only_banned = [banned] * len(Q)
    _equal(idx.excluding(X.padded(only_banned)).search_tensors(Q, 10, allowed=f), X.topk(S, 10, allowed), "banned only")


@pytest.mark.parametrize("storage,precision", [("fp32", "auto"), ("fp16", "auto")])
def test_the_depth_crosses_into_the_deep_pipeline(torch_cuda, storage, precision):
    idx = C.index(BIG, storage, precision)
    Q, S = _case(BIG)
    k = 4000
    lists = X.recipe("uneven", S, k)
    assert X.e_max(lists, BIG[0]) == 259 and X.bites(S, k, lists)
    _equal(idx.excluding(X.padded(lists)).search_tensors(Q, k), X.topk(S, k, None, lists), "deep")
    assert idx.stats["exclude_depth"] == 4259 > idx.MAX_K and idx.stats["large_k"] == 4259 and idx.stats["deep"] + idx.stats["chunked_queries"] == 8


@pytest.mark.parametrize("storage,precision", C.CONFIGS)
def test_search_ids_with_exclusions(torch_cuda, storage, precision):
    from convdr_amd.search import FlatIPIndex
    shape = (300, 3, 64, False)
    (P, Q), S = C.corpus(shape), C.scores(shape)
    col = (np.arange(300, dtype=np.int64) * 11 + 5)
    idx = FlatIPIndex(64, storage=storage, precision=precision, prepin=False)
    idx.add(P.astype(np.float16) if storage == "fp16" else P, ids=col)
    for k in (1, 10, 100):
        for name in X.RECIPES + ("nearly_all",):
            lists = X.recipe(name, S, k)
            D, I = X.topk(S, k, None, lists)
            _equal(idx.excluding(X.padded(lists)).search_ids_tensors(Q, k), (D, np.where(I >= 0, col[np.maximum(I, 0)], -1)), (name, k))
    _equal(idx.excluding(X.padded(lists)).search_ids(Q, 10), (D[:, :10], np.where(I >= 0, col[np.maximum(I, 0)], -1)[:, :10]), "numpy")


# ---- ties, rank ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,precision", C.CONFIGS)
def test_ties_keep_the_row_order_and_the_rank_follows(torch_cuda, storage, precision):
    from convdr_amd.search import FlatIPIndex
    from oracle import search as OS
    P = synth_corpus(3, 200, 64).astype(np.float16).astype(np.float32)
    P[20] = P[30] = P[10]
    Q = (P[[10, 77]] + 0.05 * synth_corpus(4, 2, 64)).astype(np.float32)
    S = OS.canonical_scores(Q, P)
    assert S[0, 10] == S[0, 20] == S[0, 30] and X.order(S[0])[:3].tolist() == [10, 20, 30]
    idx = FlatIPIndex(64, storage=storage, precision=precision, prepin=False)
    idx.add(P.astype(np.float16) if storage == "fp16" else P)
    for lists in ([[10], []], [[20], [10]], [[10, 20], [30]], [[30], [10, 20, 30]]):
        _equal(idx.excluding(lists).search_tensors(Q, 5), X.topk(S, 5, None, lists), lists)
    assert idx.excluding([[10], []]).search(Q, 5)[1][0, :2].tolist() == [20, 30]
    tgt = np.array([30, 30])
    base = idx.rank_rows(Q, tgt)
    assert base[0] == 2 and base[1] == X.rank(S[1], 30)
    for lists, drop in (([[10], [10]], 1), ([[10, 20], [20, 10, 10]], 2), ([[30], [30]], 0), ([[30, 20], [-1, 30, 10]], 1)):
        got = idx.excluding(lists).rank_rows(Q, tgt)
        assert got.tolist() == [X.rank(S[j], 30, None, lists[j]) for j in range(2)], lists
        assert got[0] == base[0] - drop and got[1] == base[1] - drop, lists


@pytest.mark.parametrize("storage,precision", C.CONFIGS)
@pytest.mark.parametrize("mask", [None, "half"])
@pytest.mark.parametrize("shape", [(300, 3, 64, False), (5000, 37, 768, True), BIG])
def test_rank_rows_with_exclusions(torch_cuda, shape, mask, storage, precision):
    idx = C.index(shape, storage, precision)
    Q, S = _case(shape)
    n, k = shape[0], 10
    allowed = None if mask is None else C.mask(n, mask)
    f = None if mask is None else idx.row_filter(allowed)
    for name in ("scattered", "uneven"):
        lists = X.recipe(name, S, k, allowed)
        ex = idx.exclude_rows(X.padded(lists))
        # targets inside the top-k: the rank is the position in the search with the same exclusions
        _, I = idx.excluding(ex).search(Q, k, allowed=f)
        assert (I >= 0).all()
        np.testing.assert_array_equal(idx.excluding(ex).rank_rows(Q, I, allowed=f), np.tile(np.arange(k), (len(Q), 1)))
        # targets at depth n / 2 of the full order, an excluded row, a row that is not allowed, padding
        full = [X.order(S[j]) for j in range(len(Q))]
        tgt = np.array([[o[n // 2], o[n // 2 + 1], X.clean(lists[j], n)[0] if len(X.clean(lists[j], n)) else o[0], o[3], -1]
                        for j, o in enumerate(full)], np.int64)
        want = np.array([[X.rank(S[j], t, allowed, lists[j]) if t >= 0 else -1 for t in tgt[j]] for j in range(len(Q))])
        plain = np.array([[X.rank(S[j], t, allowed) if t >= 0 else -1 for t in tgt[j]] for j in range(len(Q))])
        assert (want != plain).any()                        # the exclusion bites
        np.testing.assert_array_equal(idx.excluding(ex).rank_rows(Q, tgt, allowed=f), want, err_msg=str((shape, mask, name)))
        np.testing.assert_array_equal(idx.rank_rows(Q, tgt, allowed=f), plain)


# ---- range ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,precision", C.CONFIGS)
@pytest.mark.parametrize("mask", [None, "half"])
@pytest.mark.parametrize("shape", [(300, 3, 64, False), (5000, 37, 768, False), BIG])
def test_range_search_and_count_with_exclusions(torch_cuda, shape, mask, storage, precision):
    idx = C.index(shape, storage, precision)
    Q, S = _case(shape)
    n, k = shape[0], 10
    allowed = None if mask is None else C.mask(n, mask)
    f = None if mask is None else idx.row_filter(allowed)
    lists = X.recipe("scattered", S, k, allowed)
    ex = idx.exclude_rows(X.padded(lists))
    orders = [X.order(S[j], allowed) for j in range(len(Q))]
    for lo, hi in ((3, 4), (2 * k + 3, 2 * k + 4)):         # between ranks 3 and 4; below rank 2k
        rad = np.array([np.float32((S[j, o[lo]] + S[j, o[hi]]) / 2) for j, o in enumerate(orders)], np.float32)
        want = [X.in_range(S[j], rad[j], allowed, lists[j]) for j in range(len(Q))]
        plain = [X.in_range(S[j], rad[j], allowed) for j in range(len(Q))]
        assert all(len(w) < len(p) for w, p in zip(want, plain))              # the exclusion bites
        lims, D, I = idx.excluding(ex).range_search(Q, rad, allowed=f)
        np.testing.assert_array_equal(lims, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
        np.testing.assert_array_equal(I, np.concatenate(want))
        np.testing.assert_array_equal(D, np.concatenate([S[j, w].astype(np.float32) for j, w in enumerate(want)]))
        assert idx.stats["excluded_dropped"] == sum(len(p) - len(w) for w, p in zip(want, plain))
        np.testing.assert_array_equal(idx.excluding(ex).range_count(Q, rad, allowed=f), [len(w) for w in want])
        np.testing.assert_array_equal(idx.range_count(Q, rad, allowed=f), [len(p) for p in plain])
    # a radius above every score: nothing to drop from
    lims, D, I = idx.excluding(ex).range_search(Q, 1e30, allowed=f)
    assert lims.tolist() == [0] * (len(Q) + 1) and len(D) == len(I) == 0
    assert idx.excluding(ex).range_count(Q, 1e30, allowed=f).tolist() == [0] * len(Q)


# ---- documents ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,precision", C.CONFIGS)
def test_search_docs_with_exclusions(torch_cuda, storage, precision):
    from convdr_amd.search import FlatIPIndex
    shape = (5000, 37, 768, False)
    (P, Q), S = C.corpus(shape), C.scores(shape)
    n, nq = 5000, 37
    col = (np.arange(n, dtype=np.int64) // 4) * 7 + 1000         # four chunk rows per document
    idx = FlatIPIndex(768, storage=storage, precision=precision, prepin=False)
    idx.add(P.astype(np.float16) if storage == "fp16" else P, ids=col)

    def check(got, lists, allowed, k, what):
        D, K, R, _ = (t.cpu().numpy() for t in got)
        for j in range(nq):
            wd, wk, wr = X.docs(S[j], col, k, allowed, lists[j])
            np.testing.assert_array_equal(R[j], wr, err_msg=str((what, j)))
            np.testing.assert_array_equal(K[j], wk, err_msg=str((what, j)))
            np.testing.assert_array_equal(D[j], wd, err_msg=str((what, j)))
    for k in (1, 10):
        plain = [X.docs(S[j], col, k + 2) for j in range(nq)]
        # whole documents: each query's two best, an id on no row, padding
        ids = np.array([[p[1][1], 5, I64_MIN, p[1][0]] for p in plain], np.int64)
        ex = idx.exclude_ids(ids)
        lists = [np.flatnonzero(np.isin(col, ids[j])) for j in range(nq)]
        assert ex.e_max == 8 and ex.nq == nq and ex.count.tolist() == [8] * nq
        np.testing.assert_array_equal(ex.rows.cpu().numpy().view(np.uint32)[:, :8], np.array(lists))
        got = idx.excluding(ex).search_docs(Q, k)
        check(got, lists, None, k, "ids")
        K = got[1].cpu().numpy()
        assert not any(np.isin(K[j], ids[j]).any() for j in range(nq))
        # the best chunk of each query's best document only: its next chunk stands for it
        best = [np.array([p[2][0]]) for p in plain]
        got = idx.excluding(X.padded(best)).search_docs(Q, k)
        check(got, best, None, k, "best chunk")
        assert all(got[2][j, 0].item() != best[j][0] for j in range(nq))
        # with a row filter, and a small first depth so that the distinct walk deepens for the open queries
        allowed = C.mask(n, "half")
        check(idx.excluding(ex).search_docs(Q, k, allowed=idx.row_filter(allowed), depth=k), lists, allowed, k, "filter")
        assert len(idx.distinct_stats["depths"]) > 1 or k == 1
    with pytest.raises(ValueError):
        C.index((300, 3, 64, False), storage, precision).exclude_ids(np.zeros((3, 2), np.int64))          # no id column


# ---- the operand ------------------------------------------------------------------------------------------------------------------
def test_select_reuse_and_staleness(torch_cuda):
    from convdr_amd.search import FlatIPIndex, QueryExclusions
    shape = (300, 3, 64, False)
    (P, Q), S = C.corpus(shape), C.scores(shape)
    idx = FlatIPIndex(64, prepin=False)
    idx.add(P)
    lists = X.recipe("scattered", S, 10)
    ex = idx.exclude_rows(X.padded(lists))
    assert isinstance(ex, QueryExclusions) and (ex.nq, ex.n, ex.e_max) == (3, 300, 12)
    assert ex.rows.shape == (3, 12) and ex.rows.shape[1] % 4 == 0 and ex.count.tolist() == [12, 12, 12]
    rows = ex.rows.cpu().numpy().view(np.uint32)
    for j in range(3):
        np.testing.assert_array_equal(rows[j], X.clean(lists[j], 300))
    want = X.topk(S, 10, None, lists)
    _equal(idx.excluding(ex).search_tensors(Q, 10), want, "first")
    _equal(idx.excluding(ex).search_tensors(Q, 10), want, "again")
    np.testing.assert_array_equal(idx.excluding(ex).rank_rows(Q, want[1]), np.tile(np.arange(10), (3, 1)))
    sub = ex.select([2, 0])
    _equal(idx.excluding(sub).search_tensors(Q[[2, 0]], 10), (want[0][[2, 0]], want[1][[2, 0]]), "select")
    ragged = idx.exclude_rows([[5, 5, 1], [], [299]])
    assert ragged.count.tolist() == [2, 0, 1] and ragged.rows.shape == (3, 4)
    assert ragged.rows.cpu().numpy().view(np.uint32).tolist() == [[1, 5, PAD, PAD], [PAD] * 4, [299, PAD, PAD, PAD]]
    empty = idx.exclude_rows(np.zeros((3, 0), np.int64))
    assert empty.e_max == 0 and torch_cuda.equal(idx.excluding(empty).search_tensors(Q, 10)[1], idx.search_tensors(Q, 10)[1])
    # refusals: a row >= ntotal on the host and on the device, too many entries, another number of queries
    with pytest.raises(ValueError, match="ntotal"):
        idx.exclude_rows([[300], [], []])
    with pytest.raises(ValueError, match="ntotal"):
        idx.exclude_rows(torch_cuda.tensor([[1, 300], [2, 3], [4, 5]], device=idx.device))
    with pytest.raises(ValueError, match="at most"):
        idx.exclude_rows(np.zeros((1, 16385), np.int64))
    with pytest.raises(ValueError):
        idx.excluding(ex).search_tensors(Q[:2], 10)
    # stale after add: the same rule as a RowFilter
    idx.add(P[:5])
    for call in (lambda: idx.excluding(ex).search_tensors(Q, 10), lambda: idx.excluding(ex).rank_rows(Q, want[1]),
                 lambda: idx.excluding(ex).range_count(Q, 0.0), lambda: idx.excluding(ex).search_begin(Q, 10)):
        with pytest.raises(ValueError, match="stale"):
            call()
    _equal(idx.excluding(idx.exclude_rows(X.padded(lists))).search_tensors(Q, 10),
           X.topk(np.concatenate([S, S[:, :5]], 1), 10, None, lists), "rebuilt")


# ---- the C entries through ctypes ---------------------------------------------------------------------------------------------------
def _operand(torch, sets, dev):
    """device (rows int32 [nq, ld], count int32 [nq]) of sorted distinct row sets"""
    ld = max(4, (max(len(s) for s in sets) + 3) // 4 * 4)
    rows = np.full((len(sets), ld), PAD, np.uint32)
    for j, s in enumerate(sets):
        rows[j, :len(s)] = np.sort(np.asarray(s, np.uint32))
    return (torch.as_tensor(rows.view(np.int32)).to(dev), torch.as_tensor(np.array([len(s) for s in sets], np.int32)).to(dev), ld)


def _synthetic(m, seed):
    """a canonical list of m entries (the last min(3, m - 1) are padding) and three member sets: all, none, every third"""
    rs = np.random.RandomState(seed)
    valid = m - min(3, m - 1)
    I = np.full(m, -1, np.int64)
    I[:valid] = rs.permutation(200000)[:valid]
    D = np.full(m, X.PAD_SCORE, np.float32)
    D[:valid] = np.sort(rs.randn(valid).astype(np.float32))[::-1]
    return D, I, [I[:valid][:16384], np.array([200001, 7000000], np.int64), I[:valid][::3][:16384]]


@pytest.mark.parametrize("m", [1, 255, 256, 257, 5000, 70000])
def test_drop_topk_entry(torch_cuda, m):
    from convdr_amd import _lib
    torch, L, ptr = torch_cuda, _lib.lib(), _lib.ptr
    dev = torch.device("cuda:0")
    D, I, sets = _synthetic(m, m)
    ld = m + 5
    Dm = np.full((3, ld), 7.0, np.float32)
    Im = np.full((3, ld), 123, np.int64)                     # (beyond m: never read)
    Dm[:, :m], Im[:, :m] = D, I
    ex_rows, ex_count, ex_ld = _operand(torch, sets, dev)
    Dt, It = torch.as_tensor(Dm).to(dev), torch.as_tensor(Im).to(dev)
    for k in (1, m, m + 3):
        Do = torch.full((3, k), 5.0, dtype=torch.float32, device=dev)
        Io = torch.full((3, k), 5, dtype=torch.int64, device=dev)
        kept = torch.full((3,), -7, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.convdr_excl_drop_topk(ptr(Dt), ptr(It), 3, m, ld, ptr(ex_rows), ex_ld, ptr(ex_count), k, ptr(Do), ptr(Io),
                                               ptr(kept), _lib.stream_ptr()), "convdr_excl_drop_topk")
        Do, Io, kept = Do.cpu().numpy(), Io.cpu().numpy(), kept.cpu().numpy()
        for j, s in enumerate(sets):
            keep = (I >= 0) & ~np.isin(I, s)
            wD, wI = np.full(k, X.PAD_SCORE, np.float32), np.full(k, -1, np.int64)
            c = min(k, int(keep.sum()))
            wD[:c], wI[:c] = D[keep][:c], I[keep][:c]
            assert kept[j] == keep.sum(), (m, k, j)
            np.testing.assert_array_equal(Io[j], wI, err_msg=str((m, k, j)))
            np.testing.assert_array_equal(Do[j], wD, err_msg=str((m, k, j)))


def test_ragged_entries(torch_cuda):
    from convdr_amd import _lib
    torch, L, ptr = torch_cuda, _lib.lib(), _lib.ptr
    dev = torch.device("cuda:0")
    ms = [0, 1, 255, 256, 257, 5000, 70000, 300, 300]
    parts = [_synthetic(m, 50 + j) if m else (np.zeros(0, np.float32), np.zeros(0, np.int64), [np.zeros(0, np.int64)] * 3)
             for j, m in enumerate(ms)]
    # every third everywhere, but all for the query before last and none for the last one; the lists' own tail padding is cut off
    sets = [p[2][2] for p in parts[:-2]] + [parts[-2][2][0], parts[-1][2][1]]
    Ds = [p[0][p[1] >= 0] for p in parts]
    Is = [p[1][p[1] >= 0] for p in parts]
    lims = np.concatenate([[0], np.cumsum([len(i) for i in Is])]).astype(np.int64)
    D, I, total, nq = np.concatenate(Ds), np.concatenate(Is), int(lims[-1]), len(ms)
    ex_rows, ex_count, ex_ld = _operand(torch, [s if len(s) else np.zeros(0, np.int64) for s in sets], dev)
    Dt, It, lt = torch.as_tensor(D).to(dev), torch.as_tensor(I).to(dev), torch.as_tensor(lims).to(dev)
    out = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.convdr_excl_count_ragged(ptr(lt), ptr(It), total, nq, ptr(ex_rows), ex_ld, ptr(ex_count), ptr(out[1:]),
                                              _lib.stream_ptr()), "convdr_excl_count_ragged")
    keeps = [~np.isin(i, s) for i, s in zip(Is, sets)]
    np.testing.assert_array_equal(out[1:].cpu().numpy(), [int(kp.sum()) for kp in keeps])
    assert keeps[-2].sum() == 0 and keeps[-1].all()
    lo = torch.cumsum(out, 0)
    total_out = int(lo[-1].item())
    Do = torch.full((total_out + 8,), 5.0, dtype=torch.float32, device=dev)
    Io = torch.full((total_out + 8,), 5, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.convdr_excl_pack_ragged(ptr(lt), ptr(Dt), ptr(It), total, nq, ptr(ex_rows), ex_ld, ptr(ex_count), ptr(lo), ptr(Do),
                                             ptr(Io), total_out, _lib.stream_ptr()), "convdr_excl_pack_ragged")
    np.testing.assert_array_equal(Io.cpu().numpy(), np.concatenate([i[kp] for i, kp in zip(Is, keeps)] + [np.full(8, 5)]))
    np.testing.assert_array_equal(Do.cpu().numpy(), np.concatenate([d[kp] for d, kp in zip(Ds, keeps)] + [np.full(8, 5.0, np.float32)]))


def _build_rows(torch, rows, n, ld=None):
    from convdr_amd import _lib
    L, ptr = _lib.lib(), _lib.ptr
    dev = torch.device("cuda:0")
    nq, e = rows.shape
    ld = ld or max(4, (e + 3) // 4 * 4)
    t = torch.as_tensor(rows).to(dev)
    ex = torch.full((nq, ld), 77, dtype=torch.int32, device=dev)
    cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    st = torch.full((1,), 99, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.convdr_excl_build_rows(ptr(t), nq, e, e, n, ptr(ex), ld, ptr(cnt), ptr(st), _lib.stream_ptr()), "convdr_excl_build_rows")
    return ex.cpu().numpy().view(np.uint32), cnt.cpu().numpy(), int(st.item())


def _check_built(ex, cnt, want):
    for j, w in enumerate(want):
        assert cnt[j] == len(w), j
        np.testing.assert_array_equal(ex[j, :len(w)], w, err_msg=str(j))
        assert (ex[j, len(w):] == PAD).all(), j


def test_build_rows_entry(torch_cuda):
    rs = np.random.RandomState(3)
    n = 1 << 20
    for e in (1, 5, 64, 65, 1000, 1025, 16384):
        rows = rs.randint(0, max(2, e // 2), size=(4, e)).astype(np.int64)      # many repeats
        rows[0, ::3] = -1                                                       # padding in between
        rows[1, :] = -5                                                         # nothing
        rows[2, :] = 1234                                                       # one row, e times
        if e == 16384:
            rows[3] = rs.permutation(n)[:e]                                     # 16,384 distinct entries exactly
        ex, cnt, st = _build_rows(torch_cuda, rows, n)
        assert st == 0 and ex.shape[1] % 4 == 0
        _check_built(ex, cnt, [X.clean(r, n) for r in rows])
    # the largest row id, and a row >= n: bit 0, the row left out, the others intact
    rows = np.array([[n - 1, 0, n, 7], [3, 2, 1, 0]], np.int64)
    ex, cnt, st = _build_rows(torch_cuda, rows, n)
    assert st == 1
    _check_built(ex, cnt, [np.array([0, 7, n - 1]), np.array([0, 1, 2, 3])])
    ex, cnt, st = _build_rows(torch_cuda, np.array([[1 << 40, 5]], np.int64), n, ld=8)
    assert st == 1
    _check_built(ex, cnt, [np.array([5])])


def test_build_docs_entry(torch_cuda):
    from convdr_amd import _lib
    torch, L, ptr = torch_cuda, _lib.lib(), _lib.ptr
    dev = torch.device("cuda:0")
    n = 100000
    csr = np.arange(20000, dtype=np.int64) * 3 % n               # rows of the segments (any values below n)
    csr[19990] = n + 5                                           # a row >= n
    # query 0: two segments and a repeat of the first; query 1: 16,384 entries exactly; query 2: one more than that;
    # query 3: an empty segment, one outside the list, the one that holds the bad row
    start = np.array([[0, 100, 0], [1000, 9192, 0], [1000, 9192, 17384], [50, 19999, 19985]], np.int64)
    count = np.array([[4, 3, 4], [8192, 8192, 0], [8192, 8192, 1], [0, 5, 10]], np.int32)
    ex = torch.full((4, 16384), 77, dtype=torch.int32, device=dev)
    cnt = torch.full((4,), -7, dtype=torch.int32, device=dev)
    st = torch.full((1,), 99, dtype=torch.int32, device=dev)
    csr_t, start_t, count_t = (torch.as_tensor(a).to(dev) for a in (csr, start, count))       # (alive across the call)
    with torch.cuda.device(dev):
        _lib.check(L.convdr_excl_build_docs(ptr(csr_t), len(csr), ptr(start_t), ptr(count_t), 4, 3, 3, n, ptr(ex), 16384, ptr(cnt),
                                            ptr(st), _lib.stream_ptr()), "convdr_excl_build_docs")
    ex, cnt, st = ex.cpu().numpy().view(np.uint32), cnt.cpu().numpy(), int(st.item())
    assert st == 3                                               # bit 0: the row >= n; bit 1: query 2's 16,385 entries
    seg = lambda s, c: csr[s:s + c]
    want = [X.clean(np.concatenate([seg(0, 4), seg(100, 3)]), n), X.clean(seg(1000, 16384), n), None,
            X.clean(np.delete(seg(19985, 10), 5), n)]
    assert len(want[1]) == 16384
    for j in (0, 1, 3):
        assert cnt[j] == len(want[j]), j
        np.testing.assert_array_equal(ex[j, :cnt[j]], want[j])
        assert (ex[j, cnt[j]:] == PAD).all()


def test_count_ahead_entry(torch_cuda):
    """the entry against score_rows: thresholds at a listed row's own score, with and without a bitmap"""
    shape = (300, 3, 64, False)
    (P, Q), S = C.corpus(shape), C.scores(shape)
    for storage, precision in C.CONFIGS:
        idx = C.index(shape, storage, precision)
        lists = X.recipe("uneven", S, 10)                    # 0, 37 and 74 rows
        ex = idx.exclude_rows(X.padded(lists))
        allowed = C.mask(300, "half")
        torch = torch_cuda
        qt = idx._queries(Q)
        pairq = torch.tensor([2, 1, 0, 2, 1, 7], device=idx.device)
        rows = np.array([lists[2][5], lists[1][0], 4, 17, lists[1][-1], 0], np.int64)
        xs = torch.as_tensor(np.array([S[q, r] if q < 3 else 0.0 for q, r in zip(pairq.tolist(), rows)])).to(idx.device)
        for f, m in ((None, None), (idx.row_filter(allowed), allowed)):
            for row_thr in (rows, np.full(6, -1, np.int64)):
                got = idx._excluded_ahead(ex, f, qt, pairq, xs, torch.as_tensor(row_thr).to(idx.device)).cpu().numpy()
                want = [sum(1 for x in X.clean(lists[q], 300) if (m is None or m[x]) and
                            (S[q, x] > S[q, r] or (S[q, x] == S[q, r] and x < t))) if q < 3 else 0
                        for q, r, t in zip(pairq.tolist(), rows, row_thr)]
                np.testing.assert_array_equal(got, want)
