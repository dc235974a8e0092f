"""Document-level rank: FlatIPIndex.doc_ordinals / rank_ids / convdr_doc_ordinals / convdr_ip_rank_docs.

Expected values everywhere, no tolerances: the oracle of tests/doc_rank_cases.py over S = oracle.search.canonical_scores(Q, P)
(the corpora, stores and the resident index of tests/index_cases.py; the id column is doc_cases.chunked_ids(n): documents of
1 .. 6 rows scattered over the block, so documents straddle every 256-row tile edge and ndocs is no multiple of 32).  Every
rank call runs twice, over a workspace poisoned with two different byte patterns, and must return the same ranks: the bitmap
is zeroed inside the call or this fails."""
import numpy as np
import pytest

from oracle import search as OS
from tests import doc_cases as DC
from tests import doc_rank_cases as RC
from tests import key_cases as K
from tests.golden.make_golden import synth_corpus
from tests.helpers import fill_bytes
from tests.index_cases import CONFIGS, MASKS, SHAPES, torch_cuda      # noqa: F401 (torch_cuda: the fixture, by name)
from tests.index_cases import corpus as _corpus, index as _index, mask as _mask, scores as _scores
from tests.test_rank_rows_gpu import _documented_eps, _order

pytestmark = pytest.mark.gpu

PAD = np.float32(-3.4028234663852886e38)
DEPTHS = lambda n: [0, 1, 9, n // 4, n // 2, n - 1]

_COL, _TARGETS = {}, {}


def _column(n):
    if n not in _COL:
        col = DC.chunked_ids(n)
        col.setflags(write=False)
        _COL[n] = col
    return _COL[n]


def _doc_index(torch, shape, storage, precision, col):
    """the resident index of index_cases with `col` for its id column"""
    idx = _index(shape, storage, precision)
    idx._sid, idx._sid_spare = torch.from_numpy(np.array(col)).cuda(), None
    return idx


def _best_positions(order_j, inv, ndocs):
    """is_best[p]: the row at position p of the canonical order is its document's best row"""
    first = np.full(ndocs, len(order_j))
    np.minimum.at(first, inv[order_j], np.arange(len(order_j)))
    is_best = np.zeros(len(order_j), bool)
    is_best[first] = True
    return is_best


def _targets(shape, depths=None):
    """(rows int64 [nq, 6], their row ranks, ids, the oracle's document ranks): per query and depth the first row rank at or
    after the depth whose row is its document's best row for that query -- before it when there is none after (n - 1: the last
    row of the order is the best row of a one-row document only)"""
    key = (shape, None if depths is None else tuple(depths))
    if key not in _TARGETS:
        n, nq = shape[0], shape[1]
        col, S, order = _column(n), _scores(shape), _order(shape)
        _, inv = np.unique(col, return_inverse=True)
        inv = inv.reshape(-1)
        rows, rr = np.zeros((nq, len(depths or DEPTHS(n))), np.int64), np.zeros((nq, len(depths or DEPTHS(n))), np.int64)
        for j in range(nq):
            pos = np.flatnonzero(_best_positions(order[j], inv, inv.max() + 1))
            for c, r0 in enumerate(depths or DEPTHS(n)):
                i = np.searchsorted(pos, r0)
                rr[j, c] = pos[i] if i < len(pos) else pos[-1]
                rows[j, c] = order[j, rr[j, c]]
        ids = col[rows]
        want = RC.ranks(S, col, ids)
        for a in (rows, rr, ids, want):
            a.setflags(write=False)
        _TARGETS[key] = (rows, rr, ids, want)
    return _TARGETS[key]


def _rank(idx, Q, ids, allowed=None, ordinals=None):
    """rank_ids over a poisoned workspace, twice with different poison; returns (ranks, stats of the first call)"""
    if idx._ws is not None:
        fill_bytes(idx._ws, "R", 1)
    got = idx.rank_ids(Q, ids, allowed=allowed, ordinals=ordinals)
    stats = dict(idx.stats)
    assert got.dtype == np.int64 and got.shape == np.asarray(ids).shape
    fill_bytes(idx._ws, "N", 2)
    np.testing.assert_array_equal(idx.rank_ids(Q, ids, allowed=allowed, ordinals=ordinals), got,
                                  err_msg="the result depends on stale workspace bytes")
    return got, stats


# ---- ordinals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 5000, 20000])
def test_ordinals_are_bit_equal_to_the_oracle(torch_cuda, n):
    torch = torch_cuda
    from convdr_amd.search import FlatIPIndex
    idx = FlatIPIndex(64, prepin=False)
    idx.add(synth_corpus(5, n, 64), ids=np.array(DC.case(DC.FAMILIES[0], n, 40)[0]))
    for family in DC.FAMILIES:
        col = DC.case(family, n, 40)[0]
        idx._sid = torch.from_numpy(np.array(col)).cuda()
        want, ndocs = RC.ordinals(col)
        runs = []
        for fill, seed in (("R", 3), ("N", 4)):
            if getattr(idx, "_key_ws", None) is not None:
                fill_bytes(idx._key_ws, fill, seed)
            o = idx.doc_ordinals()
            assert o.n == n and o.ndocs == ndocs and o.ord.is_cuda and tuple(o.ord.shape) == (n,), family
            runs.append(o.ord.cpu().numpy().view(np.uint32))
        np.testing.assert_array_equal(runs[0], want, err_msg=family)
        assert runs[0].tobytes() == runs[1].tobytes(), family
        assert want.max() == ndocs - 1 and (family != "interleaved" or (want[3::4] == want[3]).all())


def test_ordinals_entry_flags_the_reserved_key_and_handles_an_empty_column(torch_cuda):
    torch = torch_cuda
    from convdr_amd import _lib
    from convdr_amd import search as S
    L, ptr = _lib.lib(), _lib.ptr
    col = np.array(DC.case("chunks", 300, 40)[0])
    col[[0, 299]] = K.I64_MIN
    keep = col != K.I64_MIN
    want, ndocs = RC.ordinals(col[keep])
    for n, c in ((300, col), (0, col[:0])):
        need = L.convdr_doc_ordinals_workspace_bytes(n)
        ws = fill_bytes(torch.empty(need, dtype=torch.uint8, device="cuda"), "R", 8)
        out = fill_bytes(torch.empty(n + 8, dtype=torch.int32, device="cuda"), "N", 0)
        nd = fill_bytes(torch.empty(1, dtype=torch.int64, device="cuda"), "N", 0)
        cd = torch.from_numpy(c).cuda()
        assert L.convdr_doc_ordinals(ptr(cd) if n else None, n, ptr(ws), need - 1, ptr(out), ptr(nd), _lib.stream_ptr()) < 0
        assert b"workspace too small" in L.convdr_last_error()
        assert L.convdr_doc_ordinals(ptr(cd) if n else None, n, ptr(ws), need, ptr(out), ptr(nd), _lib.stream_ptr()) == 0
        got = out.cpu().numpy().view(np.uint32)
        assert (got[n:] == 0xFFFFFFFF).all()                                   # nothing past ord[n - 1] was written
        if n:
            assert int(nd.item()) == ndocs and int(ws[:4].view(torch.int32).item()) == S.KEY_ST_COLUMN
            np.testing.assert_array_equal(got[:n][keep], want)
            assert (got[:n][~keep] == 0xFFFFFFFF).all()
        else:
            assert int(nd.item()) == 0 and int(ws[:4].view(torch.int32).item()) == 0


# ---- ranks -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,precision", CONFIGS)
@pytest.mark.parametrize("n,nq,d,clustered", SHAPES)
def test_documents_through_the_depth(torch_cuda, n, nq, d, clustered, storage, precision):
    torch = torch_cuda
    shape = (n, nq, d, clustered)
    _, Q = _corpus(shape)
    col = _column(n)
    rows, rr, ids, want = _targets(shape)
    assert (want <= rr).all() and (want[:, 3:] < rr[:, 3:]).any()        # (chunked: a document rank is below the row rank)
    idx = _doc_index(torch, shape, storage, precision, col)
    got, stats = _rank(idx, Q, ids)
    np.testing.assert_array_equal(got, want)
    assert stats["rank_fallback_pairs"] == 0 and stats["rank_cap"] >= 4096 and stats["ndocs"] == len(np.unique(col))
    assert stats["ndocs"] % 32
    k = 10
    Dd, Id, Rd, _ = idx.search_docs(Q, k)
    Id, Rd = Id.cpu().numpy(), Rd.cpu().numpy()
    shallow = 0
    for j in range(nq):
        for c in range(ids.shape[1]):
            if got[j, c] < k:
                assert Id[j, got[j, c]] == ids[j, c] and Rd[j, got[j, c]] == rows[j, c]
                shallow += 1
    assert shallow >= 2 * nq
    # (D, R) is the MaxP pair of score_ids_tensors; device ids; precomputed ordinals
    o = idx.doc_ordinals()
    rk, D, R = idx.rank_ids_tensors(Q, torch.from_numpy(np.array(ids)).cuda(), ordinals=o)
    D2, R2 = idx.score_ids_tensors(Q, ids)
    assert rk.dtype == torch.int64 and rk.is_cuda and tuple(rk.shape) == ids.shape
    assert torch.equal(D, D2) and torch.equal(R, R2)
    np.testing.assert_array_equal(R.cpu().numpy(), rows)
    np.testing.assert_array_equal(rk.cpu().numpy(), want)
    # 1-D ids, ids on no row and the reserved id
    got1, _ = _rank(idx, Q, np.ascontiguousarray(ids[:, 4]), ordinals=o)
    np.testing.assert_array_equal(got1, want[:, 4])
    ids2, want2 = ids.copy(), want.copy()
    ids2[:, 1], ids2[:, 2] = 123_456_789_000, K.I64_MIN
    want2[:, 1:3] = -1
    got2, _ = _rank(idx, Q, ids2, ordinals=o)
    np.testing.assert_array_equal(got2, want2)


@pytest.mark.parametrize("storage,precision", CONFIGS)
def test_distinct_ids_reduce_to_rank_rows(torch_cuda, storage, precision):
    torch = torch_cuda
    shape = (5000, 37, 768, False)
    n = shape[0]
    _, Q = _corpus(shape)
    col = np.arange(n, dtype=np.int64) * 7 - 3
    idx = _doc_index(torch, shape, storage, precision, col)
    rows = np.ascontiguousarray(_order(shape)[:, DEPTHS(n)])
    got, stats = _rank(idx, Q, col[rows])
    np.testing.assert_array_equal(got, np.tile(np.asarray(DEPTHS(n), np.int64), (shape[1], 1)))
    np.testing.assert_array_equal(got, idx.rank_rows(Q, rows))
    assert stats["ndocs"] == n


@pytest.mark.parametrize("storage,precision", [c for c in CONFIGS if c[0] == "fp32"])
@pytest.mark.parametrize("n,nq,d,clustered", [s for s in SHAPES if not s[3]])
def test_deep_documents_are_counted_not_rescored(torch_cuda, n, nq, d, clustered, storage, precision):
    """The selection rule of test_deep_targets_are_counted_not_rescored, applied to best rows: the documented eps on the CPU,
    and a target qualifies only if the rows within 2 eps of its score are at most half its row rank.  The thresholds are those
    of rank_rows, so the band is the same: one pass, most of the rank comes from marks, the band is at most half the row rank."""
    torch = torch_cuda
    shape = (n, nq, d, clustered)
    P, Q = _corpus(shape)
    S, col = _scores(shape), _column(n)
    depths = (n // 4, n // 2, 3 * n // 4, 7 * n // 8)
    rows, rr, ids, want = _targets(shape, depths)
    idx = _doc_index(torch, shape, storage, precision, col)
    idx.cap = 16384             # (no band of these shapes overflows it: one pass)
    o = idx.doc_ordinals()
    eps = _documented_eps(shape, precision, Q, P)
    tested = set()
    for j in range(min(nq, 3)):
        for c, r0 in enumerate(depths):
            t, r = int(rows[j, c]), int(rr[j, c])
            room = int((np.abs(S[j] - S[j, t]) <= 2 * eps[j]).sum())
            if room > r // 2:
                continue
            got, stats = _rank(idx, Q[j:j + 1], np.asarray([ids[j, c]]), ordinals=o)
            print("n=%d d=%d %s row rank=%d doc rank=%d: above=%d band=%d (2 eps on the CPU: %d rows)"
                  % (n, d, precision, r, want[j, c], stats["rank_above"], stats["rank_band_rows"], room))
            assert got[0] == want[j, c]
            assert stats["rank_rounds"] == 1
            assert stats["rank_above"] > 0 and stats["rank_band_rows"] <= r // 2, stats
            assert 1 <= stats["rank_band_rows"] <= room and stats["rank_above"] <= r
            tested.add(r0)
    assert tested and (precision == "bf16" or n // 4 in tested), tested


@pytest.mark.parametrize("storage,precision", CONFIGS)
def test_one_document_on_thousands_of_rows_is_counted_once(torch_cuda, storage, precision):
    from convdr_amd.search import FlatIPIndex
    n = 20000
    col = DC.interleaved(n)
    P = synth_corpus(31, n, 64).astype(np.float16).astype(np.float32)
    Q = synth_corpus(32, 2, 64)
    S = OS.canonical_scores(Q, P)
    idx = FlatIPIndex(64, storage=storage, precision=precision, prepin=False)
    idx.add(P.astype(np.float16) if storage == "fp16" else P, ids=np.array(col))
    ids = np.zeros((2, 3), np.int64)
    for j in range(2):
        order = np.lexsort((np.arange(n), -S[j]))
        deep = next(int(r) for r in order[n // 2:] if col[r] != DC.BIG_ID and RC.best_row(S[j], col, col[r]) == r)
        big_before = int(((S[j] > S[j, deep]) & (col == DC.BIG_ID)).sum())
        assert big_before > 1000                        # thousands of rows of the one document precede the target ...
        ids[j] = [col[deep], DC.BIG_ID, col[order[3 * n // 4]]]
    want = RC.ranks(S, col, ids)
    got, stats = _rank(idx, Q, ids)
    np.testing.assert_array_equal(got, want)            # ... and count once; none of its 5,000 rows counts against itself
    assert (want[:, 1] < 40).all() and stats["rank_fallback_pairs"] == 0


@pytest.mark.parametrize("storage,precision", CONFIGS)
def test_exact_duplicates_in_other_documents_are_ordered_by_row(torch_cuda, storage, precision):
    from convdr_amd.search import FlatIPIndex
    P = synth_corpus(21, 600, 64).astype(np.float16).astype(np.float32)
    Q = synth_corpus(22, 3, 64)
    t = 300
    P[[10, 100, 200, 400, 500]] = P[t]          # three copies below the target's best row, two above it
    col = DC.chunked_ids(600)
    col[[10, 100, 200, t, 400, 500]] = 9_000_000_000 + np.arange(6)        # six documents of one row ...
    col[401] = col[400]                                                    # ... and one that has a second row
    S = OS.canonical_scores(Q, P)
    ndocs = len(np.unique(col))
    idx = FlatIPIndex(64, storage=storage, precision=precision, prepin=False)
    idx.add(P.astype(np.float16) if storage == "fp16" else P, ids=col)
    ids = np.tile(col[[t, 10, 100, 200, 400, 500]], (3, 1))
    want = RC.ranks(S, col, ids)
    for j in range(3):
        assert (S[j] == S[j, t]).sum() == 6
        a = want[j, 1]          # the documents with a row that scores strictly above; the tying ones below row t precede it
        assert want[j].tolist()[:4] == [a + 3, a, a + 1, a + 2]
        # (the document of row 400 is among those `a` when its other row beats the tie, else its tying row 400 precedes 500)
        assert want[j, 5] == a + 4 + (1 if S[j, 401] < S[j, t] else 0)
    got, _ = _rank(idx, Q, ids)
    np.testing.assert_array_equal(got, want)
    _, Id, _, _ = idx.search_docs(Q, ndocs)
    Id = Id.cpu().numpy()
    assert all(len(np.unique(Id[j])) == ndocs for j in range(3))          # every document once, no padding
    got, _ = _rank(idx, Q, Id)                  # position for position
    np.testing.assert_array_equal(got, np.tile(np.arange(ndocs), (3, 1)))


@pytest.mark.parametrize("storage,precision", CONFIGS)
def test_all_zero_query_the_rank_is_the_ordinal(torch_cuda, storage, precision):
    """Every score is 0: a document's best row is its first row and its rank the number of documents that begin below it --
    its ordinal.  The whole block is the band: it overflows the first list of 4,096 and is re-run once at 8,192."""
    torch = torch_cuda
    shape = (5000, 37, 768, False)
    n = shape[0]
    col = _column(n)
    ordv, ndocs = RC.ordinals(col)
    idx = _doc_index(torch, shape, storage, precision, col)
    Q0 = np.zeros((2, 768), np.float32)
    ids = np.asarray([[col[0], col[1], col[2500]], [col[n - 1], col[4097], 123_456_789_000]], np.int64)
    first = np.asarray([[int(np.flatnonzero(col == k)[0]) if (col == k).any() else -1 for k in r] for r in ids])
    want = np.where(first >= 0, ordv[np.maximum(first, 0)].astype(np.int64), -1)
    got, stats = _rank(idx, Q0, ids)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, RC.ranks(np.zeros((2, n)), col, ids))
    assert stats["rank_rounds"] == 2 and stats["rank_cap"] == 8192 and stats["rank_above"] == 0, stats
    mask = _mask(n, "half")
    got, _ = _rank(idx, Q0, ids, allowed=mask)
    wantm = np.asarray([[len(np.unique(col[:f][mask[:f]])) if f >= 0 else -1 for f in r] for r in first], np.int64)
    np.testing.assert_array_equal(got, wantm)
    np.testing.assert_array_equal(got, RC.ranks(np.zeros((2, n)), col, ids, mask))


@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("storage,precision", CONFIGS)
@pytest.mark.parametrize("n,nq,d", [(5000, 37, 768), (300, 3, 64)])
def test_row_filter(torch_cuda, n, nq, d, storage, precision, name):
    torch = torch_cuda
    shape = (n, nq, d, False)
    _, Q = _corpus(shape)
    S, order, col = _scores(shape), _order(shape), _column(n)
    mask = _mask(n, name)
    allowed_rows, other_rows = np.flatnonzero(mask), np.flatnonzero(~mask)
    cols = [order[:, n // 2], order[:, 5], order[:, n - 1], np.full(nq, other_rows[len(other_rows) // 2]), np.full(nq, other_rows[0])]
    if len(allowed_rows):
        cols += [np.full(nq, allowed_rows[0]), np.full(nq, allowed_rows[-1])]
    ids = col[np.stack(cols, 1)]
    best = np.asarray([[RC.best_row(S[j], col, int(k)) for k in ids[j]] for j in range(nq)])
    want = RC.ranks(S, col, ids, mask)
    if name == "none":
        assert (want == 0).all()
    else:
        # targets whose best row is not allowed everywhere; both kinds where the mask is wide enough to hold a best row
        assert not mask[best].all() and want.max() > 0 and (name != "half" or mask[best].any())
    idx = _doc_index(torch, shape, storage, precision, col)
    got, _ = _rank(idx, Q, ids, allowed=mask)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(idx.rank_ids(Q, ids, allowed=idx.row_filter(mask)), want)
    if name == "half":          # the position in the filtered document search is the rank
        k = 50
        _, Id, Rd, _ = idx.search_docs(Q, k, allowed=mask)
        Id, Rd = Id.cpu().numpy(), Rd.cpu().numpy()
        placed = 0
        for j in range(nq):
            for c in range(ids.shape[1]):
                if mask[best[j, c]] and want[j, c] < k:
                    assert Id[j, want[j, c]] == ids[j, c] and Rd[j, want[j, c]] == best[j, c]
                    placed += 1
        assert placed >= nq


@pytest.mark.parametrize("storage,precision", CONFIGS)
def test_band_overflow_is_rerun_once_at_the_reported_size(torch_cuda, storage, precision):
    torch = torch_cuda
    shape = (5000, 37, 768, False)
    n = shape[0]
    _, Q = _corpus(shape)
    S, col = _scores(shape), _column(n)
    rows, _, ids, _ = _targets(shape)
    idx = _doc_index(torch, shape, storage, precision, col)
    Q3 = np.stack([Q[0], np.zeros(768, np.float32), Q[1]])
    S3 = np.stack([S[0], np.zeros(n), S[1]])
    ids3 = np.asarray([ids[0, 2], col[1234], ids[1, 1]], np.int64)
    try:
        idx.cap = 1024          # the smallest list the entry accepts: the zero query's band of n rows overflows it
        got, stats = _rank(idx, Q3, ids3)
    finally:
        idx.cap = 4096
    np.testing.assert_array_equal(got, RC.ranks(S3, col, ids3))
    assert stats["rank_rounds"] == 2 and stats["rank_cap"] == 8192 and stats["rank_fallback_pairs"] == 0, stats


@pytest.mark.parametrize("storage,precision", CONFIGS)
def test_a_band_beyond_the_longest_list_takes_the_fallback(torch_cuda, storage, precision):
    torch = torch_cuda
    shape = (5000, 37, 768, False)
    n = shape[0]
    _, Q = _corpus(shape)
    S, col = _scores(shape), _column(n)
    _, _, ids, _ = _targets(shape)
    idx = _doc_index(torch, shape, storage, precision, col)
    Q2 = np.stack([np.zeros(768, np.float32), Q[0]])
    S2 = np.stack([np.zeros(n), S[0]])
    ids2 = np.asarray([[col[4321], col[7]], [ids[0, 4], ids[0, 2]]], np.int64)
    mask = _mask(n, "half")
    try:
        idx.cap, idx.RANGE_MAX_CAP = 1024, 2048
        got, stats = _rank(idx, Q2, ids2)
        gotm, statsm = _rank(idx, Q2, ids2, allowed=mask)
    finally:
        idx.cap, idx.RANGE_MAX_CAP = 4096, 131072
    np.testing.assert_array_equal(got, RC.ranks(S2, col, ids2))
    np.testing.assert_array_equal(gotm, RC.ranks(S2, col, ids2, mask))
    assert stats["rank_fallback_pairs"] == 2 and statsm["rank_fallback_pairs"] == 2, (stats, statsm)


def test_empty_index_no_ids_stale_filter_and_stale_ordinals(torch_cuda):
    from convdr_amd.search import FlatIPIndex
    P, Q = synth_corpus(3, 600, 64), synth_corpus(4, 2, 64)
    col = DC.chunked_ids(600)
    idx = FlatIPIndex(64, prepin=False)
    with pytest.raises(ValueError, match="no row ids"):
        idx.rank_ids(Q, col[:2])
    with pytest.raises(ValueError, match="no row ids"):
        idx.doc_ordinals()
    idx.add(P[:500], ids=col[:500])
    f, o = idx.row_filter(np.ones(500, bool)), idx.doc_ordinals()
    assert o.n == 500 and o.ndocs == len(np.unique(col[:500]))
    assert idx.rank_ids(Q, col[:2], allowed=f, ordinals=o).shape == (2,)
    idx.add(P[500:], ids=col[500:])
    with pytest.raises(ValueError, match="stale RowFilter"):
        idx.rank_ids(Q, col[:2], allowed=f)
    with pytest.raises(ValueError, match="stale DocOrdinals"):
        idx.rank_ids(Q, col[:2], ordinals=o)
    with pytest.raises(ValueError):
        idx.rank_ids(Q, col[:3])
    assert idx.remove_ids(np.unique(col)) == 600 and idx.ntotal == 0       # an empty index that carries ids
    assert idx.doc_ordinals().ndocs == 0
    assert idx.rank_ids(Q, col[:2]).tolist() == [-1, -1]


@pytest.mark.parametrize("storage,precision", CONFIGS)
def test_c_entry_directly(torch_cuda, storage, precision):
    """convdr_ip_rank_docs through ctypes at cap = 1,024: refused with a workspace one byte short and with a NULL output, each
    with its reason; then one call over a poisoned workspace and outputs.  The entry answers for ANY row: the documents ahead
    of it other than its own."""
    torch = torch_cuda
    from convdr_amd import _lib
    shape = (5000, 37, 768, False)
    n, nq, d, _ = shape
    _, Q = _corpus(shape)
    S, order, col = _scores(shape), _order(shape), _column(n)
    idx = _doc_index(torch, shape, storage, precision, col)
    o = idx.doc_ordinals()
    L, ptr = _lib.lib(), _lib.ptr
    store = 2 if idx.storage == "fp16" else (1 if idx.kind == "f16" else 0)
    cap = 1024
    Qp = np.concatenate([Q[:5], np.zeros((1, d), np.float32)])
    tgt = np.asarray([order[0, 0], order[1, 7], order[2, n - 1], -1, n, 99], np.int64)
    npairs = len(tgt)
    need = L.convdr_ip_rank_docs_workspace_bytes(npairs, n, d, cap, o.ndocs)
    assert need > L.convdr_ip_rank_workspace_bytes(npairs, n, d, cap) > 0
    q, t = torch.from_numpy(Qp).cuda(), torch.from_numpy(tgt).cuda()
    ws = fill_bytes(torch.empty(need, dtype=torch.uint8, device="cuda"), "R", 5)
    rank = fill_bytes(torch.empty(npairs, dtype=torch.int64, device="cuda"), "R", 6)
    X = fill_bytes(torch.empty(npairs, dtype=torch.float64, device="cuda"), "R", 7)
    cnt = fill_bytes(torch.empty(npairs, dtype=torch.int64, device="cuda"), "R", 8)
    above = fill_bytes(torch.empty(npairs, dtype=torch.int64, device="cuda"), "R", 9)
    st = fill_bytes(torch.empty(npairs, dtype=torch.int32, device="cuda"), "R", 10)

    def call(ws_bytes=need, outs=None, ordp=o.ord):
        out = [rank, X, cnt, above, st] if outs is None else outs
        return L.convdr_ip_rank_docs(store, ptr(q), npairs, ptr(t), None if idx.storage == "fp16" else ptr(idx._rows), ptr(idx._pbf),
                                     float(idx._scale) if store else 1.0, None if idx.storage == "fp16" else ptr(idx._centre), n, d,
                                     ptr(idx._max_norm), None, 0, 0, ptr(ordp), o.ndocs, cap, ptr(ws), ws_bytes, *[ptr(x) for x in out],
                                     _lib.stream_ptr())
    assert call(ws_bytes=need - 1) < 0 and b"workspace too small" in L.convdr_last_error()
    assert b"convdr_ip_rank_docs" in L.convdr_last_error()
    for i in range(5):
        outs = [rank, X, cnt, above, st]
        outs[i] = None
        assert call(outs=outs) < 0 and b"NULL argument" in L.convdr_last_error(), i
    assert call(ordp=None) < 0 and b"ord is NULL" in L.convdr_last_error()
    assert call() == 0, L.convdr_last_error()
    torch.cuda.synchronize()
    rank, X, cnt, above, st = (x.cpu().numpy() for x in (rank, X, cnt, above, st))
    assert st.tolist() == [0, 0, 0, 0, 0, 1]

    def ahead(s, r):
        prec = ((s > s[r]) | ((s == s[r]) & (np.arange(n) < r))) & (col != col[r])
        return len(np.unique(col[prec]))
    assert rank.tolist() == [0, ahead(S[1], tgt[1]), ahead(S[2], tgt[2]), -1, -1, -1]
    assert cnt[5] == n and above[5] == 0 and cnt[3] == cnt[4] == 0 and above[3] == above[4] == 0
    np.testing.assert_array_equal(X[:3].view(np.uint64), S[[0, 1, 2], tgt[:3]].view(np.uint64))
    assert X[3] == X[4] == np.float64(PAD) and X[5] == 0.0
    row_rank = np.asarray([0, 7, n - 1])
    assert (above[:3] <= row_rank).all() and (above[:3] + cnt[:3] >= row_rank + 1).all() and (cnt[:3] >= 1).all()
