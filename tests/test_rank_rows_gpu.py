"""Exact score and rank of given rows: FlatIPIndex.score_rows / rank_rows / convdr_ip_score_rows / convdr_ip_rank_rows.

Expected values everywhere, no tolerances: with S = oracle.search.canonical_scores(Q, P), the score of row t for query j is
S[j, t] (fp64, bit for bit; D its fp32 rounding) and its rank is #{r : S[j, r] > S[j, t]} + #{r < t : S[j, r] == S[j, t]}, taken
over the allowed rows when there is a mask.  Both stores hold the SAME corpus (rounded to half and widened), so one oracle run
per shape serves every store and precision (the shapes and configurations of test_range_search_gpu.py).  Every rank call runs
twice, over a workspace poisoned with two different byte patterns, and must return the same ranks."""
import numpy as np
import pytest

from oracle import search as OS
from tests.golden.make_golden import synth_corpus
from tests.helpers import fill_bytes
from tests.index_cases import CONFIGS, MASKS, SHAPES, torch_cuda      # noqa: F401 (torch_cuda: the fixture, by name)
from tests.index_cases import corpus as _corpus, index as _index, mask as _mask, scores as _scores

pytestmark = pytest.mark.gpu

PAD = np.float32(-3.4028234663852886e38)

_ORDER = {}


def _order(shape):
    """order[j, r] = the row at rank r of query j in the canonical order"""
    if shape not in _ORDER:
        S = _scores(shape)
        idx = np.arange(S.shape[1])
        o = np.stack([np.lexsort((idx, -S[j])) for j in range(S.shape[0])])
        o.setflags(write=False)
        _ORDER[shape] = o
    return _ORDER[shape]


def _oracle_rank(s, t, mask=None):
    """rank of row t among the (allowed) rows for one query's scores s; -1 for padding"""
    if t < 0:
        return -1
    m = np.ones(len(s), bool) if mask is None else mask
    return int(((s > s[t]) & m).sum() + ((s == s[t]) & m & (np.arange(len(s)) < t)).sum())


def _oracle_ranks(S, rows, mask=None):
    rows2 = rows.reshape(S.shape[0], -1)
    return np.asarray([[_oracle_rank(S[j], int(t), mask) for t in rows2[j]] for j in range(S.shape[0])], np.int64).reshape(rows.shape)


def _rank(idx, Q, rows, allowed=None):
    """rank_rows over a poisoned workspace, twice with different poison; returns (ranks, stats of the first call)"""
    if idx._ws is not None:
        fill_bytes(idx._ws, "R", 1)
    got = idx.rank_rows(Q, rows, allowed=allowed)
    stats = dict(idx.stats)
    assert got.dtype == np.int64 and got.shape == np.asarray(rows).shape
    fill_bytes(idx._ws, "N", 2)
    np.testing.assert_array_equal(idx.rank_rows(Q, rows, allowed=allowed), got, err_msg="the result depends on stale workspace bytes")
    return got, stats


@pytest.mark.parametrize("storage,precision", CONFIGS)
@pytest.mark.parametrize("n,nq,d,clustered", SHAPES)
def test_scores_are_the_canonical_scores(torch_cuda, n, nq, d, clustered, storage, precision):
    torch = torch_cuda
    shape = (n, nq, d, clustered)
    _, Q = _corpus(shape)
    S = _scores(shape)
    idx = _index(shape, storage, precision)
    k = 10
    D, I = idx.search(Q, k)
    np.testing.assert_array_equal(I, _order(shape)[:, :k])
    got = idx.score_rows(Q, I)
    assert got.dtype == np.float32 and got.shape == (nq, k)
    np.testing.assert_array_equal(got.view(np.uint32), D.view(np.uint32))
    rs = np.random.RandomState(3)
    for m in (1, 7):
        rows = rs.randint(0, n, size=(nq, m)).astype(np.int64)
        rows[rs.rand(nq, m) < 0.25] = -1
        rows[0, 0], rows[-1, -1] = n - 1, 0
        want = np.where(rows >= 0, np.take_along_axis(S, np.maximum(rows, 0), 1), np.float64(PAD))
        D32, X = idx.score_rows_tensors(Q, rows)
        assert D32.dtype == torch.float32 and X.dtype == torch.float64 and tuple(X.shape) == (nq, m)
        np.testing.assert_array_equal(X.cpu().numpy().view(np.uint64), want.view(np.uint64))
        np.testing.assert_array_equal(D32.cpu().numpy().view(np.uint32), want.astype(np.float32).view(np.uint32))
        np.testing.assert_array_equal(idx.score_rows(Q, torch.from_numpy(rows).cuda()), want.astype(np.float32))
    rows = rs.randint(0, n, size=nq).astype(np.int64)           # 1-D: one row per query
    got = idx.score_rows(Q, rows)
    assert got.shape == (nq,)
    np.testing.assert_array_equal(got, S[np.arange(nq), rows].astype(np.float32))
    # an id past the end inside a DEVICE tensor is not read on the host and not dereferenced on the device: padding
    far = torch.full((nq, 2), n, dtype=torch.int64, device="cuda")
    far[:, 1] = 1 << 40
    assert (idx.score_rows(Q, far) == PAD).all()
    with pytest.raises(ValueError):
        idx.score_rows(Q, np.full(nq, n, np.int64))


@pytest.mark.parametrize("storage,precision", CONFIGS)
@pytest.mark.parametrize("n,nq,d,clustered", SHAPES)
def test_targets_through_the_depth(torch_cuda, n, nq, d, clustered, storage, precision):
    shape = (n, nq, d, clustered)
    _, Q = _corpus(shape)
    S, order = _scores(shape), _order(shape)
    idx = _index(shape, storage, precision)
    k = 10
    ranks = [0, 1, k - 1, n // 4, n // 2, n - 1]
    rows = np.ascontiguousarray(order[:, ranks])
    want = np.tile(np.asarray(ranks, np.int64), (nq, 1))
    np.testing.assert_array_equal(_oracle_ranks(S, rows), want)            # (untied data: the oracle's rank is the position)
    got, stats = _rank(idx, Q, rows)
    np.testing.assert_array_equal(got, want)
    _, I = idx.search(Q, k)
    for j in range(nq):
        for c in range(3):
            assert I[j, got[j, c]] == rows[j, c]
    assert stats["rank_fallback_pairs"] == 0 and stats["rank_cap"] >= 4096
    # padding and 1-D rows
    rows1 = rows[:, 4].copy()
    got1, _ = _rank(idx, Q, rows1)
    np.testing.assert_array_equal(got1, want[:, 4])
    rows[:, 1] = -1
    got, _ = _rank(idx, Q, rows)
    want[:, 1] = -1
    np.testing.assert_array_equal(got, want)


def _documented_eps(shape, precision, Q, P):
    """the band (IpBand::eps, csrc/ip_certify.hpp) in UNSCALED units, from the coefficients documented in csrc/ip_topk.hip
    (ip_eps_coef): per query, coef |q| max|p - centre|, +1 % for the fp16 scan's absolute term (about 0.1 % at these scales) and the 1.001 factors"""
    d_pad = (shape[2] + 63) // 64 * 64
    u = 2.0 ** -8 if precision == "bf16" else 2.0 ** -11
    coef = 2 * u + u * u + d_pad / 8388608.0
    pmax = np.linalg.norm(P.astype(np.float64) - P.astype(np.float64).mean(0), axis=1).max()
    return 1.01 * coef * np.linalg.norm(Q.astype(np.float64), axis=1) * pmax


@pytest.mark.parametrize("storage,precision", [c for c in CONFIGS if c[0] == "fp32"])
@pytest.mark.parametrize("n,nq,d,clustered", [s for s in SHAPES if not s[3]])
def test_deep_targets_are_counted_not_rescored(torch_cuda, n, nq, d, clustered, storage, precision):
    """The regime the feature exists for: a deep target's rank comes mostly from the counter, and the band that is re-scored
    is at most half the rank.  A rank is tested when the documented eps, evaluated here on the CPU, leaves that room even if
    every row within 2 eps of the target's score were listed (the scan score of a row is within eps of its exact score, the
    band is eps wide on either side); n / 4 must qualify for the fp16 scan."""
    shape = (n, nq, d, clustered)
    P, Q = _corpus(shape)
    S, order = _scores(shape), _order(shape)
    idx = _index(shape, storage, precision)
    idx.cap = 16384             # (no band of these shapes overflows it: one pass, the counters are one call's)
    eps = _documented_eps(shape, precision, Q, P)
    tested = set()
    for j in range(min(nq, 3)):
        for r in (n // 4, n // 2, 3 * n // 4, 7 * n // 8):
            t = int(order[j, r])
            room = int((np.abs(S[j] - S[j, t]) <= 2 * eps[j]).sum())
            if room > r // 2:
                continue
            got, stats = _rank(idx, Q[j:j + 1], np.asarray([t]))
            print("n=%d d=%d %s rank=%d: above=%d band=%d (2 eps on the CPU: %d rows)" % (n, d, precision, r, stats["rank_above"],
                                                                                        stats["rank_band_rows"], room))
            assert got[0] == r
            assert stats["rank_rounds"] == 1
            assert stats["rank_above"] > 0 and stats["rank_band_rows"] <= r // 2, stats
            assert 1 <= stats["rank_band_rows"] <= room and stats["rank_above"] <= r       # (the target itself is in the band)
            tested.add(r)
    assert tested and (precision == "bf16" or n // 4 in tested), tested


@pytest.mark.parametrize("storage,precision", CONFIGS)
def test_exact_duplicates_are_ordered_by_row(torch_cuda, storage, precision):
    from convdr_amd.search import FlatIPIndex
    P = synth_corpus(21, 600, 64).astype(np.float16).astype(np.float32)
    Q = synth_corpus(22, 3, 64)
    t = 300
    P[[10, 100, 200, 400, 500]] = P[t]          # three copies below the target's index, two above it
    S = OS.canonical_scores(Q, P)
    idx = FlatIPIndex(64, storage=storage, precision=precision, prepin=False)
    idx.add(P.astype(np.float16) if storage == "fp16" else P)
    rows = np.tile(np.asarray([t, 10, 100, 200, 400, 500, 0], np.int64), (3, 1))
    want = _oracle_ranks(S, rows)
    for j in range(3):
        above = int((S[j] > S[j, t]).sum())
        assert (S[j] == S[j, t]).sum() == 6
        assert want[j].tolist()[:6] == [above + 3, above, above + 1, above + 2, above + 4, above + 5]
    got, _ = _rank(idx, Q, rows)
    np.testing.assert_array_equal(got, want)
    _, I = idx.search(Q, 600)
    for j in range(3):
        np.testing.assert_array_equal(I[j, got[j]], rows[j])


@pytest.mark.parametrize("storage,precision", CONFIGS)
def test_all_zero_query_every_score_ties(torch_cuda, storage, precision):
    """Every score is 0: the rank of a row is its index among the allowed rows, the whole block is the band -- which overflows
    the first list of 4,096 and is re-run once at 8,192."""
    shape = (5000, 37, 768, False)
    n = shape[0]
    idx = _index(shape, storage, precision)
    Q0 = np.zeros((2, 768), np.float32)
    rows = np.asarray([[0, 1, 2500], [n - 1, 4097, -1]], np.int64)
    got, stats = _rank(idx, Q0, rows)
    np.testing.assert_array_equal(got, rows)
    assert stats["rank_rounds"] == 2 and stats["rank_cap"] == 8192 and stats["rank_above"] == 0
    assert stats["rank_band_rows"] == 5 * (4096 + n)
    mask = _mask(n, "half")
    got, _ = _rank(idx, Q0, rows, allowed=mask)
    before = np.concatenate([[0], np.cumsum(mask)])
    np.testing.assert_array_equal(got, np.where(rows >= 0, before[np.maximum(rows, 0)], -1))
    assert mask[rows[rows >= 0]].any() and not mask[rows[rows >= 0]].all()


@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("storage,precision", CONFIGS)
@pytest.mark.parametrize("n,nq,d", [(5000, 37, 768), (300, 3, 64)])
def test_row_filter(torch_cuda, n, nq, d, storage, precision, name):
    shape = (n, nq, d, False)
    _, Q = _corpus(shape)
    S, order = _scores(shape), _order(shape)
    mask = _mask(n, name)
    allowed_rows, other_rows = np.flatnonzero(mask), np.flatnonzero(~mask)
    cols = [order[:, n // 2], order[:, 5], order[:, n - 1], np.full(nq, other_rows[len(other_rows) // 2]),
            np.full(nq, other_rows[0])]
    if len(allowed_rows):
        cols += [np.full(nq, allowed_rows[0]), np.full(nq, allowed_rows[-1])]
    rows = np.stack(cols, 1).astype(np.int64)
    want = _oracle_ranks(S, rows, mask)
    if name == "none":
        assert (want == 0).all()
    else:
        assert mask[rows].any() and not mask[rows].all() and want.max() > 0
    idx = _index(shape, storage, precision)
    got, _ = _rank(idx, Q, rows, allowed=mask)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(idx.rank_rows(Q, rows, allowed=idx.row_filter(mask)), want)
    if name == "half":          # the position in the filtered search is the rank
        k = 50
        _, I = idx.search(Q, k, allowed=mask)
        for j in range(nq):
            for c in range(rows.shape[1]):
                if mask[rows[j, c]] and want[j, c] < k:
                    assert I[j, want[j, c]] == rows[j, c]


@pytest.mark.parametrize("storage,precision", CONFIGS)
def test_band_overflow_is_rerun_once_at_the_reported_size(torch_cuda, storage, precision):
    shape = (5000, 37, 768, False)
    n = shape[0]
    _, Q = _corpus(shape)
    S, order = _scores(shape), _order(shape)
    idx = _index(shape, storage, precision)
    Q3 = np.stack([Q[0], np.zeros(768, np.float32), Q[1]])
    S3 = np.stack([S[0], np.zeros(n), S[1]])
    rows = np.asarray([order[0, 5], 1234, order[1, 3]], np.int64)
    try:
        idx.cap = 1024          # the smallest list the entry accepts: the zero query's band of n rows overflows it
        got, stats = _rank(idx, Q3, rows)
    finally:
        idx.cap = 4096
    np.testing.assert_array_equal(got, _oracle_ranks(S3, rows))
    assert got.tolist() == [5, 1234, 3]
    assert stats["rank_rounds"] == 2 and stats["rank_cap"] == 8192 and stats["rank_fallback_pairs"] == 0, stats


@pytest.mark.parametrize("storage,precision", CONFIGS)
def test_a_band_beyond_the_longest_list_takes_the_fallback(torch_cuda, storage, precision):
    shape = (5000, 37, 768, False)
    n = shape[0]
    _, Q = _corpus(shape)
    S, order = _scores(shape), _order(shape)
    idx = _index(shape, storage, precision)
    Q2 = np.stack([np.zeros(768, np.float32), Q[0]])
    S2 = np.stack([np.zeros(n), S[0]])
    rows = np.asarray([[4321, 7], [order[0, n // 2], order[0, 2]]], np.int64)
    mask = _mask(n, "half")
    try:
        idx.cap, idx.RANGE_MAX_CAP = 1024, 2048
        got, stats = _rank(idx, Q2, rows)
        gotm, statsm = _rank(idx, Q2, rows, allowed=mask)
    finally:
        idx.cap, idx.RANGE_MAX_CAP = 4096, 131072
    np.testing.assert_array_equal(got, _oracle_ranks(S2, rows))
    np.testing.assert_array_equal(gotm, _oracle_ranks(S2, rows, mask))
    assert stats["rank_fallback_pairs"] == 2 and statsm["rank_fallback_pairs"] == 2, (stats, statsm)


def test_empty_index_and_stale_filter(torch_cuda):
    from convdr_amd.search import FlatIPIndex
    P, Q = synth_corpus(3, 600, 64), synth_corpus(4, 2, 64)
    idx = FlatIPIndex(64, prepin=False)
    assert idx.rank_rows(Q, np.asarray([-1, -1])).tolist() == [-1, -1]
    assert (idx.score_rows(Q, np.asarray([-1, -1])) == PAD).all()
    with pytest.raises(ValueError):
        idx.rank_rows(Q, np.asarray([0, -1]))
    idx.add(P[:500])
    f = idx.row_filter(np.ones(500, bool))
    assert idx.rank_rows(Q, np.asarray([3, 4]), allowed=f).shape == (2,)
    idx.add(P[500:])
    with pytest.raises(ValueError):
        idx.rank_rows(Q, np.asarray([3, 4]), allowed=f)
    with pytest.raises(ValueError):
        idx.rank_rows(Q, np.asarray([3, 600]))


@pytest.mark.parametrize("storage,precision", CONFIGS)
def test_c_entry_directly(torch_cuda, storage, precision):
    """convdr_ip_rank_rows through ctypes at cap = 1,024: refused with a workspace one byte short and with a NULL output, each
    with its reason; then one call over a poisoned workspace: OK pairs carry the oracle's rank and score, a target outside the
    block rank -1 with status OK, and the pair whose band overflows (the zero query) reports the exact band count n."""
    torch = torch_cuda
    from convdr_amd import _lib
    shape = (5000, 37, 768, False)
    n, nq, d, _ = shape
    _, Q = _corpus(shape)
    S, order = _scores(shape), _order(shape)
    idx = _index(shape, storage, precision)
    L, ptr = _lib.lib(), _lib.ptr
    store = 2 if idx.storage == "fp16" else (1 if idx.kind == "f16" else 0)
    cap = 1024
    Qp = np.concatenate([Q[:5], np.zeros((1, d), np.float32)])
    tgt = np.asarray([order[0, 0], order[1, 7], order[2, n - 1], -1, n, 99], np.int64)
    npairs = len(tgt)
    need = L.convdr_ip_rank_workspace_bytes(npairs, n, d, cap)
    assert need > 0
    q, t = torch.from_numpy(Qp).cuda(), torch.from_numpy(tgt).cuda()
    ws = fill_bytes(torch.empty(need, dtype=torch.uint8, device="cuda"), "R", 5)
    rank = fill_bytes(torch.empty(npairs, dtype=torch.int64, device="cuda"), "R", 6)
    X = fill_bytes(torch.empty(npairs, dtype=torch.float64, device="cuda"), "R", 7)
    cnt = fill_bytes(torch.empty(npairs, dtype=torch.int64, device="cuda"), "R", 8)
    above = fill_bytes(torch.empty(npairs, dtype=torch.int64, device="cuda"), "R", 9)
    st = fill_bytes(torch.empty(npairs, dtype=torch.int32, device="cuda"), "R", 10)

    def call(ws_bytes=need, outs=None):
        o = [rank, X, cnt, above, st] if outs is None else outs
        return L.convdr_ip_rank_rows(store, ptr(q), npairs, ptr(t), None if idx.storage == "fp16" else ptr(idx._rows), ptr(idx._pbf),
                                     float(idx._scale) if store else 1.0, None if idx.storage == "fp16" else ptr(idx._centre), n, d,
                                     ptr(idx._max_norm), None, 0, 0, cap, ptr(ws), ws_bytes, *[ptr(x) for x in o], _lib.stream_ptr())
    assert call(ws_bytes=need - 1) < 0 and b"workspace too small" in L.convdr_last_error()
    for i in range(5):
        outs = [rank, X, cnt, above, st]
        outs[i] = None
        assert call(outs=outs) < 0 and b"NULL argument" in L.convdr_last_error(), i
    assert call() == 0, L.convdr_last_error()
    torch.cuda.synchronize()
    rank, X, cnt, above, st = (x.cpu().numpy() for x in (rank, X, cnt, above, st))
    assert st.tolist() == [0, 0, 0, 0, 0, 1]
    assert rank.tolist() == [0, 7, n - 1, -1, -1, -1]
    assert cnt[5] == n and above[5] == 0 and cnt[3] == cnt[4] == 0 and above[3] == above[4] == 0
    np.testing.assert_array_equal(X[:3].view(np.uint64), S[[0, 1, 2], tgt[:3]].view(np.uint64))
    assert X[3] == X[4] == np.float64(PAD) and X[5] == 0.0
    assert (above[:3] + cnt[:3] >= rank[:3] + 1).all() and (above[:3] <= rank[:3]).all() and (cnt[:3] >= 1).all()
