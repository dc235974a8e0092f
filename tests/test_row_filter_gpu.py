"""Row-filtered exact top-k: FlatIPIndex.search(..., allowed=) / convdr_ip_search_filtered.

Expected value everywhere, no tolerances: with rows = np.flatnonzero(mask), oracle.search.flat_ip_search(Q, P[rows], k) with I
mapped back through rows and FAISS padding where len(rows) < k (rows is ascending: the oracle's lower-index-first tie rule
carries over).  Both stores hold the SAME corpus -- synth_corpus rounded to half and widened: the half store keeps those
halves, the fp32 store is given them as fp32 (its centred scan copies still round) -- so one oracle run per (shape, mask)
serves every store and precision.  Every comparison is assert_array_equal on D and I."""
import numpy as np
import pytest

from oracle import search as OS
from tests.golden.make_golden import synth_corpus
from tests.helpers import fill_bytes
from tests.index_cases import mask as _recipe, torch_cuda      # noqa: F401 (torch_cuda: the fixture, by name)

pytestmark = pytest.mark.gpu

PAD_D, PAD_I = np.float32(-3.4028234663852886e38), -1


# n, nq, k, d: the smallest shapes that reach each plan
SHAPES = [
    (300, 3, 10, 64),         # n <= cap, ragged last tile, ragged last word, one K step
    (5000, 37, 100, 768),     # FULL sample
    (40000, 24, 100, 768),    # TOP2 sample, strided tiles
    (33000, 130, 7, 128),     # two query tiles: Tile256 and the r3 emit path
    (20000, 4, 5000, 64),     # deep, n > cap: segment samples
    (9000, 4, 5000, 64),      # deep, n <= cap
]
# storage, precision
CONFIGS = [("fp32", "auto"), ("fp32", "bf16"), ("fp32", "fp16x3"), ("fp16", "auto"), ("fp16", "fp16x2")]
MASKS = ["all", "no_topk", "half", "one", "last_tile", "word_edges", "none"]

_CORPUS, _ORACLE, _INDEX = {}, {}, {}


def _corpus(shape):
    """(P = halves widened to fp32, Q) of a shape; computed once, never written to afterwards"""
    if shape not in _CORPUS:
        n, nq, k, d = shape
        P = synth_corpus(100 + n % 97, n, d).astype(np.float16).astype(np.float32)
        Q = synth_corpus(7, nq, d)
        P.setflags(write=False), Q.setflags(write=False)
        _CORPUS[shape] = (P, Q)
    return _CORPUS[shape]


def _filtered_oracle(Q, P, k, mask):
    rows = np.flatnonzero(mask)
    D = np.full((Q.shape[0], k), PAD_D, np.float32)
    I = np.full((Q.shape[0], k), PAD_I, np.int64)
    if len(rows):
        Dr, Ir = OS.flat_ip_search(Q, np.ascontiguousarray(P[rows]), k)
        m = min(k, len(rows))
        D[:, :m], I[:, :m] = Dr[:, :m], rows[Ir[:, :m]]
        assert (Ir[:, m:] == -1).all()
    return D, I


def _mask(shape, name):
    n, nq, k, d = shape
    if name not in ("all", "no_topk"):
        return _recipe(n, name)
    m = np.ones(n, bool)
    if name == "no_topk":                    # the whole unfiltered top-k of every query removed
        m[np.unique(_expected(shape, "all")[1])] = False
    return m


def _expected(shape, name):
    """(D, I) of the oracle over the rows mask `name` allows; computed once per (shape, mask)"""
    key = (shape, name)
    if key not in _ORACLE:
        P, Q = _corpus(shape)
        _ORACLE[key] = _filtered_oracle(Q, P, shape[2], _mask(shape, name))
    return _ORACLE[key]


def _index(shape, storage, precision):
    """one resident index per (shape, store, precision), shared by the masks"""
    from convdr_amd.search import FlatIPIndex
    key = (shape, storage, precision)
    if key not in _INDEX:
        _INDEX.clear()                       # (cases arrive grouped by index: one resident at a time)
        P, _ = _corpus(shape)
        idx = FlatIPIndex(shape[3], storage=storage, precision=precision, prepin=False)
        idx.add(P.astype(np.float16) if storage == "fp16" else P)
        _INDEX[key] = idx
    return _INDEX[key]


def _check(idx, Q, k, mask, Dr, Ir, what=""):
    D, I = idx.search(Q, k, allowed=mask)
    np.testing.assert_array_equal(I, Ir, err_msg=what)
    np.testing.assert_array_equal(D, Dr, err_msg=what)
    assert D.dtype == np.float32 and I.dtype == np.int64
    return D, I


@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("storage,precision", CONFIGS)
@pytest.mark.parametrize("n,nq,k,d", SHAPES)
def test_filtered_search_equals_the_oracle_over_the_allowed_rows(torch_cuda, n, nq, k, d, storage, precision, name):
    shape = (n, nq, k, d)
    _, Q = _corpus(shape)
    mask = _mask(shape, name)
    Dr, Ir = _expected(shape, name)
    idx = _index(shape, storage, precision)
    D, I = _check(idx, Q, k, mask, Dr, Ir, "%s %s %s" % (storage, precision, name))
    allowed = int(mask.sum())
    assert (I[:, min(k, allowed):] == -1).all() and (I[:, :min(k, allowed)] >= 0).all()
    if name == "all":                        # bit for bit the unfiltered search of the same index
        Du, Iu = idx.search(Q, k)
        np.testing.assert_array_equal(I, Iu)
        np.testing.assert_array_equal(D.view(np.uint32), Du.view(np.uint32))
    if name == "no_topk":
        Iu = _expected(shape, "all")[1]
        assert not np.intersect1d(I[I >= 0], Iu[Iu >= 0]).size
    if name == "none":
        assert (D == PAD_D).all()


@pytest.mark.parametrize("storage,precision", CONFIGS)
@pytest.mark.parametrize("n,nq,k,d", [(5000, 37, 100, 768), (40000, 24, 100, 768)])
def test_one_percent_filter_is_one_pass(torch_cuda, n, nq, k, d, storage, precision):
    """n_allowed <= cap: every allowed row is a candidate -- one pass, no threshold sample, nothing retried; at n = 5,000 the
    ~50 allowed rows are fewer than k = 100: the tail is padding."""
    shape = (n, nq, k, d)
    _, Q = _corpus(shape)
    mask = _mask(shape, "percent")
    allowed = int(mask.sum())
    assert 0 < allowed <= 4096 and (allowed < k) == (n == 5000)
    idx = _index(shape, storage, precision)
    D, I = _check(idx, Q, k, mask, *_expected(shape, "percent"))
    assert idx.stats["rounds"] == 1 and idx.stats["retried"] == 0, idx.stats
    assert (I[:, min(k, allowed):] == -1).all() and (D[:, min(k, allowed):] == PAD_D).all()


@pytest.mark.parametrize("storage,precision", CONFIGS)
def test_deep_segment_samples_see_the_filter(torch_cuda, storage, precision):
    """n = 20,000, k = 5,000, 90 % allowed: 18,000 allowed rows are more than the 16,384-entry list, so the threshold comes from
    the per-segment samples, each launched over a sub-block whose bitmap pointer advances with its rows."""
    shape = (20000, 4, 5000, 64)
    _, Q = _corpus(shape)
    mask = _mask(shape, "most")
    assert int(mask.sum()) > 16384
    idx = _index(shape, storage, precision)
    _check(idx, Q, 5000, mask, *_expected(shape, "most"))
    assert idx.stats["deep"] == 4 and idx.stats["chunked_queries"] == 0, idx.stats


def test_prebuilt_filter_device_masks_and_begin_finish(torch_cuda):
    """row_filter accepts numpy / torch, bool / uint8, host / device masks; a RowFilter is reused across searches and survives
    update_rows; search_begin / search_finish with a filter equals search."""
    torch = torch_cuda
    shape = (5000, 37, 100, 768)
    P, Q = _corpus(shape)
    mask = _mask(shape, "half")
    Dr, Ir = _expected(shape, "half")
    idx = _index(shape, "fp32", "auto")
    f = idx.row_filter(mask)
    assert f.n == 5000 and f.n_allowed == int(mask.sum()) and f.bits.numel() == (5000 + 255) // 256 * 8
    want = np.zeros((5000 + 255) // 256 * 256, bool)
    want[:5000] = mask
    np.testing.assert_array_equal(f.bits.cpu().numpy().view(np.uint32), np.packbits(want, bitorder="little").view(np.uint32))
    np.testing.assert_array_equal(f.rows().cpu().numpy(), np.flatnonzero(mask))
    for m in (f, mask.astype(np.uint8), torch.from_numpy(mask), torch.from_numpy(mask).cuda(), torch.from_numpy(mask.astype(np.uint8)).cuda()):
        _check(idx, Q, 100, m, Dr, Ir)
    D, I = idx.search_finish(idx.search_begin(Q, 100, allowed=f))
    np.testing.assert_array_equal(I.cpu().numpy(), Ir)
    np.testing.assert_array_equal(D.cpu().numpy(), Dr)
    Dd, Id, st, _ = idx.search_device(torch.from_numpy(Q).cuda(), 100, allowed=f)
    ok = (st == 0).cpu().numpy()
    assert ok.any()
    np.testing.assert_array_equal(Id.cpu().numpy()[ok], Ir[ok])
    idx.update_rows(17, torch.from_numpy(P[17:19].copy()).cuda())      # (the same rows: the filter stays valid, the result too)
    _check(idx, Q, 100, f, Dr, Ir)


def test_stale_filter_and_wrong_length_raise(torch_cuda):
    from convdr_amd.search import FlatIPIndex
    P, Q = synth_corpus(3, 600, 64), synth_corpus(4, 2, 64)
    idx = FlatIPIndex(64, prepin=False)
    idx.add(P[:500])
    f = idx.row_filter(np.ones(500, bool))
    idx.search(Q, 5, allowed=f)
    for bad in (np.ones(499, bool), np.ones(501, np.uint8), np.ones((500, 1), bool)):
        with pytest.raises(ValueError):
            idx.search(Q, 5, allowed=bad)
        with pytest.raises(ValueError):
            idx.row_filter(bad)
    idx.add(P[500:])
    for call in (lambda: idx.search(Q, 5, allowed=f), lambda: idx.search_begin(Q, 5, allowed=f),
                 lambda: idx.search_device(None, 5, allowed=f), lambda: idx.search_deep_device(None, 5000, allowed=f)):
        with pytest.raises(ValueError):
            call()
    idx.reset()
    with pytest.raises(ValueError):
        idx.search(Q, 5, allowed=f)


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_tie_group_straddles_k_with_members_masked(torch_cuda, storage):
    """60 identical rows; every third of them masked.  The allowed members keep the rule that the lower index comes first, and
    the group straddles rank k for k = 10 and 37."""
    from convdr_amd.search import FlatIPIndex
    for n in (1500, 6000):
        P = synth_corpus(33, n, 768).astype(np.float16).astype(np.float32)
        P[100:160] = P[100]
        Q = np.stack([P[100] * 3.0, P[100] * 3.0 + P[7] * 0.01, P[5]]).astype(np.float32)
        mask = np.random.RandomState(5).rand(n) < 0.7
        mask[100:160] = True
        mask[100:160:3] = False
        idx = FlatIPIndex(768, storage=storage, prepin=False)
        idx.add(P.astype(np.float16) if storage == "fp16" else P)
        f = idx.row_filter(mask)
        for k in (10, 37, 100):
            D, I = _check(idx, Q, k, f, *_filtered_oracle(Q, P, k, mask))
        group = [r for r in range(100, 160) if (r - 100) % 3]
        assert I[0, :40].tolist() == group


def test_clustered_block_takes_the_two_pass_rung_under_a_filter(torch_cuda):
    """The recipe of test_a_block_the_single_pass_cannot_certify_takes_the_two_pass_rung (half store, noise amplitude 0.02)
    at 60,000 rows with a 50 % mask: the 30,000 allowed rows are that test's block in distribution, so its derivation holds
    unchanged -- the single pass's band is ~40 % of the allowed rows, more than the largest list, the two-pass band a few
    hundred."""
    from convdr_amd.search import FlatIPIndex
    rs = np.random.RandomState(0)
    n, nq, d, k = 60000, 12, 768, 50
    c = rs.randn(d).astype(np.float32)
    P16 = (0.9 * c[None, :] + 0.02 * rs.randn(n, d)).astype(np.float32).astype(np.float16)
    Q = (0.9 * c[None, :] + 0.02 * rs.randn(nq, d)).astype(np.float32)
    mask = np.random.RandomState(1).rand(n) < 0.5
    idx = FlatIPIndex(d, storage="fp16", prepin=False)
    idx.add(P16)
    Dr, Ir = _filtered_oracle(Q, P16.astype(np.float32), k, mask)
    _check(idx, Q, k, mask, Dr, Ir)
    assert idx.stats["x2_queries"] > 0 and not idx.stats.get("exhaustive_queries"), idx.stats


def test_norms_spread_end_on_the_exhaustive_rung_under_a_filter(torch_cuda):
    """The recipe of test_norms_spread_over_orders_of_magnitude_fall_through_to_the_exhaustive_rung at 66,000 rows with a 50 %
    mask (33,000 allowed rows: that test's block in distribution).  The exhaustive rung walks the ascending list of allowed
    row ids in chunks."""
    from convdr_amd.search import FlatIPIndex
    rs = np.random.RandomState(359)
    n, d, nq, k = 66000, 768, 40, 333
    P = rs.randn(n, d).astype(np.float32) * np.exp(rs.randn(n, 1) * 2).astype(np.float32)
    Q = rs.randn(nq, d).astype(np.float32)
    mask = np.random.RandomState(2).rand(n) < 0.5
    idx = FlatIPIndex(d, prepin=False)
    idx.add(P)
    D, I = idx.search(Q, k, allowed=mask)
    assert idx.stats.get("exhaustive_queries", 0) > 0, idx.stats
    Dr, Ir = _filtered_oracle(Q, P, k, mask)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_k_beyond_the_deep_lists_takes_the_chunked_route(torch_cuda, storage):
    from convdr_amd.search import FlatIPIndex
    n, nq, k, d = 5000, 3, 65537, 64
    P = synth_corpus(41, n, d).astype(np.float16).astype(np.float32)
    P[4000:4040] = P[20:60]                     # duplicates far apart, some masked: index order decides among the allowed
    Q = synth_corpus(42, nq, d)
    mask = np.random.RandomState(3).rand(n) < 0.5
    idx = FlatIPIndex(d, storage=storage, prepin=False)
    idx.add(P.astype(np.float16) if storage == "fp16" else P)
    _check(idx, Q, k, mask, *_filtered_oracle(Q, P, k, mask))
    assert idx.stats["chunked_queries"] == nq and idx.stats["large_k"] == k, idx.stats


@pytest.mark.parametrize("storage,precision", [("fp32", "auto"), ("fp32", "bf16"), ("fp16", "auto"), ("fp16", "fp16x2")])
def test_both_settings_of_ip_fused_finish(torch_cuda, storage, precision):
    from convdr_amd import _lib
    shape = (5000, 37, 100, 768)
    _, Q = _corpus(shape)
    idx = _index(shape, storage, precision)
    L = _lib.lib()
    try:
        for fused in (0, 1):
            assert L.convdr_set_option(b"ip_fused_finish", fused) == 0
            for name in ("half", "percent", "none"):
                _check(idx, Q, 100, _mask(shape, name), *_expected(shape, name), what="fused=%d %s" % (fused, name))
    finally:
        L.convdr_set_option(b"ip_fused_finish", 1)


@pytest.mark.parametrize("n,nq,k,cap", [(5 * 256 + 37, 3, 10, 1024),            # shallow, n > cap: threshold pass; tall tile, ragged last tile
                                        (5 * 256 + 37, 129, 10, 1024),          # the 256 x 256 tile
                                        (0, 3, 10, 1024),
                                        (16384 + 256 + 37, 3, 4097, 16384),     # deep, n > cap: segment samples
                                        (0, 3, 4097, 16384)])
@pytest.mark.parametrize("storage,precision", [("fp32", "bf16"), ("fp32", "fp16"), ("fp16", "fp16")])
def test_all_ones_bitmap_is_the_direct_entry_bit_for_bit(torch_cuda, storage, precision, n, nq, k, cap):
    """The direct entry of the store and depth, then convdr_ip_search_filtered with every bit set and n_allowed = n, on the same
    operands and the same workspace size: one host pipeline serves both, so D, I and status agree bit for bit -- and tau_retry
    where a status asks for a retry.  (Every query of these shapes is certified on its first pass, so the tau_retry clause
    compares nothing today; it stands for shapes added later.)"""
    torch = torch_cuda
    from convdr_amd import _lib
    from convdr_amd.search import FlatIPIndex, RowFilter
    d = 64
    idx = FlatIPIndex(d, storage=storage, precision=precision, prepin=False)
    Q = synth_corpus(7, nq, d)
    q = torch.from_numpy(Q).cuda()
    if n:
        P = synth_corpus(100 + n % 97, n, d).astype(np.float16)
        idx.add(P if storage == "fp16" else P.astype(np.float32))
        f = idx.row_filter(np.ones(n, bool))
        p32, p16 = idx._rows, idx._pbf
    else:                                    # an empty block: the pointers are never dereferenced, the bitmap must still be one
        f = RowFilter(torch.full((8,), -1, dtype=torch.int32, device="cuda"), 0, 0)
        p32 = p16 = q
    assert f.n_allowed == n
    deep = k > idx.MAX_K
    L = _lib.lib()
    need = (L.convdr_ip_deep_workspace_bytes if deep else L.convdr_ip_workspace_bytes)(nq, n, d, k, cap)
    runs = []
    for allowed in (None, f):
        ws = fill_bytes(torch.empty(need, dtype=torch.uint8, device="cuda"), "R", 9)
        D = fill_bytes(torch.empty((nq, k), dtype=torch.float32, device="cuda"), "R", 10)
        I = fill_bytes(torch.empty((nq, k), dtype=torch.int64, device="cuda"), "R", 11)
        st = fill_bytes(torch.empty(nq, dtype=torch.int32, device="cuda"), "R", 12)
        tr = fill_bytes(torch.empty(nq, dtype=torch.float32, device="cuda"), "R", 13)
        idx._search_call(q, nq, p32, p16, None, n, k, None, cap, 0, ws, D, I, st, tr, False, deep, allowed)
        torch.cuda.synchronize()
        runs.append((D.cpu().numpy().view(np.uint32), I.cpu().numpy(), st.cpu().numpy(), tr.cpu().numpy().view(np.uint32)))
    (Da, Ia, sa, ta), (Db, Ib, sb, tb) = runs
    print("status direct", np.bincount(sa, minlength=5).tolist(), "filtered", np.bincount(sb, minlength=5).tolist())
    np.testing.assert_array_equal(sa, sb)
    np.testing.assert_array_equal(Ia, Ib)
    np.testing.assert_array_equal(Da, Db)
    np.testing.assert_array_equal(ta[sa != 0], tb[sa != 0])
    if n == 0:
        assert (sa == 0).all() and (Ia == -1).all()
    else:
        assert (Ia[sa == 0][:, :min(k, n)] >= 0).all()


@pytest.mark.parametrize("storage,n,nq,k,d", [("fp32", 5000, 37, 100, 768), ("fp16", 5000, 37, 100, 768),
                                              ("fp32", 40000, 24, 100, 768), ("fp16", 20000, 4, 5000, 64)])
def test_result_does_not_depend_on_stale_workspace_or_outputs(torch_cuda, storage, n, nq, k, d):
    """One enqueue of the filtered entry with the workspace and every output pre-filled with zeros, with 0xFF bytes (NaN as a
    float, -1 as an integer) and with random bytes: the outputs agree bit for bit, and every certified query is the oracle's."""
    torch = torch_cuda
    from convdr_amd import _lib
    shape = (n, nq, k, d)
    _, Q = _corpus(shape)
    idx = _index(shape, storage, "auto")
    which = "most" if k > 4096 else "half"          # (the deep case keeps more rows than its list holds: the sampled plan)
    f = idx.row_filter(_mask(shape, which))
    Dr, Ir = _expected(shape, which)
    q = torch.from_numpy(Q).cuda()
    deep = k > idx.MAX_K
    cap = idx._deep_cap(k) if deep else idx.cap
    L = _lib.lib()
    need = (L.convdr_ip_deep_workspace_bytes if deep else L.convdr_ip_workspace_bytes)(nq, n, d, k, cap)
    runs = {}
    for fill in ("Z", "N", "R"):
        ws = fill_bytes(torch.empty(need, dtype=torch.uint8, device="cuda"), fill, 9)
        D = fill_bytes(torch.empty((nq, k), dtype=torch.float32, device="cuda"), fill, 10)
        I = fill_bytes(torch.empty((nq, k), dtype=torch.int64, device="cuda"), fill, 11)
        st = fill_bytes(torch.empty(nq, dtype=torch.int32, device="cuda"), fill, 12)
        tr = fill_bytes(torch.empty(nq, dtype=torch.float32, device="cuda"), fill, 13)
        idx._search_call(q, nq, idx._rows, idx._pbf, None, n, k, None, cap, idx.rank_target, ws, D, I, st, tr, False, deep, f)
        torch.cuda.synchronize()
        runs[fill] = (D.cpu().numpy().view(np.uint32), I.cpu().numpy(), st.cpu().numpy(), tr.cpu().numpy().view(np.uint32))
    for fill in ("N", "R"):
        for a, b in zip(runs["Z"], runs[fill]):
            np.testing.assert_array_equal(a, b, err_msg="fill %s" % fill)
    D, I, st, _ = runs["Z"]
    ok = st == 0
    assert ok.any()
    np.testing.assert_array_equal(I[ok], Ir[ok])
    np.testing.assert_array_equal(D[ok], Dr[ok].view(np.uint32))
