"""FlatIPIndex(storage="fp16"): the passage is stored once, in 16 bits; the corpus is DEFINED as those halves and the result is
the exact top-k of the halves widened to fp32 -- `oracle.search.flat_ip_search(Q, P16.astype(np.float32), k)`, bit for bit.
Every comparison below is assert_array_equal on D and I: there are no tolerances."""
import numpy as np
import pytest

from oracle import search as OS
from tests import deep_cases, helpers
from tests.golden.make_golden import synth_corpus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _index(d=768, **kw):
    from convdr_amd.search import FlatIPIndex
    return FlatIPIndex(d, storage="fp16", **kw)


def _oracle(Q, P16, k):
    assert P16.dtype == np.float16
    return OS.flat_ip_search(Q, P16.astype(np.float32), k)


def _assert_exact(idx, Q, k, Dr, Ir, what=""):
    D, I = idx.search(Q, k)
    np.testing.assert_array_equal(I, Ir, err_msg=what)
    np.testing.assert_array_equal(D, Dr, err_msg=what)
    assert D.dtype == np.float32 and I.dtype == np.int64
    return D, I


_CASES = {}


def _case(n, nq, k, d):
    """(P fp32, P16 = P rounded to half, Q, Dr, Ir) of one shape, computed once and shared; never written to afterwards."""
    key = (n, nq, k, d)
    if key not in _CASES:
        P, Q = synth_corpus(100 + n % 97, n, d), synth_corpus(7, nq, d)
        P16 = P.astype(np.float16)
        out = (P, P16, Q) + tuple(_oracle(Q, P16, k))
        for a in out:
            a.setflags(write=False)
        _CASES[key] = out
    return _CASES[key]


def _store_bytes(idx):
    return idx.store.cpu().numpy()


SHAPES = [
    (700, 16, 100, 768),      # n <= cap: every passage is a candidate
    (5000, 37, 100, 768),     # full-score threshold pass
    (5000, 5, 10, 64),        # small d (one k-step), small k
    (40000, 24, 100, 768),    # sampled threshold pass, ragged last tile
    (33000, 130, 7, 128),     # two query tiles, ragged both ways
    (5000, 4, 100, 72),       # a padded width (zero columns inside the index)
]


@pytest.mark.parametrize("source", ["float16", "float32"])
@pytest.mark.parametrize("n,nq,k,d", SHAPES)
def test_search_matches_the_oracle_on_the_stored_halves(torch_cuda, n, nq, k, d, source):
    """float16 rows are kept bit for bit; fp32 rows are rounded to nearest even once, on the device, and the result is the
    oracle's on P.astype(float16)."""
    P, P16, Q, Dr, Ir = _case(n, nq, k, d)
    idx = _index(d)
    idx.add(P16 if source == "float16" else P)
    _assert_exact(idx, Q, k, Dr, Ir)
    if d % 64 == 0:
        want = (P16.astype(np.float32) * np.float32(idx._scale)).astype(np.float16)
        np.testing.assert_array_equal(_store_bytes(idx).view(np.uint16), want.view(np.uint16))


@pytest.mark.parametrize("precision", ["auto", "fp16", "fp16x2"])
@pytest.mark.parametrize("n,nq,k,d", [(700, 16, 100, 768), (40000, 24, 100, 768), (33000, 130, 7, 128)])
def test_every_rung_returns_the_same_exact_result(torch_cuda, precision, n, nq, k, d):
    P, P16, Q, Dr, Ir = _case(n, nq, k, d)
    idx = _index(d, precision=precision)
    idx.add(P16)
    _assert_exact(idx, Q, k, Dr, Ir)
    assert idx.stats["x2_queries"] == (nq if precision == "fp16x2" else 0) and idx.stats["x3_queries"] == 0, idx.stats


def test_one_launch_finish_equals_the_three_launch_chain(torch_cuda):
    from convdr_amd import _lib
    n, nq, k, d = 40000, 140, 100, 768
    P, P16, Q, Dr, Ir = _case(n, nq, k, d)
    L = _lib.lib()
    try:
        for fused in (0, 1):
            assert L.convdr_set_option(b"ip_fused_finish", fused) == 0
            for precision in ("fp16", "fp16x2"):
                idx = _index(d, precision=precision)
                idx.add(P16)
                _assert_exact(idx, Q, k, Dr, Ir, "fused=%d %s" % (fused, precision))
    finally:
        L.convdr_set_option(b"ip_fused_finish", 1)


@pytest.mark.parametrize("factor", [2.0 ** -10, 8.0, 2.0 ** -15])
def test_subnormal_halves_and_scale(torch_cuda, factor):
    """P16 * 2^-10: the elements below 2^-14 (|x| < 1/16 of N(0, 1): one in twenty) are subnormal halves; at 2^-15 most are.
    Scaling up by the store's 2^s is exact for them too.  P16 * 8: a block whose scale is smaller."""
    P, Q = synth_corpus(71, 20000, 768), synth_corpus(72, 12, 768)
    P16 = (P.astype(np.float16).astype(np.float32) * np.float32(factor)).astype(np.float16)
    sub = ((np.abs(P16.astype(np.float32)) < 2.0 ** -14) & (P16 != 0)).mean()
    assert sub > {2.0 ** -10: 0.04, 8.0: -1.0, 2.0 ** -15: 0.5}[factor], sub
    Dr, Ir = _oracle(Q, P16, 100)
    for precision in ("auto", "fp16"):
        idx = _index(768, precision=precision)
        idx.add(P16)
        assert idx._scale >= 1.0
        _assert_exact(idx, Q, 100, Dr, Ir)
        assert idx.stats["retried"] <= 1 and not idx.stats.get("exhaustive_queries"), idx.stats
        want = (P16.astype(np.float32) * np.float32(idx._scale)).astype(np.float16)
        np.testing.assert_array_equal(_store_bytes(idx).view(np.uint16), want.view(np.uint16))


def test_later_rows_outgrow_the_scale(torch_cuda):
    """20,000 rows fix the scale; 200 rows sixteen times longer put scale * max norm above 60,000: the search reports
    CONVDR_IP_RANGE, the store is rescaled IN PLACE by an exact power of two, and the result is exact."""
    P0 = synth_corpus(81, 20000, 768).astype(np.float16)
    P1 = (synth_corpus(82, 200, 768) * np.float32(16.0)).astype(np.float16)
    Q = synth_corpus(83, 9, 768)
    P16 = np.concatenate([P0, P1])
    Dr, Ir = _oracle(Q, P16, 20)
    idx = _index(768)
    idx.add(P0)
    s0, ptr = idx._scale, None
    idx.add(P1)
    assert idx._scale == s0
    ptr = idx._s16.data_ptr()
    _assert_exact(idx, Q, 20, Dr, Ir)
    assert idx.stats["rescaled"] == 1 and 1.0 <= idx._scale < s0 and idx._s16.data_ptr() == ptr, (idx.stats, idx._scale, s0)
    want = (P16.astype(np.float32) * np.float32(idx._scale)).astype(np.float16)
    np.testing.assert_array_equal(_store_bytes(idx).view(np.uint16), want.view(np.uint16))
    _assert_exact(idx, Q, 20, Dr, Ir)
    assert idx.stats["rescaled"] == 0


def test_refusals_leave_the_index_as_it_was(torch_cuda):
    from convdr_amd._lib import ConvdrError
    P, P16, Q, Dr, Ir = _case(5000, 37, 100, 768)
    idx = _index(768)
    idx.add(P16)
    before = (idx.ntotal, idx._scale, float(idx._max_norm.item()), _store_bytes(idx).copy())
    bad32 = synth_corpus(5, 300, 768)
    bad32[123, 45] = 1e5                                     # finite in fp32, inf once rounded to half
    long16 = np.full((10, 768), 2200.0, np.float16)          # every value finite, norm 2200 * sqrt(768) = 60,968
    nan16 = synth_corpus(6, 50, 768).astype(np.float16)
    nan16[7, 7] = np.nan
    for bad in (bad32, torch_cuda.from_numpy(bad32).cuda(), long16, nan16):
        with pytest.raises(ConvdrError):
            idx.add(bad)
        assert (idx.ntotal, idx._scale, float(idx._max_norm.item())) == before[:3]
        np.testing.assert_array_equal(_store_bytes(idx).view(np.uint16), before[3].view(np.uint16))
    _assert_exact(idx, Q, 100, Dr, Ir)
    more = synth_corpus(9, 800, 768).astype(np.float16)      # and it still takes rows
    idx.add(more)
    _assert_exact(idx, Q, 100, *_oracle(Q, np.concatenate([P16, more]), 100))
    empty = _index(768)
    with pytest.raises(ConvdrError):
        empty.add(long16)
    assert empty.ntotal == 0 and empty._scale == 1.0 and float(empty._max_norm.item()) == 0.0


def test_tie_group_straddles_k(torch_cuda):
    base = synth_corpus(33, 6000, 768).astype(np.float16)
    for n in (1500, 6000):
        P16 = base[:n].copy()
        P16[100:160] = P16[100]                              # 60 identical rows
        w = P16.astype(np.float32)
        Q = np.stack([w[100] * 3.0, w[100] * 3.0 + w[7] * 0.01, w[5]]).astype(np.float32)
        idx = _index()
        idx.add(P16)
        for k in (10, 37, 100):
            D, I = _assert_exact(idx, Q, k, *_oracle(Q, P16, k))
        assert I[0, :60].tolist() == list(range(100, 160))


def _clustered(amplitude, n=30000, nq=12, d=768):
    rs = np.random.RandomState(0)
    c = rs.randn(d).astype(np.float32)
    P = (0.9 * c[None, :] + amplitude * rs.randn(n, d)).astype(np.float32)
    Q = (0.9 * c[None, :] + amplitude * rs.randn(nq, d)).astype(np.float32)
    return P.astype(np.float16), Q


def test_a_block_the_single_pass_cannot_certify_takes_the_two_pass_rung(torch_cuda):
    """The construction of test_clustered_embeddings_are_searched_exactly with noise amplitude 0.02 (the store is not
    centred).  Derivation of the amplitude, not a measurement: |q| |p| ~ 0.81 * 768 = 622; for one query the scores of the
    30,000 rows spread with sigma ~ 0.9 |c| * 0.02 = 0.5.  Single pass: 2 eps = 2 * 1.07e-3 * 622 = 1.33 = 2.7 sigma below
    the 50th score (at +2.9 sigma): ~40 % of the block, more than the 8,192-entry list.  Two passes: 2 eps = 2 * 2.8e-4 *
    622 = 0.35 = 0.7 sigma: a few hundred rows."""
    k = 50
    P16, Q = _clustered(0.02)
    Dr, Ir = _oracle(Q, P16, k)
    idx = _index(768)
    idx.add(P16)
    _assert_exact(idx, Q, k, Dr, Ir)
    assert idx.stats["x2_queries"] > 0 and not idx.stats.get("exhaustive_queries"), idx.stats
    _assert_exact(idx, Q, k, Dr, Ir)                         # (the index remembers: x3_first)
    pinned = _index(768, precision="fp16x2")
    pinned.add(P16)
    _assert_exact(pinned, Q, k, Dr, Ir)
    assert not pinned.stats.get("exhaustive_queries"), pinned.stats


def test_norms_spread_over_orders_of_magnitude_end_on_the_exhaustive_rung(torch_cuda):
    """The construction of test_norms_spread_over_orders_of_magnitude_fall_through_to_the_exhaustive_rung, times 2^-6 so
    that the longest row (norm ~ 27.7 e^8 / 64) stays inside the half store's range."""
    rs = np.random.RandomState(359)
    n, d, nq, k = 33000, 768, 40, 333
    P = rs.randn(n, d).astype(np.float32) * np.exp(rs.randn(n, 1) * 2).astype(np.float32) * np.float32(2.0 ** -6)
    Q = rs.randn(nq, d).astype(np.float32)
    P16 = P.astype(np.float16)
    assert np.isfinite(P16.astype(np.float32)).all() and np.linalg.norm(P16.astype(np.float64), axis=1).max() < 50000
    idx = _index(d)
    idx.add(P16[:17812]); idx.add(P16[17812:])
    D, I = idx.search(Q, k)
    assert idx.stats.get("exhaustive_queries", 0) > 0, idx.stats
    Dr, Ir = _oracle(Q, P16, k)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)


@pytest.mark.parametrize("which", ["n > cap", "n <= cap"])
def test_deep_lists(torch_cuda, which):
    if which == "n > cap":
        n, nq, k, d = 20000, 3, 4097, 64                     # just above the 16,384-entry list: threshold + emit
        P16, Q = synth_corpus(300 + n % 83, n, d).astype(np.float16), synth_corpus(9, nq, d)
        P16[n - 50:n - 10] = P16[10:50]                      # exact duplicates far apart: index order decides
    else:
        Q, blocks_ = deep_cases.corpus()                     # 4,500 rows at row depth 4,400: every row a candidate
        P16, k, nq = blocks_[0][0].astype(np.float16), deep_cases.M, deep_cases.NQ
        d = deep_cases.DIM
    Dr, Ir = _oracle(Q, P16, k)
    for precision in ("auto", "fp16x2"):
        idx = _index(d, precision=precision)
        idx.add(P16)
        _assert_exact(idx, Q, k, Dr, Ir, precision)
        assert idx.stats["large_k"] == k and idx.stats["deep"] == nq and idx.stats["chunked_queries"] == 0, idx.stats


def test_streamed_adds(torch_cuda, tmp_path):
    torch = torch_cuda
    from convdr_amd import blocks
    P16 = synth_corpus(51, 9000, 768).astype(np.float16)
    Q = synth_corpus(53, 23, 768)
    ref = _index()
    ref.add(torch.from_numpy(P16).cuda())
    Dr, Ir = ref.search(Q, 100)
    np.testing.assert_array_equal(Ir, _oracle(Q, P16, 100)[1])
    want = _store_bytes(ref).view(np.uint16)
    path = str(tmp_path / "passage__emb_p__data_obj_0.pb")
    blocks.dump_block(path, P16)
    for how in ("array", "view"):
        idx = _index()
        idx.host_chunk_bytes = 1 << 20                       # 682 half rows per chunk: 13 chunks and a ragged tail
        if how == "array":
            idx.add(P16)
        else:
            with blocks.BlockView(path) as view:
                assert view.array.dtype == np.float16 and not view.array.flags.writeable
                idx.add(view)
        assert idx.stats["add_host_bytes"] == P16.nbytes      # (the streamed path ran)
        assert idx._scale == ref._scale
        np.testing.assert_array_equal(_store_bytes(idx).view(np.uint16), want, err_msg=how)
        _assert_exact(idx, Q, 100, Dr, Ir, how)
    # two streamed adds back to back keep their rows (the staging buffers are shared)
    A, B = P16[:5215], P16[5215:]
    for rep in range(5):
        idx = _index()
        idx.host_chunk_bytes = 1 << 20
        idx.add(A)
        idx.add(B)
        np.testing.assert_array_equal(_store_bytes(idx).view(np.uint16), want, err_msg="rep %d" % rep)


def test_driver_and_distinct(torch_cuda, tmp_path):
    torch = torch_cuda
    from convdr_amd import blocks
    from convdr_amd import search as S
    P0, P1 = synth_corpus(61, 3000, 768).astype(np.float16), synth_corpus(62, 2500, 768).astype(np.float16)
    P1[40:60] = P0[100:120]                                  # duplicates across the blocks
    Q = synth_corpus(63, 11, 768)
    ids = [np.arange(3000, dtype=np.int64), np.arange(2500, dtype=np.int64) + 10 ** 6]
    for r, (P, i) in enumerate(zip((P0, P1), ids)):
        blocks.dump_block(str(tmp_path / ("passage__emb_p__data_obj_%d.pb" % r)), P)
        blocks.dump_block(str(tmp_path / ("passage__embid_p__data_obj_%d.pb" % r)), i)
    idx = _index()
    idx.host_chunk_bytes = 1 << 20
    mD, mI = S.search_one_by_one(str(tmp_path), idx, Q, 100)
    oD, oI = OS.search_one_by_one([(P0.astype(np.float32), ids[0]), (P1.astype(np.float32), ids[1])], Q, 100)
    np.testing.assert_array_equal(mI, oI)
    np.testing.assert_array_equal(mD, oD)
    assert idx.twin().storage == "fp16"
    # document-level: every key owns 1..4 rows
    rs = np.random.RandomState(4)
    keys = np.repeat(np.arange(3000), rs.randint(1, 5, size=3000))[:3000][rs.permutation(3000)].astype(np.int64)
    one = _index()
    one.add(P0)
    D, I, K, counts = one.search_distinct(Q, 50, torch.from_numpy(keys).cuda())
    Dall, Iall = _oracle(Q, P0, 3000)
    Dd, Id, Kd, cd = S.distinct_topk(Dall, Iall, 50, keys)
    np.testing.assert_array_equal(I.cpu().numpy(), Id)
    np.testing.assert_array_equal(K.cpu().numpy(), Kd)
    np.testing.assert_array_equal(D.cpu().numpy(), Dd)


def test_the_index_holds_one_copy(torch_cuda):
    torch = torch_cuda
    n, d = 5000, 72
    P, P16, Q, Dr, Ir = _case(n, 4, 100, d)
    for precision in ("auto", "fp16x2"):
        idx = _index(d, precision=precision)
        idx.add(P)
        idx.search(Q, 100)
        assert idx.store.dtype == torch.float16 and idx.store.numel() * 2 == n * 128 * 2
        assert idx._s32 is None and idx._slo is None and idx._centre is None and idx._p32 is None and idx._plo is None
        big = [(name, t.dtype) for name, t in vars(idx).items()
               if isinstance(t, torch.Tensor) and t.is_cuda and t.numel() >= n and name not in ("_s16", "_ws")]
        assert not big, big


def test_stale_workspace_and_outputs(torch_cuda):
    torch = torch_cuda
    n, nq, k, d = 40000, 24, 100, 768
    P, P16, Q, Dr, Ir = _case(n, nq, k, d)
    idx = _index(d)
    idx.add(P16)
    q = torch.from_numpy(Q).cuda()
    idx.search_device(q, k)
    ptr = idx._ws.data_ptr()
    runs = {}
    for i, f in enumerate(helpers.FILLS):
        helpers.fill_bytes(idx._ws, f, seed=41 + i)
        # the outputs are torch.empty inside the call: the allocator hands back these blocks
        stale = [helpers.fill_bytes(torch.empty((nq, k), dtype=dt, device="cuda"), f, seed=51 + i)
                 for dt in (torch.float32, torch.int64)]
        del stale
        for x3 in (False, True):
            D, I, st, tr = idx.search_device(q, k, x3=x3)
            runs[f + str(int(x3))] = {"D": D.clone(), "I": I.clone(), "status": st.clone(), "tau_retry": tr.clone().view(torch.int32)}
        assert idx._ws.data_ptr() == ptr
    for x3 in "01":
        z = runs["Z" + x3]
        for f in helpers.FILLS[1:]:
            for name, t in runs[f + x3].items():
                assert torch.equal(t, z[name]), (f, x3, name)
        ok = (z["status"] == 0).cpu().numpy()
        assert ok.any()
        np.testing.assert_array_equal(z["I"].cpu().numpy()[ok], Ir[ok])
        np.testing.assert_array_equal(z["D"].cpu().numpy()[ok], Dr[ok])
    for f in helpers.FILLS:
        helpers.fill_bytes(idx._ws, f, seed=5)
        _assert_exact(idx, Q, k, Dr, Ir, f)


def test_update_rows_rounds_and_scales(torch_cuda):
    torch = torch_cuda
    P, P16, Q, Dr, Ir = _case(5000, 37, 100, 768)
    new = synth_corpus(12, 300, 768) * np.float32(1.5)
    idx = _index(768)
    idx.add(P16)
    idx.update_rows(1000, torch.from_numpy(new).cuda())
    now = P16.copy()
    now[1000:1300] = new.astype(np.float16)
    _assert_exact(idx, Q, 100, *_oracle(Q, now, 100))
    assert idx.update_flags() == 0
