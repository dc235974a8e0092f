"""The 8-bit store (FlatIPIndex(storage="sq8")) on the device, against the numpy model of tests/sq8_cases.py and the oracle.
  1. lane map        integer data whose stored codes are the rows themselves: the raw scan scores (convdr_ip_debug_list) ARE the
                     integer dot products, rounded once to fp32
  2. the inequality  |S~ - E| <= eps_doc for every pair, E in fp64 from the index's own centre, step and codes; the library's eps
                     (recovered from tau_retry, as tests/test_scan_error_gpu.py does) lies in [eps_doc, 1.003 eps_doc].  Prints
                     `SQ8ERR family d nq route n: max |S~ - E| / eps_doc`; profiles/sq8_scan_error.txt is that output.
  3. exactness       search == oracle.search.flat_ip_search over the reconstructed rows, bit for bit
  4. reconstruction  reconstruct_n == the model's v; score_rows reproduces D
  5. stale memory    workspace and outputs pre-filled with NaN: the same bits
  6. round trips     remove_rows, save / load / fingerprint, a flipped byte in the step section
  7. refused input   a NaN in an add leaves the index as it was"""
import numpy as np
import pytest

from oracle import search as OS
from tests import sq8_cases as M
from tests.index_cases import torch_cuda      # noqa: F401 (the fixture, by name)
from tests.sq8_cases import OK

pytestmark = pytest.mark.gpu
f32 = np.float32
_SHARED = {}


def _index(P, d=None, **kw):
    from convdr_amd.search import FlatIPIndex
    idx = FlatIPIndex(P.shape[1] if d is None else d, storage="sq8", prepin=False, **kw)
    idx.add(P)
    return idx


def _parts(idx):
    """(codes int8 [n, d], centre, step, max L1) as the index holds them"""
    return (idx._pbf.cpu().numpy(), idx._centre.cpu().numpy(), idx._step.cpu().numpy(), float(idx._max_norm.item()))


def _scan_scores(torch, idx, q, route, n, what):
    cap, k = (8192, n) if route == "list" else (1024, 10)
    nq = int(q.shape[0])
    _, _, st, tr, hits, band, ws = M.raw_call(torch, idx, q, k, None, cap, fused=0)
    if route == "list":
        assert (st == OK).all(), (what, st)
        ids, s = M.scan_list(torch, ws, nq, n, idx.d, k, cap)
        return M.scores_from_list(ids, s, band, n, what), cap
    T = M.scan_sample(torch, ws, nq, n, idx.d, k, cap)
    assert T is not None and T.shape[0] == (n + 255) // 256 * 256 and (T[n:] == -np.inf).all(), what
    return np.ascontiguousarray(T[:n].T), cap


@pytest.mark.parametrize("nq", [5, 130])
@pytest.mark.parametrize("d", [128, 256])
def test_lane_map_raw_scores_are_the_integer_dot_products(torch_cuda, d, nq):
    torch = torch_cuda
    Q, P, want_codes = M.lane_map_case(d, nq)
    idx = _index(P)
    codes, centre, step, l1 = _parts(idx)
    assert (centre == 0).all() and (step == 1).all() and (codes == want_codes).all()
    hi, lo, te = M.query_split(Q, step)
    assert (te == 0).all() and (128 * hi + lo == Q.astype(np.int64)).all() and np.abs(hi).max() > 0 and np.abs(lo).max() > 0
    S, _ = _scan_scores(torch, idx, torch.tensor(Q, device="cuda"), "list", P.shape[0], ("lane map", d, nq))
    want = M.int_scan(hi, lo, codes)[0]
    assert (S == want.astype(f32)).all(), np.argwhere(S != want.astype(f32))[:5]


def _inequality_case(torch, d, nq, route, n):
    held = 0
    for fam in M.FAMILIES:
        Q, P = M.family(fam, d, nq, n)
        idx = _index(P)
        codes, centre, step, l1 = _parts(idx)
        assert (step == M.step_of(P, centre)).all() and (codes == M.codes_of(P, centre, step)[0]).all()
        assert l1 == np.abs(codes.astype(np.int64)).sum(axis=1).max()
        if fam == "saturated":
            assert (np.abs(codes.astype(int)) == 127).all()
        hi, lo, te = M.query_split(Q, step)
        what = (fam, d, nq, route, n)
        S, cap = _scan_scores(torch, idx, torch.tensor(Q, device="cuda"), route, n, what)
        E = M.exact_scaled(Q, codes, centre, step, te)
        eps = M.eps_doc(Q, codes, centre, step, te, l1)
        ratio = np.abs(S.astype(np.float64) - E) / eps[:, None]
        print("SQ8ERR %-9s d=%-4d nq=%-3d %-6s n=%-4d max |S~ - E| / eps_doc = %.4f" % (fam, d, nq, route, n, ratio.max()))
        assert np.isfinite(S).all() and ratio.max() <= 1.0, (what, ratio.max())
        assert (S == M.int_scan(hi, lo, codes)[0].astype(f32)).all(), what          # stronger: the scan is the model's integers
        if route == "list":
            got = M.hold_band(torch, idx, torch.tensor(Q, device="cuda"), S, E, eps, cap, what)
            held += got
            assert fam != "random" or got >= nq // 2, (what, "queries whose band was held", got)
    assert route != "list" or held > 0


@pytest.mark.parametrize("nq", [5, 130])
@pytest.mark.parametrize("d", [128, 768, 1024])
def test_list_route_scores_are_inside_the_band(torch_cuda, d, nq):
    for n in (1024, 1000):
        _inequality_case(torch_cuda, d, nq, "list", n)


@pytest.mark.parametrize("nq", [5, 130])
def test_sample_route_scores_are_inside_the_band(torch_cuda, nq):
    _inequality_case(torch_cuda, 768, nq, "sample", 1280)


def _corpus():
    """one random index of 20,000 x 768 rows, its reconstructed rows and the oracle's top 5,000; never written to afterwards"""
    if "corpus" not in _SHARED:
        rs = np.random.RandomState(5)
        spread = np.exp(rs.uniform(-0.55, 0.55, 768)).astype(f32)
        P = (rs.randn(20000, 768) * spread + rs.randn(768) * 0.5).astype(f32)
        Q = rs.randn(7, 768).astype(f32)
        idx = _index(P)
        V = idx.reconstruct_n(0, idx.ntotal)
        _SHARED["corpus"] = (idx, P, Q, V, OS.flat_ip_search(Q, V, 5000))
    return _SHARED["corpus"]


@pytest.mark.parametrize("k", [1, 100, 4096, 5000])
def test_search_is_the_oracle_over_the_reconstructed_rows(torch_cuda, k):
    idx, P, Q, V, (Dr, Ir) = _corpus()
    D, I = idx.search(Q, k)
    assert np.array_equal(I, Ir[:, :k]) and np.array_equal(D, Dr[:, :k])
    if k == 100:
        assert idx.stats["sq8_first_pass"] == len(Q), idx.stats       # every query certified on the first integer pass
        assert idx.stats["sq8_saturated"] == 0
    if k == 5000:
        assert idx.stats["deep"] == len(Q), idx.stats


def test_reconstruction_is_the_model_and_score_rows_reproduces_d(torch_cuda):
    idx, P, Q, V, (Dr, Ir) = _corpus()
    codes, centre, step, l1 = _parts(idx)
    assert (step == M.step_of(P, centre)).all() and (codes == M.codes_of(P, centre, step)[0]).all() and codes.min() >= -127
    assert np.array_equal(V.view(np.int32), M.reconstruct(codes, centre, step).view(np.int32))
    rows = np.array([0, 19999, 7, 7], dtype=np.int64)
    assert np.array_equal(idx.reconstruct_batch(rows), V[rows]) and np.array_equal(idx.reconstruct(19999), V[19999])
    assert np.array_equal(idx.rows_tensors(rows.reshape(2, 2)).cpu().numpy(), V[rows].reshape(2, 2, -1))
    D, I = idx.search(Q, 100)
    assert np.array_equal(idx.score_rows(Q, I).view(np.int32), D.view(np.int32))


@pytest.mark.parametrize("share", [0.01, 0.5])
def test_row_filter_is_the_oracle_over_the_allowed_rows(torch_cuda, share):
    idx, P, Q, V, _ = _corpus()
    mask = np.random.RandomState(int(share * 100)).rand(idx.ntotal) < share
    rows = np.flatnonzero(mask)
    k = 100
    Dr, Ir = OS.flat_ip_search(Q, V[rows], k)
    D, I = idx.search(Q, k, allowed=mask)
    assert np.array_equal(I, np.where(Ir >= 0, rows[np.clip(Ir, 0, None)], -1)) and np.array_equal(D, Dr)
    f = idx.row_filter(mask)
    Dt, It, st, _ = idx.search_device(torch_cuda.tensor(Q, device="cuda"), k, allowed=f)
    assert (st.cpu().numpy() == OK).all() and np.array_equal(It.cpu().numpy(), I)
    q = torch_cuda.tensor(Q, device="cuda")
    Dt, It = idx.search_tensors(q, k, allowed=f)
    Db, Ib = idx.search_finish(idx.search_begin(Q, k, allowed=f))
    for Dx, Ix in ((Dt, It), (Db, Ib)):
        assert np.array_equal(Ix.cpu().numpy(), I) and np.array_equal(Dx.cpu().numpy(), D)


def test_deep_route_with_a_row_filter_is_the_oracle(torch_cuda):
    """k = 5,000 over half of the rows: convdr_ip_search_filtered_q8 with deep = 1 (the sampling segments' bitmap offsets), through
    search and through one raw search_deep_device call"""
    idx, P, Q, V, _ = _corpus()
    mask = np.random.RandomState(50).rand(idx.ntotal) < 0.5
    rows = np.flatnonzero(mask)
    k = 5000
    Dr, Ir = OS.flat_ip_search(Q, V[rows], k)
    want = np.where(Ir >= 0, rows[np.clip(Ir, 0, None)], -1)
    f = idx.row_filter(mask)
    D, I = idx.search(Q, k, allowed=f)
    assert np.array_equal(I, want) and np.array_equal(D, Dr) and idx.stats["deep"] == len(Q), idx.stats
    Dd, Id, st, _ = idx.search_deep_device(torch_cuda.tensor(Q, device="cuda"), k, allowed=f)
    ok = st.cpu().numpy() == OK
    assert ok.any() and np.array_equal(Id.cpu().numpy()[ok], want[ok]) and np.array_equal(Dd.cpu().numpy()[ok], Dr[ok])


def test_duplicates_small_blocks_and_padded_width(torch_cuda):
    rs = np.random.RandomState(11)
    P = rs.randn(3000, 200).astype(f32)                      # d_in = 200 -> d = 256
    P[100], P[2500], P[17] = P[40], P[40], P[40]             # equal rows -> equal codes -> equal scores: the lower row first
    Q = np.concatenate([rs.randn(4, 200).astype(f32), P[40:41] * f32(2)])
    idx = _index(P)
    assert idx.d == 256 and idx.ntotal == 3000               # n <= cap: no threshold pass
    V = idx.reconstruct_n(0, 3000)
    assert V.shape == (3000, 200) and np.array_equal(V[40], V[2500])
    Dr, Ir = OS.flat_ip_search(Q, V, 50)
    D, I = idx.search(Q, 50)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr) and list(I[4, :4]) == [17, 40, 100, 2500]
    one = _index(P[:1])                                      # n = 1: centre = the row, every step 0, every code 0
    assert (one._step.cpu().numpy() == 0).all() and (one._pbf.cpu().numpy() == 0).all()
    V1 = one.reconstruct_n(0, 1)
    assert np.array_equal(V1, P[:1])
    D1, I1 = one.search(Q, 3)
    Dr1, Ir1 = OS.flat_ip_search(Q, V1, 3)
    assert np.array_equal(I1, Ir1) and np.array_equal(D1, Dr1)


def test_a_block_inside_one_band_is_finished_by_the_ladder(torch_cuda):
    """rows that differ by single code steps: more rows than any list holds lie within 2 eps of the k-th score"""
    n, d = 9000, 1024        # eps >= 127 x 1024 / 2 = 65,024 units against scores that differ by at most 2 x 16,256
    unit = f32(0.01)
    C = np.zeros((n, d), dtype=f32)
    C[0], C[1] = 127, -127                                   # the range: step = unit (up to rounding), centre ~ 0
    r = np.arange(2, n)
    C[r, r % d] += 1
    C[r, (r * 7 + 3) % d] -= 1
    P = (C * unit).astype(f32)
    Q = np.random.RandomState(2).randn(3, d).astype(f32)
    idx = _index(P)
    V = idx.reconstruct_n(0, n)
    Dr, Ir = OS.flat_ip_search(Q, V, 10)
    D, I = idx.search(Q, 10)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    assert idx.stats["exhaustive_queries"] > 0 and idx.stats["sq8_first_pass"] < 3, idx.stats


def test_a_second_add_outside_the_range_saturates_and_stays_exact(torch_cuda):
    rs = np.random.RandomState(4)
    A, B = rs.randn(5000, 128).astype(f32), (rs.randn(3000, 128) * 2.5).astype(f32)
    Q = rs.randn(6, 128).astype(f32)
    idx = _index(A)
    codes0, centre, step, _ = _parts(idx)
    idx.add(B.astype(np.float16))                            # (fp16 rows are widened exactly)
    Bw = B.astype(np.float16).astype(f32)
    want, sat = M.codes_of(Bw, centre, step)
    assert sat > 0 and idx.stats["sq8_saturated"] == sat
    codes, centre2, step2, l1 = _parts(idx)
    assert np.array_equal(centre2, centre) and np.array_equal(step2, step) and np.array_equal(codes[5000:], want)
    assert l1 == np.abs(codes.astype(np.int64)).sum(axis=1).max() and codes.min() >= -127
    V = idx.reconstruct_n(0, 8000)
    D, I = idx.search(Q, 100)
    Dr, Ir = OS.flat_ip_search(Q, V, 100)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr) and idx.stats["sq8_saturated"] == sat


def test_stale_workspace_and_outputs_do_not_show(torch_cuda):
    """the same raw call on a zeroed and on a 0xFF-filled workspace (NaN as fp32 / fp64, -1 as integers), outputs pre-set to NaN
    and -7: both certified, both the oracle's answer -- so neither reads a word it did not write"""
    torch = torch_cuda
    idx, P, Q, V, (Dr, Ir) = _corpus()
    q = torch.tensor(Q, device="cuda")
    k = 100
    for fused in (1, 0):
        for fill in (0, 0xFF):
            D, I, st, tr, _, _, _ = M.raw_call(torch, idx, q, k, None, 4096, fused=fused, fill=fill)
            assert (st == OK).all(), (fused, fill, st)
            assert np.array_equal(I, Ir[:, :k]) and np.array_equal(D.view(np.int32), Dr[:, :k].view(np.int32)), (fused, fill)
    D, I, st, _, _, _, _ = M.raw_call(torch, idx, q, 5000, None, 16384, deep=True, fill=0xFF)
    assert (st == OK).all() and np.array_equal(I, Ir) and np.array_equal(D.view(np.int32), Dr.view(np.int32))


def test_remove_rows_save_load_and_a_flipped_step_byte(torch_cuda, tmp_path):
    from convdr_amd import _lib
    from convdr_amd import search as S
    rs = np.random.RandomState(8)
    P = rs.randn(6000, 128).astype(f32)
    Q = rs.randn(5, 128).astype(f32)
    idx = _index(P)
    idx2 = S.FlatIPIndex(128, storage="sq8", prepin=False)
    idx2.add(P, ids=np.arange(6000, dtype=np.int64) * 3)
    gone = np.flatnonzero(rs.rand(6000) < 0.5)
    keep = np.ones(6000, dtype=bool)
    keep[gone] = False
    D0, I0 = idx.search(Q, 50, allowed=keep)
    assert idx.remove_rows(gone) == len(gone) and idx.ntotal == int(keep.sum())
    D1, I1 = idx.search(Q, 50)
    assert np.array_equal(D1, D0) and np.array_equal(I1, (np.cumsum(keep) - 1)[I0])
    # ids, rows_of / id_filter / remove_ids ride on the id column, whatever the rows' width
    Di, Ii = idx2.search_ids(Q, 50, allowed=keep)
    assert np.array_equal(Ii, I0 * 3) and np.array_equal(Di, D0)
    f_ids = idx2.id_filter(np.flatnonzero(keep) * 3)           # the same subset, named by ids
    assert f_ids.n_allowed == int(keep.sum()) and np.array_equal(idx2.search_ids(Q, 50, allowed=f_ids)[1], I0 * 3)
    probe = np.array([0, 3 * 5999, 3 * 77, 1], dtype=np.int64)  # (1 is no id of this index)
    first, count = idx2.rows_of(probe)
    assert first.cpu().tolist() == [0, 5999, 77, -1] and count.cpu().tolist() == [1, 1, 1, 0]
    assert np.array_equal(idx2.reconstruct_ids(probe[:3]), idx2.reconstruct_batch(np.array([0, 5999, 77])))
    twin = S.FlatIPIndex(128, storage="sq8", prepin=False)
    twin.add(P)
    assert twin.keep_rows(twin.row_filter(keep)) == len(gone) and np.array_equal(twin.search(Q, 50)[1], I1)
    assert np.array_equal(twin.reconstruct_n(0, twin.ntotal), idx.reconstruct_n(0, idx.ntotal))
    assert idx2.remove_ids(gone * 3) == len(gone)
    assert np.array_equal(idx2.search_ids(Q, 50)[1], I0 * 3)
    path = str(tmp_path / "sq8.convdr")
    idx2.save(path, window_rows=1024)
    h = S.verify_snapshot(path)
    assert h["storage"] == "sq8" and h["sections"]["rows"]["row_bytes"] == 128 and "step" in h["sections"] and "sq8_saturated" in h
    back = S.FlatIPIndex.load(path, verify=True, prepin=False)
    assert back.fingerprint() == idx2.fingerprint() and back.storage == "sq8"
    Db, Ib = back.search_ids(Q, 50)
    assert np.array_equal(Ib, I0 * 3) and np.array_equal(Db, D0)
    raw = bytearray(open(path, "rb").read())
    raw[h["sections"]["step"]["offset"] + 9] ^= 0x10
    flipped = str(tmp_path / "flipped.convdr")
    with open(flipped, "wb") as f:
        f.write(raw)
    with pytest.raises(_lib.ConvdrError, match=r"section 'step'"):
        S.FlatIPIndex.load(flipped, prepin=False)
    # reset and reserve
    idx.reset()
    idx.reserve(7000)
    idx.add(P)
    assert idx.ntotal == 6000 and np.array_equal(idx.search(Q, 50, allowed=keep)[1], I0)


def test_a_nan_in_an_add_is_refused_and_changes_nothing(torch_cuda):
    from convdr_amd import _lib
    rs = np.random.RandomState(9)
    P, Q = rs.randn(2000, 128).astype(f32), rs.randn(4, 128).astype(f32)
    idx = _index(P)
    fp, (D0, I0) = idx.fingerprint(), idx.search(Q, 20)
    bad = rs.randn(100, 128).astype(f32)
    bad[57, 3] = np.nan
    with pytest.raises(_lib.ConvdrError, match="not finite"):
        idx.add(bad)
    assert idx.ntotal == 2000 and idx.fingerprint() == fp
    D1, I1 = idx.search(Q, 20)
    assert np.array_equal(I1, I0) and np.array_equal(D1, D0)
    empty = __import__("convdr_amd.search", fromlist=["FlatIPIndex"]).FlatIPIndex(128, storage="sq8", prepin=False)
    with pytest.raises(_lib.ConvdrError, match="not finite"):
        empty.add(bad)
    assert empty.ntotal == 0 and empty._centre is None and empty._step is None
    empty.add(P)
    assert np.array_equal(empty.search(Q, 20)[1], I0)


def test_streamed_host_adds_quantise_chunk_by_chunk(torch_cuda):
    """a later add of a host array larger than a staging chunk (fp32, then fp16) is quantised per chunk, over several windows of
    the staging ring: the codes are the model's, row for row"""
    rs = np.random.RandomState(12)
    A = rs.randn(4000, 128).astype(f32)
    B = (rs.randn(30000, 128) * 1.5).astype(f32)
    from convdr_amd.search import FlatIPIndex
    idx = FlatIPIndex(128, storage="sq8", prepin=False)
    idx.host_chunk_bytes = 1 << 20          # 2,048 fp32 rows per chunk, 8,192 per window of four buffers
    idx.add(A)                              # (the first add: streamed whole, then centre and step)
    codes, centre, step, _ = _parts(idx)
    assert (codes == M.codes_of(A, centre, step)[0]).all()
    idx.add(B)
    idx.add(B.astype(np.float16))
    codes, c2, s2, l1 = _parts(idx)
    w32, sat32 = M.codes_of(B, centre, step)
    w16, sat16 = M.codes_of(B.astype(np.float16).astype(f32), centre, step)
    assert idx.ntotal == 64000 and np.array_equal(c2, centre) and np.array_equal(s2, step)
    assert np.array_equal(codes[4000:34000], w32) and np.array_equal(codes[34000:], w16)
    assert idx.stats["sq8_saturated"] == sat32 + sat16 > 0 and l1 == np.abs(codes.astype(np.int64)).sum(axis=1).max()
