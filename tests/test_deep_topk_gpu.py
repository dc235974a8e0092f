"""Exact top-k for 4096 < k <= 65536 on the device (convdr_ip_search_deep*: candidate lists, band and ordering in global
memory) and the driver-level block walk at that depth.  Every comparison is bit-exact against the CPU oracle."""
import numpy as np
import pytest

from oracle import search as OS
from tests import helpers
from tests.golden.make_golden import synth_corpus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _index(d, **kw):
    from convdr_amd.search import FlatIPIndex
    return FlatIPIndex(d, **kw)


_CASES = {}


def _case(n, nq, k, d):
    """(P, Q, Dr, Ir) of one shape, computed once and shared; the arrays are never written to afterwards."""
    key = (n, nq, k, d)
    if key not in _CASES:
        P, Q = synth_corpus(300 + n % 83, n, d), synth_corpus(9, nq, d)
        P[n - 50:n - 10] = P[10:50]             # exact duplicates far apart: equal scores, index order decides
        out = (P, Q) + tuple(OS.flat_ip_search(Q, P, k))
        for a in out:
            a.setflags(write=False)
        _CASES[key] = out
    return _CASES[key]


def _check_deep(idx, Q, k, Dr, Ir, nq):
    D, I = idx.search(Q, k)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)
    assert D.dtype == np.float32 and I.dtype == np.int64
    st = idx.stats
    assert st["large_k"] == k and st["deep"] == nq and st["chunked_queries"] == 0, st
    return st


SHAPES = [
    (20000, 3, 4097, 64),       # first k of the route; n just above the 16,384-entry list: threshold (every score a sample) + emit
    (40000, 3, 5000, 64),       # sampled threshold; k > n / 128
    (70000, 2, 20000, 64),      # list of 65,536 < n; the ordering spans many LDS tiles
    (140000, 1, 65536, 64),     # the contract's upper end, list of 131,072 < n
    (13000, 2, 13000, 128),     # every row a candidate, k = n
    (6000, 2, 9000, 64),        # k > n: FAISS padding in the tail
    (20000, 130, 4500, 64),     # more than 128 queries: the 256 x 256 scan tile class and padded query rows
]


@pytest.mark.parametrize("n,nq,k,d", SHAPES)
def test_deep_search_matches_oracle_bit_exact(torch_cuda, n, nq, k, d):
    P, Q, Dr, Ir = _case(n, nq, k, d)
    idx = _index(d)
    idx.add(P)
    st = _check_deep(idx, Q, k, Dr, Ir, nq)
    assert st["deep_cap"] >= 2 * k and st["deep_cap"] & (st["deep_cap"] - 1) == 0, st
    if k > n:
        assert (Ir[:, n:] == -1).all() and (Ir[:, :n] >= 0).all()


def test_deep_search_on_the_bf16_rung(torch_cuda):
    n, nq, k, d = 40000, 3, 5000, 64
    P, Q, Dr, Ir = _case(n, nq, k, d)
    idx = _index(d, precision="bf16")
    idx.add(P)
    _check_deep(idx, Q, k, Dr, Ir, nq)


def test_deep_search_ignores_the_fused_finish_switch(torch_cuda):
    from convdr_amd import _lib
    n, nq, k, d = 20000, 3, 4097, 64
    P, Q, Dr, Ir = _case(n, nq, k, d)
    idx = _index(d)
    idx.add(P)
    L = _lib.lib()
    assert L.convdr_set_option(b"ip_fused_finish", 0) == 0
    try:
        _check_deep(idx, Q, k, Dr, Ir, nq)
    finally:
        assert L.convdr_set_option(b"ip_fused_finish", 1) == 0


def test_tie_group_larger_than_any_lds_list(torch_cuda):
    """5,000 copies of one row, scattered over the index range, that scores near the top for query 0: the result lists them
    in index order.  (The chunked route cannot order more than 4,096 rows that share one fp32 score and raises.)"""
    n, d, k, nq = 20000, 64, 6000, 2
    P, Q = synth_corpus(411, n, d), synth_corpus(12, nq, d)
    s0 = P.astype(np.float64) @ Q[0].astype(np.float64)
    tenth = int(np.argsort(-s0)[9])                      # the 10th best row of query 0
    rows = np.random.RandomState(3).choice(n, 5000, replace=False)
    rows = np.union1d(rows[rows != tenth][:4999], [tenth])
    P[rows] = P[tenth].copy()
    Dr, Ir = OS.flat_ip_search(Q, P, k)
    start = int(np.nonzero(Ir[0] == rows[0])[0][0])
    assert len(rows) == 5000 and start < 16 and np.array_equal(Ir[0, start:start + 5000], rows)   # the oracle: one run, ascending
    idx = _index(d)
    idx.add(P)
    _check_deep(idx, Q, k, Dr, Ir, nq)


def test_block_no_scan_can_certify(torch_cuda):
    """5,000 of 20,000 rows are 300 times longer: the error band, which scales with the longest row, swallows any list.
    Whatever rung answers, the answer is the oracle's."""
    n, d, k, nq = 20000, 64, 4200, 3
    P = np.concatenate([synth_corpus(81, 15000, d), synth_corpus(82, 5000, d) * np.float32(300.0)])
    Q = synth_corpus(83, nq, d)
    idx = _index(d)
    idx.add(P[:15000])
    idx.add(P[15000:])
    D, I = idx.search(Q, k)
    Dr, Ir = OS.flat_ip_search(Q, P, k)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)
    st = idx.stats
    assert st["large_k"] == k and st["deep"] + st["chunked_queries"] == nq, st
    # the rung is recorded, not pinned
    helpers.margin("deep_topk/uncertifiable/chunked_queries", st["chunked_queries"], nq)
    helpers.margin("deep_topk/uncertifiable/x3_queries", st["x3_queries"], nq)
    helpers.margin("deep_topk/uncertifiable/rounds", st["rounds"], 16)
    helpers.margin("deep_topk/uncertifiable/deep_cap", st["deep_cap"], 131072)


def test_k_beyond_the_deep_limit_takes_the_chunked_route(torch_cuda):
    from convdr_amd.search import FlatIPIndex
    n, nq, d = 66000, 1, 64
    k = FlatIPIndex.DEEP_MAX_K + 1
    P, Q = synth_corpus(300 + n % 83, n, d), synth_corpus(9, nq, d)
    idx = _index(d)
    idx.add(P)
    D, I = idx.search(Q, k)
    Dr, Ir = OS.flat_ip_search(Q, P, k)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)
    assert idx.stats["large_k"] == k and idx.stats["deep"] == 0 and idx.stats["chunked_queries"] == nq, idx.stats


def test_deep_search_does_not_depend_on_stale_memory(torch_cuda):
    """The index's workspace and the memory the outputs land in are pre-filled (zeros, 0xFF = NaN bytes, random bytes): one raw
    deep pass (D, I, status, tau_retry) and the certified result are the same bits every time."""
    torch = torch_cuda
    n, nq, k, d = 40000, 3, 5000, 64
    P, Q, Dr, Ir = _case(n, nq, k, d)
    idx = _index(d)
    idx.add(P)
    q = torch.from_numpy(Q).cuda()
    idx.search_deep_device(q, k)
    ptr = idx._ws.data_ptr()
    runs = {}
    for i, f in enumerate(helpers.FILLS):
        helpers.fill_bytes(idx._ws, f, seed=41 + i)
        # the outputs are torch.empty inside the call: the allocator hands back these blocks
        stale = [helpers.fill_bytes(torch.empty((nq, k), dtype=dt, device="cuda"), f, seed=51 + i)
                 for dt in (torch.float32, torch.int64)]
        del stale
        D, I, st, tr = idx.search_deep_device(q, k)
        runs[f] = ({"D": D.clone(), "I": I.clone(), "status": st.clone(), "tau_retry": tr.clone().view(torch.int32)},
                   ptr, idx._ws.data_ptr())
    helpers.assert_fills_agree(runs, "deep/%d_%d_%d" % (n, nq, k))
    assert (runs["Z"][0]["status"] == 0).all()
    np.testing.assert_array_equal(runs["Z"][0]["I"].cpu().numpy(), Ir)
    np.testing.assert_array_equal(runs["Z"][0]["D"].cpu().numpy(), Dr)
    for f in helpers.FILLS:
        helpers.fill_bytes(idx._ws, f, seed=5)
        _check_deep(idx, Q, k, Dr, Ir, nq)


def test_deep_search_is_the_same_bytes_run_to_run(torch_cuda):
    torch = torch_cuda
    n, nq, k, d = 70000, 2, 20000, 64
    P, Q, Dr, Ir = _case(n, nq, k, d)
    idx = _index(d)
    idx.add(P)
    a = idx.search_tensors(Q, k)
    b = idx.search_tensors(Q, k)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    np.testing.assert_array_equal(a[1].cpu().numpy(), Ir)


def test_search_one_by_one_at_depth(torch_cuda, tmp_path):
    """Three block files, topN = 5,000: the running merge of lists longer than convdr_topk_merge takes."""
    from convdr_amd import blocks
    from convdr_amd import search as S
    sizes, d, nq, topN = (6000, 7000, 5500), 64, 3, 5000
    rs = np.random.RandomState(0)
    Q = rs.randn(nq, d).astype(np.float32)
    embs = [rs.randn(n, d).astype(np.float32) for n in sizes]
    embs[1][77], embs[2][4001] = 2.0 * Q[0], 2.0 * Q[0]         # equal best hits of query 0 in two blocks (2 |q|^2 ~ 128, the random rows' ~ 4 x 8)
    embs[2][10:40] = embs[0][100:130]                           # thirty duplicates across blocks 0 and 2
    embs[1][6000:6020] = embs[0][5000:5020]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    ids = [np.arange(starts[b], starts[b + 1], dtype=np.int64) for b in range(len(sizes))]
    for b, (e, i) in enumerate(zip(embs, ids)):
        blocks.dump_block(str(tmp_path / ("passage__emb_p__data_obj_%d.pb" % b)), e)
        blocks.dump_block(str(tmp_path / ("passage__embid_p__data_obj_%d.pb" % b)), i)
    mD, mI = OS.search_one_by_one(list(zip(embs, ids)), Q, topN)
    assert mD.shape == (nq, 2 * topN) and list(mI[0, :2]) == [int(ids[1][77]), int(ids[2][4001])]
    index = S.FlatIPIndex(d)
    D, I = S.search_one_by_one(str(tmp_path), index, Q, topN)
    assert D.dtype == np.float64 and I.dtype == np.int64 and D.shape == I.shape == (nq, 2 * topN)
    np.testing.assert_array_equal(I, mI)
    np.testing.assert_array_equal(D, mD)
