"""The certificate of queries that are NOT certified: the raw first pass of the three cut kernels (k_ip_finish, k_ip_cut,
k_ip_cut_deep) must draw the same verdict -- status and the bits of tau_retry -- from the same list, and the list entries
(range, rank of rows, rank of documents) the same RANGE.  Every other suite compares certified queries only.

One block of 3,000 x 64 rows, 8 queries, k = 10.  A per-query tau_in, chosen on the CPU from fp64 scores, makes every verdict
occur: -inf (OK), a quarter of the error band below the exact k-th score (UNCERTAIN), +1e30 (TOO_FEW); cap = 1,024 with
tau_in = -inf overflows the list; an fp16 copy built with 16 times its scale is out of RANGE.  That the thresholds must give
these verdicts is checked on the CPU first (_expect), with the scan emulated: bf16 operands, fp64 sums, the fp32 accumulation
charged at d 2^-23 |q| max|p|."""
import numpy as np
import pytest

from tests.golden.make_golden import synth_corpus
from tests.index_cases import torch_cuda      # noqa: F401 (the fixture, by name)

pytestmark = pytest.mark.gpu

N, D, NQ, K = 3000, 64, 8, 10
N_TILES = (N + 255) // 256 * 256        # rows the scan scores: whole 256-row tiles
OK, OVERFLOW, TOO_FEW, UNCERTAIN, RANGE = 0, 1, 2, 3, 4
WANT = np.asarray([OK, UNCERTAIN, TOO_FEW, OK, UNCERTAIN, TOO_FEW, UNCERTAIN, OK], np.int32)
NEG_INF_BITS = np.float32(-np.inf).view(np.int32)

_DATA = {}


def _data():
    if not _DATA:
        _DATA["P"], _DATA["Q"] = synth_corpus(71, N, D), synth_corpus(72, NQ, D)
        for a in _DATA.values():
            a.setflags(write=False)
    return _DATA["P"], _DATA["Q"]


def _bf16(x):
    """fp32 -> bf16 -> fp32, round to nearest even (finite inputs)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)


def _expect(idx, P, Q):
    """(tau_in fp32 [NQ], eps [NQ], emulated scan scores [NQ, N], their slack [NQ]) and the CPU's proof that tau_in gives WANT"""
    c = idx._centre.cpu().numpy()
    pm = float(idx._max_norm.item())                               # max |p - centre|, as the kernels read it
    qn = np.linalg.norm(Q.astype(np.float64), axis=1) * (1 + 1e-6)
    u = 2.0 ** -8
    eps = (2 * u + u * u + D / 8388608.0) * 1.0001 * qn * pm * 1.001                    # ip_eps_coef, IpBand::eps (bf16: no absolute term)
    S = Q.astype(np.float64) @ (P.astype(np.float64) - c.astype(np.float64)).T          # exact, in scan units
    Se = _bf16(Q).astype(np.float64) @ _bf16(P - c).astype(np.float64).T                # the scan, but for its fp32 accumulation
    slack = D * 2.0 ** -23 * qn * pm
    kth = -np.sort(-S, axis=1)[:, K - 1]
    kth_e = -np.sort(-Se, axis=1)[:, K - 1]
    tau = np.where(WANT == OK, -np.inf, np.where(WANT == TOO_FEW, 1e30, kth - eps / 4)).astype(np.float32)
    for j in np.flatnonzero(WANT == UNCERTAIN):
        # at least K rows are listed whatever the accumulation order, and S~(k) - 2 eps lies below the threshold
        assert (Se[j] >= tau[j] + slack[j]).sum() >= K, j
        assert kth_e[j] + slack[j] - 2 * eps[j] * (1 - 1e-5) < tau[j], j
    assert Se.max() + slack.max() < 1e30                                                # TOO_FEW: no row is listed
    return tau, eps, Se, slack


def _raw(torch, idx, q, tau_in, cap, deep=False, fused=1):
    """one raw call of the index's top-k entry; (status, tau_retry bits, hit counts, band sizes) -- the last two shallow only"""
    from convdr_amd import _lib
    L = _lib.lib()
    nq, n = int(q.shape[0]), idx.ntotal
    need = (L.convdr_ip_deep_workspace_bytes if deep else L.convdr_ip_workspace_bytes)(nq, n, idx.d, K, cap)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    Dv = torch.empty((nq, K), dtype=torch.float32, device="cuda")
    Iv = torch.empty((nq, K), dtype=torch.int64, device="cuda")
    st = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
    tr = torch.zeros(nq, dtype=torch.float32, device="cuda")
    assert L.convdr_set_option(b"ip_fused_finish", fused) == 0
    try:
        idx._search_call(q, nq, idx._p32, idx._pbf, None, n, K, tau_in, cap, 0, ws, Dv, Iv, st, tr, False, deep)
        torch.cuda.synchronize()
    finally:
        assert L.convdr_set_option(b"ip_fused_finish", 1) == 0
    dbg = [None, None]
    if not deep:
        for i, fn in enumerate((L.convdr_ip_debug_counts, L.convdr_ip_debug_band)):
            off = fn(_lib.ptr(ws), nq, n, idx.d, K, cap) - ws.data_ptr()
            dbg[i] = ws[off:off + 4 * nq].view(torch.int32).cpu().numpy()
    return st.cpu().numpy(), tr.cpu().numpy().view(np.int32), dbg[0], dbg[1]


def test_every_verdict_of_the_three_cut_kernels(torch_cuda):
    torch = torch_cuda
    from convdr_amd.search import FlatIPIndex
    P, Q = _data()
    idx = FlatIPIndex(D, precision="bf16")
    idx.add(P)
    tau, eps, Se, slack = _expect(idx, P, Q)
    q, t = torch.tensor(Q, device="cuda"), torch.tensor(tau, device="cuda")
    fused = _raw(torch, idx, q, t, 8192, fused=1)
    chain = _raw(torch, idx, q, t, 8192, fused=0)
    deep = _raw(torch, idx, q, t, 16384, deep=True)
    print("status", fused[0], "tau_retry", fused[1].view(np.float32), "hits", fused[2], "band", fused[3])
    np.testing.assert_array_equal(fused[0], WANT)
    assert {OK, TOO_FEW, UNCERTAIN} <= set(fused[0].tolist())
    for name, a, b in zip(("status", "tau_retry bits", "hit count", "band size"), fused, chain):
        np.testing.assert_array_equal(a, b, err_msg="k_ip_finish against k_ip_cut: " + name)
    np.testing.assert_array_equal(deep[0], fused[0], err_msg="k_ip_cut_deep: status")
    np.testing.assert_array_equal(deep[1], fused[1], err_msg="k_ip_cut_deep: tau_retry bits")
    # what the verdicts say, against the CPU: hits, and a retry threshold only where there is something to retry
    # (no threshold: the rows past the block's end in the scan's last tile score -inf and are listed too; the cut drops them)
    assert (fused[2][WANT == OK] == N_TILES).all() and (fused[2][WANT == TOO_FEW] == 0).all()
    assert (fused[1][WANT == OK] == NEG_INF_BITS).all()
    retry = fused[1].view(np.float32).astype(np.float64)
    for j in np.flatnonzero(WANT == UNCERTAIN):
        assert K <= fused[2][j] < N and fused[3][j] == fused[2][j]          # the band is the whole list: it reaches below tau
        assert retry[j] < tau[j] and abs(retry[j] - (np.sort(Se[j])[-K] - 2 * eps[j])) <= slack[j] + 1e-4 * eps[j]
    for j in np.flatnonzero(WANT == TOO_FEW):
        assert abs(retry[j] - (1e30 - 1e-3 * 1e30)) <= 1e-6 * 1e30


def test_overflow_verdict_fused_and_three_launch(torch_cuda):
    """cap = 1,024 and no threshold: every scored row hits (3,072: the last tile's rows past the end score -inf).  WHICH 1,024
    of them hold the list's slots depends on the order the scan's reservations arrive in, so the cut over the stored scores --
    and with it tau_retry and the band -- differs from run to run (each call scans for itself): status and hit count are
    compared, the retry threshold is held to what any stored subset allows: finite, at most S~(k) - 2 eps of the whole block
    (a subset's k-th score is not above the block's) and not below that of the 1,024 worst."""
    torch = torch_cuda
    from convdr_amd.search import FlatIPIndex
    P, Q = _data()
    idx = FlatIPIndex(D, precision="bf16")
    idx.add(P)
    _, eps, Se, slack = _expect(idx, P, Q)
    q = torch.tensor(Q, device="cuda")
    t = torch.full((NQ,), -np.inf, dtype=torch.float32, device="cuda")
    kth_e = -np.sort(-Se, axis=1)[:, K - 1]
    low_e = -np.sort(-Se, axis=1)[:, N_TILES - 1024 + K - 1]    # the k-th best of the WORST 1,024 scored rows (a real row)
    assert N_TILES - 1024 + K - 1 < N
    runs = [_raw(torch, idx, q, t, 1024, fused=f) for f in (1, 0)]
    for st, tr, hits, band in runs:
        print("status", st, "tau_retry", tr.view(np.float32), "hits", hits, "band", band)
        assert (st == OVERFLOW).all() and (hits == N_TILES).all() and ((band >= K) & (band <= 1024)).all(), (st, hits, band)
        retry = tr.view(np.float32).astype(np.float64)
        assert np.isfinite(retry).all()
        assert (retry <= kth_e + slack - 2 * eps * (1 - 1e-5)).all() and (retry >= low_e - slack - 2 * eps * (1 + 1e-5) - 1e-4).all()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][2], runs[1][2])


def test_range_verdict_of_every_entry(torch_cuda):
    """An fp16 copy built with 16 times the scale that fits its norms: max norm x scale >= 65,536 > 60,000.  All three cut
    kernels report RANGE with tau_retry = -inf, and so do the range, rank-rows and rank-docs entries on the same block."""
    torch = torch_cuda
    from convdr_amd import _lib
    from convdr_amd.search import FlatIPIndex
    P, Q = _data()
    idx = FlatIPIndex(D, precision="fp16")
    idx.add(P, ids=np.arange(N, dtype=np.int64) // 3)
    idx._scale = float(idx._scale) * 16.0
    idx._prepare_into(idx._p32, idx._pbf, idx._plo)
    assert float(idx._max_norm.item()) * idx._scale > 60000.0
    L, ptr = _lib.lib(), _lib.ptr
    q = torch.tensor(Q, device="cuda")
    for kw in (dict(cap=8192, fused=1), dict(cap=8192, fused=0), dict(cap=16384, deep=True)):
        st, tr, _, _ = _raw(torch, idx, q, None, **kw)
        assert (st == RANGE).all() and (tr == NEG_INF_BITS).all(), (kw, st, tr.view(np.float32))
    store, r32, r16, scale, centre = idx._operands()
    assert store == 1
    cap = 4096
    # range search
    need = L.convdr_ip_range_workspace_bytes(NQ, N, D, cap)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rad = torch.zeros(NQ, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(NQ, dtype=torch.int64, device="cuda")
    lims = torch.zeros(NQ + 1, dtype=torch.int64, device="cuda")
    st = torch.full((NQ,), -1, dtype=torch.int32, device="cuda")
    _lib.check(L.convdr_ip_range_search(store, ptr(q), NQ, r32, r16, scale, centre, N, D, ptr(idx._max_norm), ptr(rad), cap, 0, None, 0,
                                        ptr(ws), need, ptr(cnt), ptr(lims), ptr(st), _lib.stream_ptr()), "convdr_ip_range_search")
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == RANGE).all() and int(lims[-1].item()) == 0
    # rank of rows, rank of documents
    o = idx.doc_ordinals()
    tgt = torch.arange(NQ, dtype=torch.int64, device="cuda") * 7
    for docs in (False, True):
        need = (L.convdr_ip_rank_docs_workspace_bytes(NQ, N, D, cap, o.ndocs) if docs else L.convdr_ip_rank_workspace_bytes(NQ, N, D, cap))
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        rank = torch.zeros(NQ, dtype=torch.int64, device="cuda")
        X = torch.zeros(NQ, dtype=torch.float64, device="cuda")
        cnt = torch.zeros(NQ, dtype=torch.int64, device="cuda")
        above = torch.zeros(NQ, dtype=torch.int64, device="cuda")
        st = torch.full((NQ,), -1, dtype=torch.int32, device="cuda")
        head = (store, ptr(q), NQ, ptr(tgt), r32, r16, scale, centre, N, D, ptr(idx._max_norm), None, 0, 0)
        tail = (cap, ptr(ws), need, ptr(rank), ptr(X), ptr(cnt), ptr(above), ptr(st), _lib.stream_ptr())
        if docs:
            _lib.check(L.convdr_ip_rank_docs(*head, ptr(o.ord), o.ndocs, *tail), "convdr_ip_rank_docs")
        else:
            _lib.check(L.convdr_ip_rank_rows(*head, *tail), "convdr_ip_rank_rows")
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == RANGE).all() and (rank.cpu().numpy() == -1).all(), (docs, st, rank)
