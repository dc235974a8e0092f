"""A numpy model of the 8-bit store (FlatIPIndex(storage="sq8")), written from include/convdr_hip.h "8-bit store" and the
derivation beside IP_Q8_COEF (csrc/ip_topk.hip) -- the quantiser, the reconstruction, the query's hi / lo split, the integer
scan, the exact scaled score E and the documented band WITHOUT the library's safety factors -- and the input families of
tests/test_sq8_store_cpu.py and tests/test_sq8_store_gpu.py.  float32 arithmetic is numpy's: one rounding per operation."""
import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
QMAX = 16256                      # 127 x 128
R_DOC = 16256 * U * (2 + 2 * U) + 2.0 ** -36      # query rounding + int-to-float conversion, per unit of ||c||_1
FAMILIES = ("random", "aligned", "saturated", "offset", "onehot")


def step_of(P, centre):
    """step[j] = max_i |p_ij - centre_j| / 127 in fp32; a quotient below the normal range is a constant column"""
    s = (np.abs(P.astype(f32) - centre.astype(f32)).max(axis=0) / f32(127)).astype(f32)
    return np.where(s >= np.finfo(f32).tiny, s, f32(0)).astype(f32)


def codes_of(P, centre, step):
    """(codes int8 [n, d], saturated count)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.rint((P.astype(f32) - centre) / step)
    t = np.where(step > 0, t, f32(0))
    sat = int((np.abs(t) > 127).sum())
    return np.clip(t, -127, 127).astype(np.int8), sat


def reconstruct(codes, centre, step):
    """v = fl32(centre + fl32(step * c))"""
    return (centre.astype(f32) + (step.astype(f32) * codes.astype(f32)).astype(f32)).astype(f32)


def query_split(Q, step):
    """(hi int32 [nq, d], lo, te int [nq]): q' = fl32(q step), t = 2^te with max |q'| / t in (8128, 16256], Qi = rint(q' / t)"""
    qp = (Q.astype(f32) * step.astype(f32)).astype(f32)
    mx = np.abs(qp).max(axis=1)
    te = np.zeros(len(Q), dtype=np.int64)
    for i, m in enumerate(mx):
        if m > 0:
            _, ex = np.frexp(m)
            te[i] = int(ex) - 14
            if np.ldexp(f64(m), -int(te[i])) > QMAX:
                te[i] += 1
    qi = np.rint(np.ldexp(qp.astype(f64), -te[:, None])).astype(np.int64)
    hi = (qi + 64) >> 7
    lo = qi - 128 * hi
    return hi.astype(np.int32), lo.astype(np.int32), te


def int_scan(hi, lo, codes):
    """(S int64 [nq, n] = 128 S_hi + S_lo, S_hi, S_lo): the integers the MFMA accumulates"""
    c = codes.astype(np.int64)
    s_hi, s_lo = hi.astype(np.int64) @ c.T, lo.astype(np.int64) @ c.T
    return 128 * s_hi + s_lo, s_hi, s_lo


def exact_scaled(Q, codes, centre, step, te):
    """E [nq, n] = (1 / t) sum_j q_j (v_ij - centre_j) in fp64"""
    w = reconstruct(codes, centre, step).astype(f64) - centre.astype(f64)
    return np.ldexp(Q.astype(f64) @ w.T, -te[:, None])


def a_term(Q, centre, step, te):
    """A(q) = (u / t) sum_j |q_j| (|centre_j| + 127 (2 + u) step_j)"""
    rho = np.abs(centre.astype(f64)) + 127 * (2 + U) * step.astype(f64)
    return np.ldexp(U * (np.abs(Q.astype(f64)) @ rho), -te)


def eps_doc(Q, codes, centre, step, te, l1max=None):
    l1max = np.abs(codes.astype(np.int64)).sum(axis=1).max() if l1max is None else l1max
    return (0.5 + R_DOC) * float(l1max) + a_term(Q, centre, step, te)


def family(fam, d, nq, n, seed=0):
    """(Q [nq, d], P [n, d]) fp32: rows whose first-add quantisation shows the family's property"""
    rs = np.random.RandomState(1000 * seed + 17 * d + nq + n + FAMILIES.index(fam))
    spread = np.exp(rs.uniform(-0.55, 0.55, d)).astype(f32)         # per-column spreads over a factor of ~3
    P = (rs.randn(n, d) * spread).astype(f32)
    Q = rs.randn(nq, d).astype(f32)
    if fam == "aligned":
        Q = (P[np.arange(nq) % n] * f32(1.7)).astype(f32)
    elif fam == "saturated":                                        # every code +-127: rows at the ends of every column's range
        assert n % 2 == 0                                           # (in +- pairs: the column mean is exactly 0)
        half = (np.where(rs.rand(n // 2, d) < 0.5, -1, 1) * spread).astype(f32)
        P[0::2], P[1::2] = half, -half
    elif fam == "offset":                                           # large centre, small spread: the roundings of v dominate
        P = (f32(100) + f32(0.01) * P).astype(f32)
    elif fam == "onehot":                                           # one large element: hi = +-127 there (or nearly), lo everything else
        Q = (f32(1e-3) * Q).astype(f32)
        Q[np.arange(nq), (7 * np.arange(nq)) % d] = f32(3.0) * np.where(np.arange(nq) % 2, -1, 1)
    return Q, P


def lane_map_case(d, nq, n=512):
    """Integer data with centre exactly 0 and step exactly 1 (rows in +- pairs, +-127 in every column), so that the stored codes
    ARE the rows, and integer queries with max |q| in (8128, 16256], so that t = 1 and Qi = q: (Q, P, codes) with every
    product asymmetric in (row, column) and in (query, column)."""
    r, j = np.arange(n // 2)[:, None], np.arange(d)[None, :]
    half = ((r * 7 + j * 13 + (r * j) % 5) % 255 - 127).astype(np.int64)
    half[0] = 127
    P = np.empty((n, d), dtype=np.int64)
    P[0::2], P[1::2] = half, -half
    i = np.arange(nq)[:, None]
    Q = ((i * 3701 + j * 1013 + (i * j) % 11) % 16001 - 8000).astype(np.int64)
    Q[:, 0] = QMAX - np.arange(nq) % 100
    return Q.astype(f32), P.astype(f32), P.astype(np.int8)


# ---- device helpers of tests/test_sq8_store_gpu.py: one raw call of the store's top-k entry and the reading of what it left -----
OK, OVERFLOW, TOO_FEW, UNCERTAIN, RANGE = 0, 1, 2, 3, 4
K_BAND = 10


def raw_call(torch, idx, q, k, tau_in, cap, fused=0, deep=False, allowed=None, fill=0):
    """One call of the index's top-k entry on a workspace of its own, every byte of it and of the outputs pre-set (`fill`: the
    workspace's byte; 0xFF reads as NaN / -1).  Returns (D, I, status, tau_retry bits, hits, band, ws); hits / band shallow only."""
    import ctypes as C     # noqa: F401
    from convdr_amd import _lib
    L = _lib.lib()
    nq, n = int(q.shape[0]), idx.ntotal
    need = (L.convdr_ip_deep_workspace_bytes if deep else L.convdr_ip_workspace_bytes)(nq, n, idx.d, k, cap)
    assert need > 0
    ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
    Dv = torch.full((nq, k), float("nan"), dtype=torch.float32, device="cuda")
    Iv = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    st = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
    tr = torch.full((nq,), float("nan"), dtype=torch.float32, device="cuda")
    assert L.convdr_set_option(b"ip_fused_finish", fused) == 0
    try:
        idx._search_call(q, nq, None, idx._pbf, None, n, k, tau_in, cap, 0, ws, Dv, Iv, st, tr, False, deep, allowed)
        torch.cuda.synchronize()
    finally:
        assert L.convdr_set_option(b"ip_fused_finish", 1) == 0
    dbg = [None, None]
    if not deep:
        for i, fn in enumerate((L.convdr_ip_debug_counts, L.convdr_ip_debug_band)):
            off = fn(_lib.ptr(ws), nq, n, idx.d, k, cap) - ws.data_ptr()
            dbg[i] = ws[off:off + 4 * nq].view(torch.int32).cpu().numpy()
    return Dv.cpu().numpy(), Iv.cpu().numpy(), st.cpu().numpy(), tr.cpu().numpy().view(np.int32), dbg[0], dbg[1], ws


def scan_list(torch, ws, nq, n, d, k, cap):
    """(ids int64 [nq, cap], scan scores fp32 [nq, cap]) of the call that last used ws (convdr_ip_debug_list)"""
    import ctypes as C
    from convdr_amd import _lib
    pi, ps = C.c_void_p(), C.c_void_p()
    assert _lib.lib().convdr_ip_debug_list(_lib.ptr(ws), nq, n, d, k, cap, C.byref(pi), C.byref(ps)) == 0
    out = []
    for p, dt in ((pi, torch.int32), (ps, torch.float32)):
        off = p.value - ws.data_ptr()
        assert 0 <= off and off + 4 * nq * cap <= ws.numel()
        out.append(ws[off:off + 4 * nq * cap].view(dt).view(nq, cap).cpu().numpy())
    return out[0].astype(np.int64), out[1]


def scan_sample(torch, ws, nq, n, d, k, cap):
    """the threshold sample as [rows of the scanned tiles, nq] fp32, or None (convdr_ip_debug_sample)"""
    import ctypes as C
    from convdr_amd import _lib
    pT, ld = C.c_void_p(), C.c_int64()
    assert _lib.lib().convdr_ip_debug_sample(_lib.ptr(ws), nq, n, d, k, cap, C.byref(pT), C.byref(ld)) == 0
    if pT.value is None:
        return None
    rows = (n + 255) // 256 * 256
    off = pT.value - ws.data_ptr()
    assert 0 <= off and off + 4 * rows * ld.value <= ws.numel() and ld.value >= nq
    return ws[off:off + 4 * rows * ld.value].view(torch.float32).view(rows, ld.value)[:, :nq].cpu().numpy()


def scores_from_list(ids, s, band, n, what):
    """every row exactly once among the first `band` entries, and S~ [nq, n] in row order"""
    assert (band == n).all(), (what, "band sizes", band, n)
    head = ids[:, :n]
    order = np.argsort(head, axis=1, kind="stable")
    assert (np.take_along_axis(head, order, axis=1) == np.arange(n)[None, :]).all(), (what, "rows listed twice, missing, or past n")
    return np.take_along_axis(s[:, :n], order, axis=1)


def hold_band(torch, idx, q, S, E, eps, cap, what):
    """The library's own band: a second call (k = 10, tau_in a quarter band below the exact k-th score) comes back UNCERTAIN with
    tau_retry = S~(k) - 2 eps_lib, and eps_doc <= eps_lib <= 1.003 eps_doc, held on tau_retry's own fp32 arithmetic.  Returns
    how many queries were UNCERTAIN for certain and held."""
    kth = -np.sort(-E, axis=1)[:, K_BAND - 1]
    tau = (kth - eps / 4).astype(f32)
    s10 = -np.sort(-S, axis=1)[:, K_BAND - 1]
    listed = (S >= tau[:, None]).sum(axis=1)
    t64, s64 = tau.astype(f64), s10.astype(f64)
    sure = (listed >= K_BAND) & (s64 - 2 * eps < t64 - 1e-6 * (np.abs(t64) + np.abs(s64)))
    _, _, st, tr, hits, band, _ = raw_call(torch, idx, q, K_BAND, torch.tensor(tau, device="cuda"), cap, fused=0)
    assert (hits == listed).all(), (what, "hits", hits, listed)
    assert (st[sure] == UNCERTAIN).all() and (st[listed < K_BAND] == TOO_FEW).all(), (what, st, listed)
    retry = tr.view(f32)
    e_lo = eps.astype(f32)
    e_lo = np.where(e_lo.astype(f64) > eps, np.nextafter(e_lo, f32(0)), e_lo)
    e_hi = (1.003 * eps).astype(f32)
    e_hi = np.where(e_hi.astype(f64) < 1.003 * eps, np.nextafter(e_hi, f32(np.inf)), e_hi)
    top = np.nextafter((s10 - f32(2) * e_lo).astype(f32), f32(-np.inf))
    bot = np.nextafter((s10 - f32(2) * e_hi).astype(f32), f32(-np.inf))
    for j in np.flatnonzero(sure):
        assert bot[j] <= retry[j] <= top[j], (what, j, float(retry[j]), (float(s10[j]) - float(retry[j])) / 2 / eps[j])
    return int(sure.sum())
