"""The one inequality every search result rests on, measured on the device: |S~ - exact scaled score| <= eps for every (query,
row), S~ the RAW score of the scan kernels (k_ip_scan_r3, k_ip_scan<.., PASSES>), read back through convdr_ip_debug_list /
convdr_ip_debug_sample.  Reference, bound and input families: tests/scan_error_cases.py (fp64 from the fp32 inputs; eps_doc from
the formulas documented in csrc/ip_topk.hip, without the library's safety factors); what the families reach in a CPU model of
the scan: test_scan_error_cpu.py.

Rungs: the four precisions of the fp32 store and the half store in one and two passes.  Shapes: d = 64 (one K step), 768, 4096
(the entry's maximum: the largest accumulation term; 5 queries only); nq = 5 (IP_TILE_TALL) and 130 (IP_TILE_256); the list
route with n = 1,024 and 1,000 (ragged last tile), k = n, cap = 8,192 on the three-launch chain -- the band is the whole list, so
the list holds every row's scan score --, and the sample route n = 1,280, cap = 1,024, k = 10 (IP_MODE_FULL: the threshold
sample holds every row's score).  Per case and family:
  1. list completeness   every row exactly once among the first convdr_ip_debug_band entries;
  2. the inequality      |S~ - exact| <= eps_doc for every pair;
  3. the library's band  a second call (k = 10, tau_in a quarter band below the exact k-th score) comes back UNCERTAIN with
                         tau_retry = S~(k) - 2 eps_lib, and eps_doc <= eps_lib <= 1.003 eps_doc (1.0001 x 1.001 x the norms' 1 + 1e-6):
                         held on tau_retry's own fp32 arithmetic, which is monotone in eps;
  4. norms               idx._max_norm in [1, 1 + 1e-5] x max |p - c|;
  5. the row filter      (bf16, bf16x3: both kernels, both tiles) lists exactly the allowed rows with the unfiltered call's bits;
  6. the query scale     fp16 kinds: the device's scale is the documented 2^(12 - e), the scaled norm in [2^11, 2^12).
Every test prints `SCANERR rung family d nq route n: max |S~ - exact| / eps_doc` (accumulate, swamp: also against the
accumulation term d 2^-23 sum |q_i p_i| alone); profiles/ip_scan_error.txt is that output.  Family `tiny` (bf16 kinds) is not
bounded but REFUSED: CONVDR_IP_RANGE from every entry, an error from FlatIPIndex.search, the oracle's answer from precision="auto"."""
import ctypes as C

import numpy as np
import pytest

from oracle import search as OS
from tests import scan_error_cases as SC
from tests.index_cases import torch_cuda      # noqa: F401 (the fixture, by name)

pytestmark = pytest.mark.gpu

OK, OVERFLOW, TOO_FEW, UNCERTAIN, RANGE = 0, 1, 2, 3, 4
NEG_INF_BITS = np.float32(-np.inf).view(np.int32)
K_BAND = 10
_BASE = {}


def _family(fam, rung, d):
    """the family's few queries and rows, computed once per (family, operand types, d) and never written to afterwards"""
    key = (fam, SC.kind(rung), SC.half_store(rung), d)
    if key not in _BASE:
        Q, P = SC.family(fam, rung, d, 1)
        Q.setflags(write=False), P.setflags(write=False)
        _BASE[key] = (Q, P)
    return _BASE[key]


def _index(rung, d, rows):
    from convdr_amd.search import FlatIPIndex
    storage, precision, _, _ = SC.RUNGS[rung]
    idx = FlatIPIndex(d, storage=storage, precision=precision, prepin=False)
    idx.add(rows.astype(np.float16) if storage == "fp16" else rows)
    if SC.split(rung) and storage == "fp32":
        idx._ensure_lo()
    return idx


def _raw(torch, idx, rung, q, k, tau_in, cap, fused=0, deep=False, allowed=None):
    """One raw call of the index's top-k entry on a workspace of its own (the pattern of test_ip_certificate_gpu._raw).  Returns
    (status, tau_retry bits, hits, band, ws): the last three shallow only."""
    from convdr_amd import _lib
    L = _lib.lib()
    nq, n = int(q.shape[0]), idx.ntotal
    need = (L.convdr_ip_deep_workspace_bytes if deep else L.convdr_ip_workspace_bytes)(nq, n, idx.d, k, cap)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    Dv = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    Iv = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    st = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
    tr = torch.zeros(nq, dtype=torch.float32, device="cuda")
    assert L.convdr_set_option(b"ip_fused_finish", fused) == 0
    try:
        idx._search_call(q, nq, idx._p32, idx._pbf, idx._plo, n, k, tau_in, cap, 0, ws, Dv, Iv, st, tr, SC.split(rung), deep, allowed)
        torch.cuda.synchronize()
    finally:
        assert L.convdr_set_option(b"ip_fused_finish", 1) == 0
    dbg = [None, None]
    if not deep:
        for i, fn in enumerate((L.convdr_ip_debug_counts, L.convdr_ip_debug_band)):
            off = fn(_lib.ptr(ws), nq, n, idx.d, k, cap) - ws.data_ptr()
            dbg[i] = ws[off:off + 4 * nq].view(torch.int32).cpu().numpy()
    return st.cpu().numpy(), tr.cpu().numpy().view(np.int32), dbg[0], dbg[1], ws


def _list(torch, ws, nq, n, d, k, cap):
    """(ids int64 [nq, cap], scan scores fp32 [nq, cap]) of the call that last used ws"""
    from convdr_amd import _lib
    pi, ps = C.c_void_p(), C.c_void_p()
    assert _lib.lib().convdr_ip_debug_list(_lib.ptr(ws), nq, n, d, k, cap, C.byref(pi), C.byref(ps)) == 0
    out = []
    for p, dt in ((pi, torch.int32), (ps, torch.float32)):
        off = p.value - ws.data_ptr()
        assert 0 <= off and off + 4 * nq * cap <= ws.numel()
        out.append(ws[off:off + 4 * nq * cap].view(dt).view(nq, cap).cpu().numpy())
    return out[0].astype(np.int64), out[1]


def _sample(torch, ws, nq, n, d, k, cap):
    """the threshold sample as [rows of the scanned tiles, nq] fp32, or None"""
    from convdr_amd import _lib
    pT, ld = C.c_void_p(), C.c_int64()
    assert _lib.lib().convdr_ip_debug_sample(_lib.ptr(ws), nq, n, d, k, cap, C.byref(pT), C.byref(ld)) == 0
    if pT.value is None:
        return None
    rows = (n + 255) // 256 * 256
    off = pT.value - ws.data_ptr()
    assert 0 <= off and off + 4 * rows * ld.value <= ws.numel() and ld.value >= nq
    return ws[off:off + 4 * rows * ld.value].view(torch.float32).view(rows, ld.value)[:, :nq].cpu().numpy()


def _scan_scores_from_list(ids, s, band, n, what):
    """assertion 1, and S~ [nq, n] in row order"""
    assert (band == n).all(), (what, "band sizes", band, n)
    head = ids[:, :n]
    order = np.argsort(head, axis=1, kind="stable")
    listed = np.take_along_axis(head, order, axis=1)
    assert (listed == np.arange(n)[None, :]).all(), (what, "rows listed more than once, missing, or past n")
    return np.take_along_axis(s[:, :n], order, axis=1)


def _reference(rung, idx, Qe, rows):
    """(exact [nq, n], eps_doc [nq], Qs, Ps, qs, ps, max |p - c|): the index's centre and scale read as data"""
    centre = None if idx._centre is None else idx._centre.cpu().numpy()
    ps = float(idx._scale) if SC.kind(rung) == "f16" else 1.0
    qs = SC.query_scale(rung, Qe)
    exact, Qs, Ps = SC.exact_scores(Qe, rows, centre, qs, ps)
    pmu = float(SC.norms(Ps).max()) / ps
    return exact, SC.eps_doc(rung, rows.shape[1], SC.norms(Qs), ps * pmu), Qs, Ps, qs, ps, pmu


def _hold(rung, fam, d, nq, route, n, S, exact, eps, Qs, Ps):
    """assertion 2 with the worst pair reported, and the printed measurement"""
    err = np.abs(S.astype(np.float64) - exact)
    ratio = err / eps[:, None]
    j, r = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    line = "SCANERR %-7s %-11s d=%-4d nq=%-3d %-6s n=%-4d max |S~ - exact| / eps_doc = %.4f" % (rung, fam, d, nq, route, n, ratio[j, r])
    if fam in ("accumulate", "swamp"):
        line += "   / (d 2^-23 sum |q_i p_i|) = %.4f" % float((err / SC.accumulation_term(d, Qs, Ps)).max())
    print(line)
    assert np.isfinite(S).all() and ratio[j, r] <= 1.0, \
        "%s %s d=%d nq=%d %s n=%d: query %d row %d: S~ = %r, exact = %r, |error| = %.6g = %.4f eps_doc (%.6g)" % (
            rung, fam, d, nq, route, n, j, r, float(S[j, r]), exact[j, r], err[j, r], ratio[j, r], eps[j])


def _hold_norms(rung, idx, pmu, Qs, qs, Qe, fam, S, exact):
    """assertions 4 and 6"""
    got = float(idx._max_norm.item())
    assert pmu <= got <= pmu * (1 + 1e-5), (rung, fam, "max norm", got, pmu)
    if SC.kind(rung) != "f16":
        return
    assert SC.away_from_a_power_of_two(SC.norms(Qe)), (rung, fam)
    qn = SC.norms(Qs)
    assert ((qn >= 2.0 ** 11) & (qn < 2.0 ** 12)).all(), (rung, fam, qn)        # NOT [2^12, 2^13): that is the block's interval
    if fam == "aligned":
        # the device's own scale: S~ / (unscaled exact) on the rows each query is parallel to, where |exact| = qn pm >> eps
        own = np.abs(exact) >= 0.999 * np.abs(exact).max(axis=1, keepdims=True)
        dev = (S.astype(np.float64) / (exact / qs[:, None]))[own]
        want = np.broadcast_to(qs[:, None], exact.shape)[own]
        assert (np.abs(dev / want - 1) < 0.01).all(), (rung, "query scale on the device", dev[:4], want[:4])


def _hold_band(torch, rung, fam, idx, q, S, exact, eps, cap):
    """assertion 3; returns how many queries came back UNCERTAIN as predicted and were held"""
    f32 = np.float32
    nq, n = S.shape
    kth = -np.sort(-exact, axis=1)[:, K_BAND - 1]
    tau = (kth - eps / 4).astype(f32)
    s10 = -np.sort(-S, axis=1)[:, K_BAND - 1]                                      # S~(k), fp32
    listed = (S >= tau[:, None]).sum(axis=1)
    # UNCERTAIN for certain: k rows are listed, and S~(k) - 2 eps is below tau already with the smallest admitted eps
    t64, s64 = tau.astype(np.float64), s10.astype(np.float64)
    sure = (listed >= K_BAND) & (s64 - 2 * eps < t64 - 1e-6 * (np.abs(t64) + np.abs(s64)))
    st, tr, hits, band, _ = _raw(torch, idx, rung, q, K_BAND, torch.tensor(tau, device="cuda"), cap, fused=0)
    assert (hits == listed).all(), (rung, fam, "hits", hits, listed)               # the second scan's scores are the first's
    assert (st[sure] == UNCERTAIN).all() and (st[listed < K_BAND] == TOO_FEW).all(), (rung, fam, st, listed)
    retry = tr.view(f32)
    with np.errstate(over="ignore"):
        e_lo = eps.astype(f32)
        e_lo = np.where(e_lo.astype(np.float64) > eps, np.nextafter(e_lo, f32(0)), e_lo)                   # <= eps_doc
        e_hi = (1.003 * eps).astype(f32)
        e_hi = np.where(e_hi.astype(np.float64) < 1.003 * eps, np.nextafter(e_hi, f32(np.inf)), e_hi)      # >= 1.003 eps_doc
        top = np.nextafter((s10 - f32(2) * e_lo).astype(f32), f32(-np.inf))       # tau_retry of eps_lib = eps_doc ...
        bot = np.nextafter((s10 - f32(2) * e_hi).astype(f32), f32(-np.inf))       # ... and of 1.003 eps_doc
    for j in np.flatnonzero(sure):
        assert bot[j] <= retry[j] <= top[j], \
            "%s %s query %d: tau_retry = %r gives eps_lib = %.8g, eps_doc = %.8g (ratio %.6f, allowed [1, 1.003])" % (
                rung, fam, j, float(retry[j]), (float(s10[j]) - float(retry[j])) / 2, eps[j], (float(s10[j]) - float(retry[j])) / 2 / eps[j])
    return int(sure.sum())


def _run_case(torch, rung, d, nq, route, n):
    cap, k = (8192, n) if route == "list" else (1024, K_BAND)
    held = 0
    for fam in SC.families_of(rung):
        Q, P = _family(fam, rung, d)
        Qe, rows = SC.expand(fam, Q, P, nq, n)
        idx = _index(rung, d, rows)
        q = torch.tensor(Qe, device="cuda")
        what = (rung, fam, d, nq, route, n)
        st, tr, hits, band, ws = _raw(torch, idx, rung, q, k, None, cap, fused=0)
        if route == "list":
            assert (st == OK).all(), (what, st)           # (the sample route's verdict depends on the threshold estimate: not held)
            assert (hits == (n + 255) // 256 * 256).all(), (what, hits)
            assert _sample(torch, ws, nq, n, d, k, cap) is None
            ids, s = _list(torch, ws, nq, n, d, k, cap)
            S = _scan_scores_from_list(ids, s, band, n, what)
        else:
            T = _sample(torch, ws, nq, n, d, k, cap)
            assert T is not None and T.shape[0] == (n + 255) // 256 * 256 and (T[n:] == -np.inf).all(), what
            S = np.ascontiguousarray(T[:n].T)
        exact, eps, Qs, Ps, qs, ps, pmu = _reference(rung, idx, Qe, rows)
        _hold(rung, fam, d, nq, route, n, S, exact, eps, Qs, Ps)
        _hold_norms(rung, idx, pmu, Qs, qs, Qe, fam, S, exact)
        if route == "list":
            got = _hold_band(torch, rung, fam, idx, q, S, exact, eps, cap)
            held += got
            assert fam != "random" or got >= nq // 2, (what, "queries whose band was held", got)
        if fam == "subnormal16":
            follow = np.flatnonzero((Qs[:, :2] == 0).all(axis=1) & (np.arange(nq) < 4))
            centre = None if idx._centre is None else idx._centre.cpu().numpy()
            grad = SC.model_scores(rung, Qe, rows, centre, qs, ps)[follow, 2 * follow]
            flsh = SC.model_scores(rung, Qe, rows, centre, qs, ps, flush=True)[follow, 2 * follow]
            dev = S[follow, 2 * follow].astype(np.float64)
            print("SCANERR %-7s subnormal16 d=%-4d nq=%-3d %-6s n=%-4d subnormal fp16 inputs: the device matches the %s model "
                  "(|S~ - gradual| = %.3g, |S~ - flushed| = %.3g, |gradual| = %.3g)" % (
                      rung, d, nq, route, n, "GRADUAL" if np.abs(dev - grad).max() < np.abs(dev - flsh).max() else "FLUSHED",
                      np.abs(dev - grad).max(), np.abs(dev - flsh).max(), np.abs(grad).max()))
    if route == "list":
        assert held > 0


@pytest.mark.parametrize("nq", [5, 130])
@pytest.mark.parametrize("d", [64, 768])
@pytest.mark.parametrize("rung", list(SC.RUNGS))
def test_list_route_scores_are_inside_the_band(torch_cuda, rung, d, nq):
    for n in (1024, 1000):
        _run_case(torch_cuda, rung, d, nq, "list", n)


@pytest.mark.parametrize("rung", list(SC.RUNGS))
def test_widest_rows_are_inside_the_band(torch_cuda, rung):
    """d = 4096, the entry's maximum: the accumulation term d 2^-23 is at its largest (with 5 queries: IP_TILE_TALL only)"""
    for n in (1024, 1000):
        _run_case(torch_cuda, rung, 4096, 5, "list", n)


@pytest.mark.parametrize("rung", list(SC.RUNGS))
def test_sample_route_scores_are_inside_the_band(torch_cuda, rung):
    """cap < n <= 32,768: the threshold pass (IP_MODE_FULL) scores the whole block; its sample is held to the same bound"""
    _run_case(torch_cuda, rung, 768, 5, "sample", 1280)


@pytest.mark.parametrize("nq", [5, 130])
@pytest.mark.parametrize("rung", ["bf16", "bf16x3"])
def test_row_filter_acts_on_finished_accumulators(torch_cuda, rung, nq):
    """A filter that drops every third row: the listed rows are exactly the allowed ones, and their scan scores are BIT-equal to
    the unfiltered call's (the filter masks accumulators after the main loop; it changes no operand and no order of summation)."""
    torch = torch_cuda
    d, n, cap = 768, 1024, 8192
    Q, P = _family("random", rung, d)
    Qe, rows = SC.expand("random", Q, P, nq, n)
    idx = _index(rung, d, rows)
    q = torch.tensor(Qe, device="cuda")
    st, _, _, band, ws = _raw(torch, idx, rung, q, n, None, cap, fused=0)
    ids, s = _list(torch, ws, nq, n, d, n, cap)
    S = _scan_scores_from_list(ids, s, band, n, (rung, nq, "unfiltered"))
    allow = np.arange(n) % 3 != 0
    f = idx.row_filter(allow)
    m = int(allow.sum())
    st, _, hits, band, ws = _raw(torch, idx, rung, q, n, None, cap, fused=0, allowed=f)
    assert (st == OK).all() and (hits == m).all() and (band == m).all(), (st, hits, band, m)
    ids, s = _list(torch, ws, nq, n, d, n, cap)
    order = np.argsort(ids[:, :m], axis=1, kind="stable")
    listed = np.take_along_axis(ids[:, :m], order, axis=1)
    assert (listed == np.flatnonzero(allow)[None, :]).all()
    got = np.take_along_axis(s[:, :m], order, axis=1)
    np.testing.assert_array_equal(got.view(np.int32), S[:, allow].view(np.int32))


def _tiny_block(rung, nq, n):
    Q, P = _family("tiny", rung, 64)
    return SC.expand("tiny", Q, P, nq, n)


@pytest.mark.parametrize("rung", ["bf16", "bf16x3"])
def test_tiny_norms_are_refused_by_every_entry(torch_cuda, rung):
    """Norms below 2^-60 (family `tiny`: where the CPU model exceeds eps_doc): CONVDR_IP_RANGE with tau_retry = -inf from the
    three cut kernels, RANGE from the range, rank-rows and rank-docs entries, ConvdrError from FlatIPIndex.search.  The raw list
    still holds the scan's scores: what the device does with bf16 subnormals is printed against the CPU models.  A block of
    ordinary rows: a tiny query alone is refused, an ordinary and an all-zero query beside it are certified."""
    torch = torch_cuda
    from convdr_amd import _lib
    from convdr_amd.search import FlatIPIndex
    d, n, nq = 64, 64, 8
    Qe, rows = _tiny_block(rung, nq, n)
    idx = FlatIPIndex(d, precision=SC.RUNGS[rung][1], prepin=False)
    idx.add(rows, ids=np.arange(n, dtype=np.int64) // 3)
    if SC.split(rung):
        idx._ensure_lo()
    assert 0 < float(idx._max_norm.item()) < SC.NORM_FLOOR
    q = torch.tensor(Qe, device="cuda")
    for kw in (dict(cap=1024, fused=1), dict(cap=1024, fused=0), dict(cap=16384, deep=True)):
        st, tr, *_ = _raw(torch, idx, rung, q, K_BAND, None, **kw)
        assert (st == RANGE).all() and (tr == NEG_INF_BITS).all(), (kw, st, tr.view(np.float32))
    # what the device made of the subnormal operands (a measurement: no score of a refused query is used for anything)
    st, _, _, band, ws = _raw(torch, idx, rung, q, n, None, 1024, fused=0)
    ids, s = _list(torch, ws, nq, n, d, n, 1024)
    if (band == n).all():
        S = _scan_scores_from_list(ids, s, band, n, (rung, "tiny")).astype(np.float64)
        exact, eps, Qs, Ps, qs, ps, pmu = _reference(rung, idx, Qe, rows)
        model = SC.model_scores(rung, Qe, rows, None if idx._centre is None else idx._centre.cpu().numpy(), qs, ps)
        for j in range(4):          # query j against its own row 2 j, held to the bound of THAT pair's norms (as the CPU test does)
            e = float(SC.eps_doc(rung, d, SC.norms(Qe[j:j + 1])[0], SC.norms(rows[2 * j:2 * j + 1])[0]))
            print("SCANERR %-7s tiny        pair %d: |S~ - exact| / eps_doc(pair) = %.3f, operand-rounding model (gradual subnormals): %.3f; "
                  "S~ = %.9g, model = %.9g, exact = %.9g" % (rung, j, abs(S[j, 2 * j] - exact[j, 2 * j]) / e,
                                                           abs(model[j, 2 * j] - exact[j, 2 * j]) / e, S[j, 2 * j], model[j, 2 * j], exact[j, 2 * j]))
    L, ptr = _lib.lib(), _lib.ptr
    store, r32, r16, scale, centre = idx._operands()
    assert store == 0
    cap = 4096
    need = L.convdr_ip_range_workspace_bytes(nq, n, d, cap)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rad = torch.zeros(nq, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(nq, dtype=torch.int64, device="cuda")
    lims = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    st = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
    _lib.check(L.convdr_ip_range_search(store, ptr(q), nq, r32, r16, scale, centre, n, d, ptr(idx._max_norm), ptr(rad), cap, 0, None, 0,
                                        ptr(ws), need, ptr(cnt), ptr(lims), ptr(st), _lib.stream_ptr()), "convdr_ip_range_search")
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == RANGE).all() and int(lims[-1].item()) == 0
    o = idx.doc_ordinals()
    tgt = torch.arange(nq, dtype=torch.int64, device="cuda") * 7
    for docs in (False, True):
        need = (L.convdr_ip_rank_docs_workspace_bytes(nq, n, d, cap, o.ndocs) if docs else L.convdr_ip_rank_workspace_bytes(nq, n, d, cap))
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        rank = torch.zeros(nq, dtype=torch.int64, device="cuda")
        X = torch.zeros(nq, dtype=torch.float64, device="cuda")
        cnt = torch.zeros(nq, dtype=torch.int64, device="cuda")
        above = torch.zeros(nq, dtype=torch.int64, device="cuda")
        st = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
        head = (store, ptr(q), nq, ptr(tgt), r32, r16, scale, centre, n, d, ptr(idx._max_norm), None, 0, 0)
        tail = (cap, ptr(ws), need, ptr(rank), ptr(X), ptr(cnt), ptr(above), ptr(st), _lib.stream_ptr())
        if docs:
            _lib.check(L.convdr_ip_rank_docs(*head, ptr(o.ord), o.ndocs, *tail), "convdr_ip_rank_docs")
        else:
            _lib.check(L.convdr_ip_rank_rows(*head, *tail), "convdr_ip_rank_rows")
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == RANGE).all() and (rank.cpu().numpy() == -1).all(), (docs, st, rank)
    # the Python entries end loudly, naming the cause and the remedy
    for call in (lambda: idx.search(Qe, 5), lambda: idx.range_search(Qe, np.zeros(nq, np.float32)),
                 lambda: idx.rank_rows(Qe, np.arange(nq, dtype=np.int64))):
        with pytest.raises(_lib.ConvdrError, match='2\\^-60.*precision="auto"'):
            call()
    # an ordinary block: the floor is per query, and a zero norm stays in range
    Qn, Pn = _family("random", rung, d)
    _, rows_n = SC.expand("random", Qn, Pn, 1, n)
    idx2 = _index(rung, d, rows_n)
    q3 = np.stack([Qe[3], Qn[0], np.zeros(d, np.float32)])                         # norm 2.7e-22, ordinary, zero
    st, tr, *_ = _raw(torch, idx2, rung, torch.tensor(q3, device="cuda"), K_BAND, None, 1024, fused=1)
    assert st.tolist() == [RANGE, OK, OK], st
    st, tr, *_ = _raw(torch, idx2, rung, torch.tensor(q3, device="cuda"), K_BAND, None, 1024, fused=0)
    assert st.tolist() == [RANGE, OK, OK], st


def test_tiny_norms_are_searched_exactly_by_the_rescaling_scan(torch_cuda):
    """the remedy the error names: the same data on a precision="auto" index (fp16 scan: both operands rescaled) returns the oracle's top-k"""
    from convdr_amd.search import FlatIPIndex
    Qe, rows = _tiny_block("bf16", 8, 64)
    idx = FlatIPIndex(64, precision="auto", prepin=False)
    idx.add(rows)
    D, I = idx.search(Qe, 5)
    Dr, Ir = OS.flat_ip_search(Qe, rows, 5)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)
