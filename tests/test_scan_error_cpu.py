"""The inputs and the bound of the scan-error test, checked without a GPU (tests/scan_error_cases.py; the device's scores are held
to the same bound in test_scan_error_gpu.py).  What is asserted here, with the scan emulated by the operand-rounding model (round
to nearest even to the 16-bit type, fp64 sums -- everything but the fp32 accumulation):
  * every family stays inside eps_doc in the model, on every rung;
  * `aligned` reaches >= 0.95 of eps_doc on the one-pass rungs at d = 64: a coefficient tightened by more than a few per cent fails
    the GPU test's inequality;
  * `subnormal16` is covered whether the MFMA takes subnormal halves gradually or flushes them;
  * `tiny` EXCEEDS eps_doc on the bf16 kinds -- the recorded proof that their relative-only bound has a hole below the normal
    range -- and the norm floor (IP_BF16_NORM_FLOOR) refuses exactly those inputs;
  * the families are what they say: exact operands, positive products, one swamping product, exact orthogonality, query norms
    1 % away from a power of two, blocks that centre by exactly zero."""
import numpy as np
import pytest

from tests import scan_error_cases as C

WIDTHS = (64, 768)


def _centre_as_the_index_computes_it(rows):
    """k_colsum_f32 on fewer than 4,096 rows: one sequential fp32 sum per column, divided in fp64, rounded to fp32"""
    s = np.zeros(rows.shape[1], np.float32)
    for r in rows:
        s = (s + r).astype(np.float32)
    return (s.astype(np.float64) / len(rows)).astype(np.float32)


def _case(rung, d, fam, nq=5, n=64, seed=1):
    """(exact, model, flushed model, eps_doc [nq, 1], Qs, Ps, queries, rows, centre) of one expanded family, CPU only"""
    Q, P = C.family(fam, rung, d, seed)
    Qe, Pe = C.expand(fam, Q, P, nq, n)
    centre = None if C.half_store(rung) else _centre_as_the_index_computes_it(Pe)
    V = Pe.astype(np.float64) - (0.0 if centre is None else centre.astype(np.float64))
    pmu = float(C.norms(V).max())
    ps, qs = C.block_scale(rung, pmu), C.query_scale(rung, Qe)
    exact, Qs, Ps = C.exact_scores(Qe, Pe, centre, qs, ps)
    eps = C.eps_doc(rung, d, C.norms(Qs), ps * pmu)[:, None]
    model = C.model_scores(rung, Qe, Pe, centre, qs, ps)
    flushed = C.model_scores(rung, Qe, Pe, centre, qs, ps, flush=True)
    return exact, model, flushed, eps, Qs, Ps, Qe, Pe, centre


@pytest.mark.parametrize("rung", list(C.RUNGS))
def test_every_family_is_inside_the_bound_in_the_model(rung):
    for d in WIDTHS + (4096,):
        for fam in C.families_of(rung):
            exact, model, flushed, eps, Qs, Ps, Qe, Pe, centre = _case(rung, d, fam, nq=9, n=64)
            ratio = float((np.abs(model - exact) / eps).max())
            print("%-7s d=%-4d %-11s model / eps_doc = %.4f" % (rung, d, fam, ratio))
            assert ratio <= 1.0, (rung, d, fam, ratio)
            if C.kind(rung) == "f16":
                assert C.away_from_a_power_of_two(C.norms(Qe)), (rung, d, fam)      # qs is unambiguous
                qn = C.norms(Qs)
                assert ((qn >= 2.0 ** 11) & (qn < 2.0 ** 12)).all(), (rung, d, fam, qn)   # the documented interval of the scaled norm
                pm = C.norms(Ps).max()
                assert 2.0 ** 12 <= pm < 2.0 ** 13 or (C.half_store(rung) and pm < 2.0 ** 13), (rung, d, fam, pm)
            else:
                assert not C.bf16_out_of_range(C.norms(Qs).min(), C.norms(Ps).max())
            if fam != "offset" and centre is not None:
                assert not centre.any(), (rung, d, fam)                               # the +- pairs centre by exactly zero


@pytest.mark.parametrize("rung", ["bf16", "fp16"])
def test_aligned_reaches_the_bound_on_the_one_pass_rungs(rung):
    exact, model, _, eps, *_ = _case(rung, 64, "aligned", nq=8, n=8)
    ratio = np.abs(model - exact) / eps
    own = np.abs(exact) >= 0.999 * np.abs(exact).max(axis=1, keepdims=True)            # the rows each query is parallel to
    print(rung, "aligned: model / eps_doc =", float(ratio[own].min()), "..", float(ratio[own].max()))
    assert ratio[own].min() >= 0.95 and ratio.max() <= 1.0, (rung, ratio[own].min(), ratio.max())


@pytest.mark.parametrize("rung", [r for r in C.RUNGS if C.kind(r) == "f16"])
def test_subnormal_halves_are_covered_gradual_or_flushed(rung):
    for d in WIDTHS:
        exact, model, flushed, eps, Qs, Ps, *_ = _case(rung, d, "subnormal16", nq=8, n=16)
        small = (np.abs(Ps) < C.ETA) & (Ps != 0)
        assert small.sum(axis=1).min() >= d - 3 and (np.abs(Ps[small]) >= 2.0 ** -24).all()      # all but the dominant coordinate (and a half rounded up to 2^-14)
        assert float(C.norms(Ps).max()) == pytest.approx(6144.0, rel=1e-6)                      # written in scaled units: scale 1
        assert (np.abs(model - exact) <= eps).all() and (np.abs(flushed - exact) <= eps).all()
        # the two models differ on the queries that avoid the dominant coordinates: the GPU test can tell which one the device is
        follow = np.flatnonzero((Qs[:, :2] == 0).all(axis=1))
        assert len(follow) == 4
        # (against its own row, 2 j of the expanded block, such a query's products all have one sign; a few elements of
        #  [2^-15, 2^-14) round UP into the normal range and survive the flush)
        own_m, own_f = np.abs(model[follow, 2 * follow]), np.abs(flushed[follow, 2 * follow])
        assert (own_m > 0).all() and (own_f <= 0.25 * own_m).all(), (rung, d, own_m, own_f)


@pytest.mark.parametrize("rung", ["bf16", "bf16x3"])
def test_tiny_inputs_break_the_relative_bound_and_the_floor_refuses_them(rung):
    Q, P = C.family("tiny", rung, 64, 1)
    one = np.ones(1)
    worst = []
    for j in range(4):
        q, p = Q[j:j + 1], P[j:j + 1]
        exact, Qs, Ps = C.exact_scores(q, p, None, one, 1.0)
        qn, pm = float(C.norms(q)[0]), float(C.norms(p)[0])
        eps = float(C.eps_doc(rung, 64, qn, pm))
        model = float(C.model_scores(rung, q, p, None, one, 1.0)[0, 0])
        if j < 3:       # rows of bf16 SUBNORMALS against a long query that follows their rounding errors: operand rounding alone
            err = abs(model - exact[0, 0])
        else:           # exact operands whose products underflow: one fp32 rounding per product, fp64 sum
            assert (C.bf16(q) == q).all() and (C.bf16(p) == p).all()
            with np.errstate(under="ignore"):
                prod = (q[0] * p[0]).astype(np.float32)
            err = abs(float(prod.astype(np.float64).sum()) - exact[0, 0])
        worst.append(err / eps)
        assert err > eps, (rung, j, err, eps)                          # THE DEFECT: the documented bound does not hold here
        assert C.bf16_out_of_range(qn, pm), (rung, j, qn, pm)          # ... and the floor refuses the pair
    print(rung, "tiny: model error / eps_doc =", ["%.2f" % w for w in worst])
    if rung == "bf16":
        assert worst[0] < worst[1] < worst[2]                          # the deeper into the subnormals, the worse


def test_floor_arithmetic():
    f = C.NORM_FLOOR
    assert f == 2.0 ** -60 and np.float32(f) == f
    assert not C.bf16_out_of_range(1.0, 1.0)
    assert not C.bf16_out_of_range(f, f) and not C.bf16_out_of_range(1e30, f)            # the floor itself is in range
    below = float(np.nextafter(np.float32(f), np.float32(0)))
    assert C.bf16_out_of_range(below, 1.0) and C.bf16_out_of_range(1.0, below) and C.bf16_out_of_range(below, below)
    assert not C.bf16_out_of_range(0.0, 1.0) and not C.bf16_out_of_range(1.0, 0.0) and not C.bf16_out_of_range(0.0, 0.0)
    assert C.bf16_out_of_range(0.0, below) and C.bf16_out_of_range(1e-45, 1.0)           # zero excuses only itself
    # the derivation's margins at the widest admitted d: operand term sqrt(d) 2^-134 |q| against u |q| pm, product term d 2^-150
    # against d 2^-23 |q| pm
    d = 4096
    assert 2.0 ** -8 * f / (np.sqrt(d) * 2.0 ** -134) >= 2.0 ** 50
    assert 2.0 ** -23 * f * f / 2.0 ** -150 >= 2.0 ** 7


def test_the_families_are_what_they_say():
    for rung in C.RUNGS:
        for d in WIDTHS:
            # accumulate: no operand error, every product of one sign
            Q, P = C.family("accumulate", rung, d, 1)
            qs = C.query_scale(rung, Q)
            for X, s in ((Q, qs), (P, np.full(len(P), C.block_scale(rung, float(C.norms(P).max()))))):
                Xs = (X * s.astype(np.float32)[:, None]).astype(np.float32)
                assert (C.to16(rung, Xs) == Xs.astype(np.float64)).all(), (rung, d)
            assert (Q[:, None, :].astype(np.float64) * P[None, :, :] > 0).all(), (rung, d)
            # swamp: query j and row j share one product 2^20 times the largest other one (within the factor 4 of the (1, 2) draws)
            Q, P = C.family("swamp", rung, d, 1)
            assert (C.to16(rung, Q) == Q).all() and (C.to16(rung, P) == P).all(), (rung, d)        # exact operands
            for j, c in enumerate((0, d // 2, d - 1)):
                prod = np.abs(Q[j].astype(np.float64) * P[j])
                rest = np.delete(prod, c)
                assert prod.argmax() == c and 2.0 ** 19 <= prod[c] / rest.max() and prod[c] / rest.min() <= 2.0 ** 22, (rung, d, j)
            # cancel: every coordinate pair of a query against its own row cancels exactly
            Q, P = C.family("cancel", rung, d, 1)
            if not C.half_store(rung):
                prods = Q.astype(np.float64) * P.astype(np.float64)                     # exact: 48-bit products
                assert (prods[:, 0::2] + prods[:, 1::2] == 0).all() and (np.abs(prods) > 0).any(), (rung, d)
            # offset: the common vector is 100 times the rest
            Q, P = C.family("offset", rung, d, 1)
            c = C.offset_centre(P)
            ratio = np.linalg.norm(c) / C.norms(P.astype(np.float64) - c).max()
            assert 50 <= ratio <= 200, (rung, d, ratio)
            # aligned: each operand rounds by almost a full u, always toward zero
            Q, P = C.family("aligned", rung, d, 1)
            rel = (np.abs(P.astype(np.float64)) - np.abs(C.to16(rung, P))) / np.abs(P)
            if not C.half_store(rung):
                assert (rel > 0.99 * C.unit(rung)).all() and (rel < C.unit(rung)).all(), (rung, d)


def test_expand_keeps_pairs_and_fills_every_query():
    Q, P = C.family("random", "bf16", 64, 1)
    qq, rows = C.expand("random", Q, P, 130, 1000)
    assert qq.shape == (130, 64) and rows.shape == (1000, 64)
    assert (rows[0::2] == -rows[1::2]).all() and (rows[0:128:2] == P).all() and (rows[128:256:2] == P).all()
    assert (qq[:8] == Q).all() and (qq[8:16] == -Q).all() and (qq[16:24] == Q).all()
    assert not _centre_as_the_index_computes_it(rows).any()
