"""Inputs, reference and bound of the scan-error tests (test_scan_error_cpu.py, test_scan_error_gpu.py): is every raw scan
score S~ within the certificate's eps of the exact scaled score (csrc/ip_certify.hpp: IpBand::eps "bounds |S~ - exact scaled
score| for every row of the block")?

The reference is the plain one: from the fp32 inputs, in fp64,  exact = qs ps sum_i q_i (p_i - c_i)  with c the index's stored
centre (read as data), ps its power-of-two scale (1 for bf16) and qs the per-query power of two of k_rows_to_half<F16, true>
(`query_scale`, written from the rule in csrc/ip_prepare.hpp; 1 for bf16).  The bound is written out from the formulas in the
comment above ip_eps_coef (csrc/ip_topk.hip), WITHOUT the library's 1.0001 / 1.001 safety factors and without its + 1e-30:
    eps_doc = coef qn pm + abs (qn + pm) + abs^2,      qn = qs |q|, pm = ps max_r |p_r - c|   (exact fp64 norms, scan units).

Families: functions of (rung, d, seed) that return a few queries and a few rows; every magnitude is set by powers of two, and
`expand` turns them into a block: row 2j = base row j mod m, row 2j + 1 = its negation, so that the column sums are exactly
zero after every pair and the index centres by exactly 0 (family `offset` adds a common vector: there the centring does the
work).  Nothing here touches a GPU."""
import numpy as np

# name, storage, precision, kind, split (the query's -- and, with a remainder copy, the rows' -- remainders are operands)
RUNGS = {
    "bf16": ("fp32", "bf16", "bf16", False),
    "bf16x3": ("fp32", "bf16x3", "bf16", True),
    "fp16": ("fp32", "fp16", "f16", False),
    "fp16x3": ("fp32", "fp16x3", "f16", True),
    "h16": ("fp16", "fp16", "f16", False),        # the half store, one pass: the rows ARE halves
    "h16x2": ("fp16", "fp16x2", "f16", True),     # the half store, two passes: P Qh + P Ql
}
ETA = 2.0 ** -14                # csrc/ip_topk.hip: IP_F16_ETA
NORM_FLOOR = 2.0 ** -60         # csrc/ip_topk.hip: IP_BF16_NORM_FLOOR
NORM_LIMIT = 60000.0            # csrc/ip_topk.hip: IP_F16_NORM_LIMIT
FAMILIES = ("random", "aligned", "accumulate", "swamp", "cancel", "offset", "subnormal16")     # + "tiny": refused, not bounded


def kind(rung):
    return RUNGS[rung][2]


def split(rung):
    return RUNGS[rung][3]


def half_store(rung):
    return RUNGS[rung][0] == "fp16"


def unit(rung):
    """u: the relative error of one rounding to the rung's 16-bit type"""
    return 2.0 ** -11 if kind(rung) == "f16" else 2.0 ** -8


def coefficients(rung, d):
    """(coef, abs) of the ip_topk.hip comment, no safety factor.  The half store uses the fp16 scan's, unchanged."""
    u, acc = unit(rung), d / 8388608.0
    coef = 3 * u * u * (1 + 2 * u) + 3 * acc if split(rung) else 2 * u + u * u + acc
    ab = 0.0
    if kind(rung) == "f16":
        ab = (2.0 if split(rung) else 1.0) * ETA * (1 + 2.0 ** -11) * np.sqrt(float(d))
    return coef, ab


def eps_doc(rung, d, qn, pm):
    """qn [nq] and pm (scalar) in scan units, exact fp64"""
    coef, ab = coefficients(rung, d)
    return coef * qn * pm + ab * (qn + pm) + ab * ab


def accumulation_term(d, Qs, Ps):
    """d 2^-23 sum_i |q_i p_i| per (query, row), operands in scan units: what the bound charges the fp32 accumulation of one chain"""
    return d * 2.0 ** -23 * (np.abs(Qs) @ np.abs(Ps).T)


def bf16_out_of_range(qn, pm):
    """IpBand::out_of_range of the bf16 kinds: a NON-ZERO norm below the floor (a zero norm stays in range: the score is exactly 0)"""
    return bool((0.0 < pm < NORM_FLOOR) or (0.0 < qn < NORM_FLOOR))


# ---- the rules the reference needs -----------------------------------------------------------------------------------------
def norms(X):
    return np.sqrt((np.asarray(X, np.float64) ** 2).sum(axis=1))


def query_scale(rung, Q):
    """[nq] the power of two each query is multiplied by: 2^(12 - e) with fl32(|q|) = m 2^e, m in [0.5, 1) (clamped to 2^+-100;
    1 for a zero or non-finite norm, and for the bf16 kinds)"""
    if kind(rung) != "f16":
        return np.ones(len(Q))
    nm = norms(Q).astype(np.float32)
    _, ex = np.frexp(nm)
    sh = np.clip(12 - ex.astype(np.int64), -100, 100)
    return np.where((nm > 0) & np.isfinite(nm), np.ldexp(1.0, sh), 1.0)


def block_scale(rung, pm_unscaled):
    """convdr_ip_f16_scale, and the half store's max(1, .): the CPU tests' copy -- the GPU test reads idx._scale as data"""
    if kind(rung) != "f16" or not pm_unscaled > 0:
        return 1.0
    _, ex = np.frexp(np.float32(pm_unscaled * (1 + 1e-6)))
    s = float(np.ldexp(1.0, int(np.clip(13 - int(ex), -100, 100))))
    return max(1.0, s) if half_store(rung) else s


def away_from_a_power_of_two(x, margin=0.01):
    """every x at least `margin` (relative) away from the powers of two on both sides: frexp mantissa in [0.5 (1 + m), 1 - m / 2]"""
    m, _ = np.frexp(np.asarray(x, np.float64))
    return bool(((m >= 0.5 * (1 + margin)) & (m <= 1 - margin / 2)).all())


def exact_scores(Q, P, centre, qs, ps):
    """[nq, n] fp64: qs ps sum q_i (p_i - c_i); and the operands in scan units (fp64)"""
    V = np.asarray(P, np.float64) - (0.0 if centre is None else np.asarray(centre, np.float64))
    Qs, Ps = np.asarray(Q, np.float64) * np.asarray(qs, np.float64)[:, None], V * float(ps)
    return Qs @ Ps.T, Qs, Ps


# ---- the operand-rounding model: round to nearest even to the 16-bit type, fp64 sums ---------------------------------------------
def bf16(x):
    """fp32 -> bf16 -> fp32, round to nearest even on the integer pattern (finite inputs; bf16 subnormals come out gradual)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)


def to16(rung, x32, flush=False):
    """fp32 -> the rung's 16-bit type -> fp64.  flush: fp16 subnormal results (|x| < 2^-14) become 0 (an MFMA that flushes its inputs)"""
    if kind(rung) != "f16":
        return bf16(x32).astype(np.float64)
    with np.errstate(over="ignore", under="ignore"):
        h = np.asarray(x32, np.float32).astype(np.float16).astype(np.float64)
    return np.where(np.abs(h) < ETA, 0.0, h) if flush else h


def model_scores(rung, Q, P, centre, qs, ps, flush=False):
    """The scan but for its fp32 accumulation: the operands as k_rows_to_half / the half store make them (fp32 arithmetic, one
    rounding to 16 bits, remainders where the rung has them), every product and sum in fp64.  [nq, n] in scan units."""
    f32 = np.float32
    Qs = (np.asarray(Q, f32) * np.asarray(qs, np.float64).astype(f32)[:, None]).astype(f32)            # exact: a power of two
    V = np.asarray(P, f32) if centre is None else (np.asarray(P, f32) - np.asarray(centre, f32)).astype(f32)
    Vs = (V * f32(ps)).astype(f32)
    qh = to16(rung, Qs, flush)
    ql = to16(rung, (Qs - qh.astype(f32)).astype(f32), flush)
    ph = to16(rung, Vs, flush)
    if not split(rung):
        return qh @ ph.T
    if half_store(rung):
        return qh @ ph.T + ql @ ph.T                                                                    # P Qh + P Ql
    pl = to16(rung, (Vs - ph.astype(f32)).astype(f32), flush)
    return qh @ ph.T + qh @ pl.T + ql @ ph.T                                                            # hi hi + hi lo + lo hi


# ---- the families ----------------------------------------------------------------------------------------------------------
def _exact16(rung, rs, shape, spread):
    """values with all of the 16-bit type's significant bits set at random (an odd integer of 8 / 11 bits) times 2^-r, r in
    [0, spread): exactly representable, so the operands carry no error"""
    t = 11 if kind(rung) == "f16" else 8
    m = rs.randint(1 << (t - 1), 1 << t, size=shape) | 1
    return np.ldexp(m.astype(np.float64), -(t - 1) - rs.randint(0, spread, size=shape)).astype(np.float32)


def _queries_off_powers(make, count):
    """`count` queries from make(j, attempt), each re-drawn until its norm is 1 % away from a power of two (qs is then unambiguous)"""
    out = []
    for j in range(count):
        for attempt in range(64):
            q = make(j, attempt)
            if away_from_a_power_of_two(norms(q[None])):
                break
        else:
            raise AssertionError("no query norm away from a power of two")
        out.append(q)
    return np.stack(out).astype(np.float32)


def family(name, rung, d, seed):
    """(Q [a few, d], P [a few, d]) fp32; P of the half-store rungs holds halves (widened).  `offset` returns rows that already
    contain the common vector; expand() pairs them about it."""
    rs = np.random.RandomState(seed * 7919 + d)
    u = unit(rung)
    f32 = np.float32
    sign = lambda shape: rs.choice(np.asarray([-1.0, 1.0], f32), size=shape)
    if name == "random":
        P = rs.standard_normal((64, d)).astype(f32)
        Q = _queries_off_powers(lambda j, a: np.random.RandomState(seed * 31 + j * 64 + a).standard_normal(d).astype(f32), 8)
    elif name == "aligned":
        # q || p, every element (1 + u (1 - 2^-10)) 2^e: each operand rounds DOWN by almost a full u, no error cancels.  e = i mod 2
        # keeps |q| = sqrt(2.5 d) (1 + u') 2^e' away from the powers of two.
        base = (1.0 + u * (1.0 - 2.0 ** -10)) * np.ldexp(1.0, np.arange(d) % 2)
        P = np.stack([base * sign(d) for _ in range(4)]).astype(f32)
        Q = np.concatenate([P * f32(2.0 ** 3), -P * f32(2.0 ** -5)]).astype(f32)
    elif name == "accumulate":
        # zero operand error, every product positive with 16 / 22 significant bits, exponents spread over 14 binades: every fp32
        # partial sum must round.  What the device does with them is the unmeasured part.
        s = sign((1, d))
        P = _exact16(rung, rs, (16, d), 7) * s
        Q = _queries_off_powers(lambda j, a: _exact16(rung, np.random.RandomState(seed * 37 + j * 64 + a), (d,), 7) * s[0], 6)
    elif name == "swamp":
        # one product 2^20 times the others, at K position 0, in the middle and at d - 1 (1.5 * 2^10 on either side); every operand
        # exactly representable, so that what is measured is the accumulation alone: the small products against the large sum
        pos = [0, d // 2, d - 1]
        P = _exact16(rung, rs, (3, d), 1) * sign((3, d))
        Q = _exact16(rung, rs, (3, d), 1) * sign((3, d))
        for j, c in enumerate(pos):
            P[j, c] = f32(1536.0) * np.sign(P[j, c])
            Q[j, c] = f32(1536.0) * np.sign(Q[j, c])
        assert away_from_a_power_of_two(norms(Q))
    elif name == "cancel":
        # q _|_ p exactly: coordinate pairs (a, b) against 2^7 (b, -a); each query is orthogonal to its own row only
        def turned(p):
            q = np.empty_like(p)
            q[..., 0::2], q[..., 1::2] = p[..., 1::2] * f32(128.0), -p[..., 0::2] * f32(128.0)
            return q
        Q = _queries_off_powers(lambda j, a: turned(np.random.RandomState(seed * 47 + j * 64 + a).standard_normal(d).astype(f32)), 6)
        P = -turned(Q) * f32(2.0 ** -14)                                   # turning twice negates: the rows the queries came from
    elif name == "offset":
        # rows c + v with |c| = 100 and |v| ~ 1 (every element of c is +-100 / sqrt(d)), each with its mirror image c - v
        c = (sign(d) * f32(100.0 / np.sqrt(d))).astype(f32)
        v = (rs.standard_normal((32, d)) / np.sqrt(d)).astype(f32)
        P = (c + v).astype(f32)
        P = np.concatenate([P, (c - (P - c)).astype(f32)])                # the mirror images about c, row j + 32 (fp32 arithmetic)
        Q = _queries_off_powers(lambda j, a: np.random.RandomState(seed * 41 + j * 64 + a).standard_normal(d).astype(f32), 6)
    elif name == "subnormal16":
        # fp16 kinds, written in SCALED units (the block's scale comes out as 1): one dominant coordinate carries the norm
        # (1.5 * 2^12: into [2^12, 2^13)), every other one lies in [2^-24, 2^-14), below the halves' normal range.  Queries: four
        # that are zero on the dominant coordinates and follow the signs of row j elsewhere (a flushed input then loses
        # sum |q_i p_i| coherently), and four Gaussian ones.
        assert kind(rung) == "f16"
        small = lambda shape: np.ldexp(1.0 + rs.rand(*shape), rs.randint(-24, -14, size=shape)).astype(f32)
        P = small((8, d)) * sign((8, d))
        dom = np.arange(8) % 2
        P[np.arange(8), dom] = f32(6144.0) * sign(8)
        def follower(j, a):
            q = np.sign(P[j]) * (1.0 + np.random.RandomState(seed * 53 + j * 64 + a).rand(d)).astype(f32) * f32(256.0)
            q[:2] = 0
            return q
        A = _queries_off_powers(follower, 4)
        G = _queries_off_powers(lambda j, a: np.random.RandomState(seed * 43 + j * 64 + a).standard_normal(d).astype(f32) * f32(64.0), 4)
        Q = np.concatenate([A, G]).astype(f32)
    elif name == "tiny":
        # bf16 kinds: what the relative-only bound cannot cover (rows A, B, C: the first construction at three magnitudes; row D
        # and query D: the second)
        assert kind(rung) == "bf16" and d == 64
        rowsA = [np.ldexp(1.0 + rs.rand(d), e).astype(f32) * sign(d) for e in (-129, -131, -132)]       # fp32 subnormals
        err = [np.sign(r.astype(np.float64) - bf16(r).astype(np.float64)) for r in rowsA]
        qA = [(np.where(e == 0, 1.0, e) * 2.0 ** 40).astype(f32) for e in err]                           # signs follow the row's rounding errors
        el = lambda: bf16((3e-23 * (1.0 + 0.25 * rs.rand(d))).astype(f32))                               # exactly representable: zero operand error
        P = np.stack(rowsA + [el()]).astype(f32)
        Q = np.stack(qA + [el()]).astype(f32)
    else:
        raise KeyError(name)
    if half_store(rung) and name != "tiny":
        with np.errstate(under="ignore"):
            P = P.astype(np.float16).astype(f32)          # the passages ARE these halves
    return Q, P


def offset_centre(P):
    """the common vector of the `offset` rows, recovered as the mean of a row and its mirror image (the test reads idx._centre instead)"""
    m = len(P) // 2
    return ((P[:m].astype(np.float64) + P[m:].astype(np.float64)) / 2).mean(axis=0)


def expand(name, Q, P, nq, n):
    """The block and the queries of one case: n rows (n even) in +- pairs -- `offset`: a row and its mirror image --, nq queries
    cycling through Q with the sign flipped on every second cycle.  Both are exact operations on the family's values."""
    assert n % 2 == 0
    m = len(P) // 2 if name == "offset" else len(P)
    j = np.arange(n // 2) % m
    rows = np.empty((n, P.shape[1]), np.float32)
    rows[0::2] = P[j]
    rows[1::2] = P[j + m] if name == "offset" else -P[j]
    i = np.arange(nq)
    qq = Q[i % len(Q)] * np.where((i // len(Q)) % 2 == 1, np.float32(-1.0), np.float32(1.0))[:, None]
    return np.ascontiguousarray(qq, np.float32), rows


def families_of(rung):
    return [f for f in FAMILIES if f != "subnormal16" or kind(rung) == "f16"]
