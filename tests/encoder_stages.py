"""Stage-wise, teacher-forced references for the inference forward (csrc/encoder.hip) -- helper module, no GPU needed to import.

The GPU tests of the forward see the pooled [B, out_dim] embedding only; a non-CLS token reaches it as one key among `len`.
Here every stage of a layer is compared, for EVERY live token, with an fp64 reference computed from the inputs the GPU
itself gave that stage (the workspace buffers of a run cut off after `l` layers), so the error budget is one stage deep.
u = 2^-8 is bf16's unit roundoff; e24 = 2^-24 fp32's.

  stage  inputs (GPU's own)        output        bound on |gpu - ref|                                    derived / measured
  A      tok_id, tok_pos           X_0           u |ref| + (1 + u) e32                                   derived (ln_fp32_err)
  B      X_{l-1}                   Q, K, V       u (|y| + acc) + acc,  acc = (K + 1) e24 (|X| |W|^T + |b|)  derived
  C      Q, K, V                   ctx           u (|ref| + A) + (1 + u) f32,  A = P |V|                 derived (attention_ref)
  D      ctx, X_{l-1}              Hm, X_l       2 u |ref| + c rms(ref row), share of differing elements <= f
                                                 c <= 4 c_ref, f <= max(10 f_ref, 1 %)                   measured against the
                                                 reference pair (fp32- vs fp64-accumulating chain on the same inputs)
  E      Y (fp32 pre-LN sums)      X_l           u |ref| + (1 + u) e32                                   derived (ln_fp32_err)
  F      X_{l-1}                   out [B, H]    c rms(ref row), c <= 4 c_ref                            measured, as D; c_ref = the larger
                                                 of the pair on the CLS rows and the pair on all rows of the all-token layer
  G      cls_b (the pooled row)    head_y        (K + 1) e24 (|x| |W|^T + |b|)  (fp32 sums, not rounded)   derived (head_ratios)
         head_y                    out [B, E]    ln_fp32_err of the given head_y  (fp32 output)          derived
  -      X_l                       pooled mean   (len + 2) e24 mean|x|                                   derived (k_masked_mean)

Stage B holds only if Q is stored UNSCALED (the EPI_QKV epilogue adds the bias and rounds; AttnArgs carries 0.125), stage C
only with that 0.125 inside the softmax.  X1, the attention-output LayerNorm, is written in place into X and overwritten by
the layer's output: it is the one hand-off no run can show, which is why stage D spans the whole tail.

Weights are the values the library packs: GEMM weights rounded to bf16, everything else fp32; all arithmetic of the
references is fp64 (torch, CPU).  The stand-in "kernels" (`acc=torch.float32`) are the same code accumulating in fp32: the
CPU test uses them to show that the bounds hold for a correct implementation and that planted faults break them.
"""
import contextlib
import ctypes as C
import hashlib
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.encoder import _attention_bf16, gelu_tail_fit

U = 2.0 ** -8          # bf16 unit roundoff (8 significand bits, round to nearest even)
E24 = 2.0 ** -24       # fp32 unit roundoff
F64, F32 = torch.float64, torch.float32
LOG2E = 1.44269504088896341

# lengths on both sides of the 8-row alignment, the 64-key tile and the 128-query workgroup; 512 = the position table's end.
# 2,064 packed rows: no multiple of 32, 128 or 256, few enough for the 4-slice split-contraction FFN2.
LENS_S = [1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 191, 193, 256, 257, 512]


def bf16r(t):
    """Round to bf16 (nearest even) -> fp64 values."""
    return t.to(torch.bfloat16).to(F64)


def bf16_trunc(t):
    """Planted fault: truncation towards zero instead of RNE."""
    b = t.to(F32).contiguous().view(torch.int32) & -65536
    return b.view(F32).to(F64)


# ---- weights ---------------------------------------------------------------------------------------------------------
class Weights:
    """fp64 copies of what EncoderTower.packed() hands the kernels: bf16-rounded GEMM weights, fp32 everything else."""

    def __init__(self, tower):
        cfg = tower.config
        self.H, self.heads, self.I = cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size
        self.eps = float(np.float32(cfg.layer_norm_eps))
        d = lambda p: p.detach().cpu().float().to(F64)
        e = tower.embeddings
        self.word, self.pos, self.type0 = d(e.word_embeddings.weight), d(e.position_embeddings.weight), d(e.token_type_embeddings.weight)[0]
        self.emb_g, self.emb_b = d(e.LayerNorm.weight), d(e.LayerNorm.bias)
        self.layers = []
        for ly in tower.encoder.layer:
            s = ly.attention.self
            self.layers.append(dict(
                wqkv=bf16r(torch.cat([d(s.query.weight), d(s.key.weight), d(s.value.weight)], 0)),
                bqkv=torch.cat([d(s.query.bias), d(s.key.bias), d(s.value.bias)], 0),
                wo=bf16r(d(ly.attention.output.dense.weight)), bo=d(ly.attention.output.dense.bias),
                ln1_g=d(ly.attention.output.LayerNorm.weight), ln1_b=d(ly.attention.output.LayerNorm.bias),
                w1=bf16r(d(ly.intermediate.dense.weight)), b1=d(ly.intermediate.dense.bias),
                w2=bf16r(d(ly.output.dense.weight)), b2=d(ly.output.dense.bias),
                ln2_g=d(ly.output.LayerNorm.weight), ln2_b=d(ly.output.LayerNorm.bias)))


# ---- building blocks -------------------------------------------------------------------------------------------------
def lin(x, w, b, acc=F64):
    """x W^T + b accumulated in `acc` -> fp64 values."""
    if acc is F64:
        return x @ w.T + b
    return F.linear(x.to(acc), w.to(acc), b.to(acc)).to(F64)


def ln(x, g, b, eps, acc=F64):
    if acc is F64:
        mu = x.mean(-1, keepdim=True)
        d = x - mu
        return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps) * g + b
    return F.layer_norm(x.to(acc), (x.shape[-1],), g.to(acc), b.to(acc), eps).to(F64)


def ln_fp32_err(x, g, b, eps, dx=None):
    """Elementwise bound on |fp32 LayerNorm(x) - exact LayerNorm(x)| for the kernels' row LayerNorm (ln_normalize, k_layernorm_rows,
    k_slab_finish_ln: a lane adds its H / 64 elements in sequence, a 6-level butterfly adds the lanes: a sum is D = H / 64 + 6
    additions deep).  x: exact fp64 rows; dx: bound on what the kernel's fp32 x already carries (None: x is given in fp32).
      mean      |d mean| <= D e24 mean|x| + mean(dx)                                  =: em
      d = x-mean |dd_i|  <= dx_i + em + e24 |d_i|                                      =: ed_i
      var       relative  <= (D + 3) e24 + 2 sum(|d_i| ed_i) / sum(d_i^2)             (squares, sum, / H, + eps)
      rstd      relative  <= half of that + 2 e24                                      (rsqrtf: 1 ulp)   =: er
      y_i       |dy_i|    <= |g_i| rstd ed_i + |d_i rstd g_i| (er + 3 e24) + e24 |y_i|
    With d / sigma = O(1) this is `a few e24 x (|d| / sigma |g| + |b|)`: D + 4 = 22 of them at H = 768 in the worst case."""
    H = x.shape[-1]
    D = H // 64 + 6
    dx = torch.zeros_like(x) if dx is None else dx
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    em = D * E24 * x.abs().mean(-1, keepdim=True) + dx.mean(-1, keepdim=True)
    ed = dx + em + E24 * d.abs()
    ss = (d * d).sum(-1, keepdim=True)
    var = ss / H + eps
    rstd = 1.0 / torch.sqrt(var)
    er = 0.5 * ((D + 3) * E24 + 2 * (d.abs() * ed).sum(-1, keepdim=True) / H / var) + 2 * E24
    y = d * rstd * g + b
    return g.abs() * rstd * ed + (d * rstd * g).abs() * (er + 3 * E24) + E24 * y.abs()


def ratio_bf16_of_fp32(gpu, ref, e32):
    """max over elements of |gpu - ref| / (u |ref| + (1 + u) e32): gpu = RNE_bf16(an fp32 value within e32 of ref)."""
    return float(((gpu - ref).abs() / (U * ref.abs() + (1 + U) * e32)).max())


# ---- stage A: embedding ----------------------------------------------------------------------------------------------
def embed_ref(W, tok_id, tok_pos):
    """-> (ref, e32).  The kernel adds word + pos + type in fp32 (two roundings) and normalises the row."""
    a, c, t = W.word[tok_id.long()], W.pos[tok_pos.long()], W.type0
    x = a + c + t
    dx = 2 * E24 * (a.abs() + c.abs() + t.abs())
    return ln(x, W.emb_g, W.emb_b, W.eps), ln_fp32_err(x, W.emb_g, W.emb_b, W.eps, dx)


def embed_sim(W, tok_id, tok_pos, rnd=bf16r):
    x = (W.word[tok_id.long()].to(F32) + W.pos[tok_pos.long()].to(F32) + W.type0.to(F32)).to(F64)
    return rnd(ln(x, W.emb_g, W.emb_b, W.eps, F32))


# ---- stage B: a projection with one rounding of an fp32 sum -----------------------------------------------------------
def proj_ref(x, w, b):
    """-> (y, bound): y = x W^T + b exactly; the kernel forms it as an fp32 sum of K + 1 terms in some order and rounds once."""
    y = x @ w.T + b
    acc = (x.shape[1] + 1) * E24 * (x.abs() @ w.abs().T + b.abs())
    return y, U * (y.abs() + acc) + acc


def qkv_sim(W, l, x, rnd=bf16r, acc=F32):
    L = W.layers[l - 1]
    return rnd(lin(x, L["wqkv"], L["bqkv"], acc))


# ---- stage C: attention ----------------------------------------------------------------------------------------------
def attention_ref(q, k, v, heads):
    """One sequence: q, k, v [len, H] (the kernel's bf16 operands) -> (ref, bound) [len, H].
    ref = P V, P = softmax(0.125 q k^T) in fp64.  The kernel (k_attention_fwd) evaluates p_j = exp2(fma(s_j, c, -m c)) in fp32,
    rounds the unnormalised p_j of a 64-key tile to bf16 for the P V product, sums the UNROUNDED p_j for the denominator,
    and rounds the quotient once:
      * bf16 p_j = p_j (1 + d_j), |d_j| <= u      ->  u sum_j P_j |v_j| = u A          (relative: the tile rescaling does not matter)
      * one rounding of the result                  ->  u |ref|
      * fp32: the score is a 64-term fp32 dot product, |ds_j| <= 65 e24 (|q| |k|^T)_j; the exponent fma(s, c, -fl(m c))
        carries 2 e24 (|s_j c| + |m c|); v_exp_f32 1 ulp.  Relative error of p_j:
            ep_j = 0.125 * 65 e24 (|q| |k|^T)_j + ln2 * 2 e24 (|s_j c| + |m c|) + 2 e24 * 2,
        in the numerator and (unrounded) in the denominator: sum_j P_j ep_j |v_j| + |ref| sum_j P_j ep_j;
        the fp32 accumulation of numerator and denominator over len terms: 2 (len + 8) e24 A.
    These fp32 terms are 1e-2 of the u terms at N(0, 0.02) weights and stay below them at logits of +-100."""
    n, H = q.shape
    d = H // heads
    qh, kh, vh = (t.view(n, heads, d).transpose(0, 1) for t in (q, k, v))          # [h, n, d]
    s = 0.125 * (qh @ kh.transpose(1, 2))
    P = torch.softmax(s, dim=-1)
    ref = P @ vh
    A = P @ vh.abs()
    s2 = s * LOG2E
    ep = 0.125 * 65 * E24 * (qh.abs() @ kh.abs().transpose(1, 2)) \
        + math.log(2.0) * 2 * E24 * (s2.abs() + s2.max(dim=-1, keepdim=True).values.abs()) + 4 * E24
    Pe = P * ep
    f32 = Pe @ vh.abs() + ref.abs() * Pe.sum(-1, keepdim=True) + 2 * (n + 8) * E24 * A
    bound = U * (ref.abs() + A) + (1 + U) * f32
    back = lambda t: t.transpose(0, 1).reshape(n, H)
    return back(ref), back(bound), back(U * (ref.abs() + A))


def attention_sim(q, k, v, heads, n_keys=None):
    """One sequence through the oracle's kernel-arithmetic attention (tiles of 64 keys, bf16 P, fp32 accumulators);
    n_keys: keys admitted (default all rows of k)."""
    n, H = q.shape
    d = H // heads
    nk = k.shape[0]
    L = max(n, nk)
    pad = lambda t: F.pad(t.to(F32), (0, 0, 0, L - t.shape[0])).view(1, L, heads, d).transpose(1, 2)
    o = _attention_bf16(pad(q), pad(k), pad(v), [nk if n_keys is None else n_keys], 0.125, None)
    return bf16r(o.transpose(1, 2).reshape(L, H)[:n].to(F64))


def per_sequence(lens, fn, *mats):
    """Apply fn to each sequence's rows of the live-row matrices `mats`; concatenates the (tuple of) results."""
    outs, o = [], 0
    for n in lens:
        r = fn(*(m[o:o + n] for m in mats))
        outs.append(r if isinstance(r, tuple) else (r,))
        o += n
    cat = tuple(torch.cat([x[i] for x in outs], 0) for i in range(len(outs[0])))
    return cat if len(cat) > 1 else cat[0]


# ---- stage D: the tail of a layer through the unobservable X1 -----------------------------------------------------------
def tail_chain(W, l, ctx, xprev, acc=F64, rnd=bf16r, resid_from_x1=False):
    """(ctx, X_{l-1}) -> (Hm, X_l, X_l unrounded):  X1 = bf16(LN(ctx Wo^T + bo + X_{l-1})), Hm = bf16(gelu_tail_fit(X1 W1^T + b1)),
    X_l = bf16(LN(Hm W2^T + b2 + X1)); the third value is the last LayerNorm's output before the rounding (the CLS tail's `out`).
    resid_from_x1: planted fault -- the attention-output stage reads its residual after X1 overwrote it in place."""
    L = W.layers[l - 1]
    x1 = rnd(ln(lin(ctx, L["wo"], L["bo"], acc) + xprev, L["ln1_g"], L["ln1_b"], W.eps, acc))
    if resid_from_x1:
        x1 = rnd(ln(lin(ctx, L["wo"], L["bo"], acc) + x1, L["ln1_g"], L["ln1_b"], W.eps, acc))
    pre = lin(x1, L["w1"], L["b1"], acc)
    hm = rnd(gelu_tail_fit(pre if acc is F64 else pre.to(acc)).to(F64))
    y = lin(hm, L["w2"], L["b2"], acc) + x1
    xl = ln(y, L["ln2_g"], L["ln2_b"], W.eps, acc)
    return hm, rnd(xl), xl


def tail_metrics(got, ref, rel=2 * U):
    """-> (c, f): c = max over elements of (|got - ref| - rel |ref|)+ / rms(ref row); f = share of elements that differ at all."""
    rms = ref.pow(2).mean(-1, keepdim=True).sqrt()
    c = float((((got - ref).abs() - rel * ref.abs()).clamp(min=0) / rms).max())
    return c, float((got != ref).double().mean())


def tail_bars(c_ref, f_ref):
    """GPU bars from the reference pair's floors: another summation order of the same length has the same error scale, and 4x
    covers three chained GEMMs whose orders all differ; a truncating / biased conversion differs on ~half of all elements."""
    return 4 * c_ref, max(10 * f_ref, 0.01)


# ---- stage F: the CLS tail of the last layer --------------------------------------------------------------------------
def cls_chain(W, l, xprev, lens, fold, acc=F64):
    """X_{l-1} (live rows) -> out [B, H]: the last layer for the CLS rows only, fp32 LayerNorm output unrounded.
    fold: Wk, Wv folded through the CLS query (cls_fold.hpp: fp32 u, softmax weights and z -- no bf16 K, V or P);
    else K, V of every token in bf16 and the kernel-arithmetic attention (bf16 P per 64-key tile)."""
    L = W.layers[l - 1]
    H, heads = W.H, W.heads
    d = H // heads
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    xc = xprev[torch.as_tensor(starts)]
    q = bf16r(lin(xc, L["wqkv"][:H], L["bqkv"][:H], acc))
    ctx = []
    if not fold:
        kv = bf16r(lin(xprev, L["wqkv"][H:], L["bqkv"][H:], acc))
    for b, (s, n) in enumerate(zip(starts, lens)):
        x = xprev[s:s + n]
        if fold:
            wk, wv, bv = L["wqkv"][H:2 * H].view(heads, d, H), L["wqkv"][2 * H:], L["bqkv"][2 * H:]
            u = 0.125 * torch.einsum("hj,hjn->hn", q[b].view(heads, d), wk)            # [heads, H]
            p = torch.softmax(x @ u.T, dim=0)                                               # [n, heads]
            z = p.T @ x                                                                     # [heads, H]
            c = torch.einsum("hjn,hn->hj", wv.view(heads, d, H), z).reshape(H) + bv
            ctx.append(bf16r(c)[None])
        else:
            k, v = kv[s:s + n, :H], kv[s:s + n, H:]
            if acc is F64:
                qh, kh, vh = q[b].view(heads, 1, d), k.view(n, heads, d).transpose(0, 1), v.view(n, heads, d).transpose(0, 1)
                sc = 0.125 * LOG2E * (qh @ kh.transpose(1, 2))                              # [h, 1, n]
                o, den = torch.zeros(heads, 1, d, dtype=F64), torch.zeros(heads, 1, 1, dtype=F64)
                m = sc.max(dim=-1, keepdim=True).values
                for k0 in range(0, n, 64):       # bf16 P relative to the running maximum of the tiles so far, as the kernel's
                    mt = sc[..., :k0 + 64].max(dim=-1, keepdim=True).values
                    pr = torch.exp2(sc[..., k0:k0 + 64] - mt)
                    sc_f = torch.exp2(mt - m)
                    o += sc_f * (bf16r(pr) @ vh[:, k0:k0 + 64])
                    den += sc_f * pr.sum(-1, keepdim=True)
                ctx.append(bf16r((o / den).reshape(1, H)))
            else:
                ctx.append(attention_sim(q[b][None], k, v, heads))
    ctx = torch.cat(ctx, 0)
    return tail_chain(W, l, ctx, xc, acc=acc)[2]


# ---- stage G: the head, LayerNorm(Linear(H, E)(pooled row)) -----------------------------------------------------------------
class HeadWeights:
    """fp64 copies of what packed(head) hands the head kernels: the Linear's weight rounded to bf16, the rest fp32."""

    def __init__(self, lin_mod, ln_mod):
        d = lambda p: p.detach().cpu().float().to(F64)
        self.w, self.b, self.g, self.beta = bf16r(d(lin_mod.weight)), d(lin_mod.bias), d(ln_mod.weight), d(ln_mod.bias)
        self.eps = float(np.float32(ln_mod.eps))


def head_ratios(HW, cls_b, head_y, out):
    """-> (ratio of head_y, ratio of out), both against derived bounds, teacher-forced:
      head_y  against cls_b W^T + b in fp64 within (K + 1) e24 (|x| |W|^T + |b|): launch_gemm<EPI_F32> stores the fp32 sum of
              K + 1 terms unrounded -- the `acc` term of proj_ref;
      out     against the exact LayerNorm of the GIVEN head_y within ln_fp32_err (k_layernorm with H = E, fp32 output)."""
    y = cls_b @ HW.w.T + HW.b
    acc = (cls_b.shape[1] + 1) * E24 * (cls_b.abs() @ HW.w.abs().T + HW.b.abs())
    rY = float(((head_y - y).abs() / acc).max())
    ref, e32 = ln(head_y, HW.g, HW.beta, HW.eps), ln_fp32_err(head_y, HW.g, HW.beta, HW.eps)
    return rY, float(((out - ref).abs() / e32).max())


def head_sim(HW, cls_b):
    """The stand-in head: fp32 accumulation, fp32 LayerNorm -> (head_y, out)."""
    y = lin(cls_b, HW.w, HW.b, F32)
    return y, ln(y, HW.g, HW.beta, HW.eps, F32)


def make_head(H, E, seed=17):
    """Linear(H, E) + LayerNorm(E) with init statistics: N(0, 0.02) weight and bias, gain 1 + N(0, 0.05), bias N(0, 0.02)."""
    g = torch.Generator().manual_seed(seed + E)
    lin_mod, ln_mod = torch.nn.Linear(H, E), torch.nn.LayerNorm(E)
    with torch.no_grad():
        lin_mod.weight.copy_(torch.randn(E, H, generator=g) * 0.02)
        lin_mod.bias.copy_(torch.randn(E, generator=g) * 0.02)
        ln_mod.weight.add_(torch.randn(E, generator=g) * 0.05)
        ln_mod.bias.copy_(torch.randn(E, generator=g) * 0.02)
    return lin_mod, ln_mod


# ---- workspace decoders ----------------------------------------------------------------------------------------------
def blocked_index(rows, N):
    """Element offsets of a [rows, N] matrix in the blocked layout (csrc/gemm_kernel.hpp:hm_blocked_offset)."""
    t = torch.arange(rows)[:, None]
    f = torch.arange(N)[None, :]
    return ((t >> 5) * (N >> 3) + (f >> 3)) * 256 + (t & 31) * 8 + (f & 7)


def decode_blocked(flat, rows, N, swap_last_halves=False):
    """flat: 1-D buffer in the blocked layout -> [rows, N].  swap_last_halves: planted fault -- the two 16-row halves of the
    (ragged) last 32-row block exchanged."""
    t = torch.arange(rows)
    if swap_last_halves:
        t = torch.where((t >> 5) == ((rows - 1) >> 5), t ^ 16, t)
    return flat[blocked_index((rows + 31) // 32 * 32, N)[t]]


def encode_blocked(m):
    """[rows, N] -> flat blocked buffer of ceil(rows / 32) * 32 * N elements (unwritten slots NaN)."""
    rows, N = m.shape
    flat = torch.full((((rows + 31) // 32) * 32 * N,), float("nan"), dtype=m.dtype)
    flat[blocked_index(rows, N)] = m
    return flat


def decode_rowmajor(flat, rows, N):
    return flat[:rows * N].view(rows, N)


def decode_featmajor(flat, rows, N, ld):
    return flat[:N * ld].view(N, ld)[:, :rows].T


# ---- the library under the stages (GPU) ------------------------------------------------------------------------------
DEFAULTS = dict(fused_ln_min_rows=128 * 192, fused_ln_max_k=1 << 30, hm_blocked=1, cls_fold=1, cls_fold_min_rows=16384,
                gemm_tile_policy=0, ffn2_splitk=1, ln_rows=1)
_opts = dict(DEFAULTS)


@contextlib.contextmanager
def options(kslice=False, **kw):
    """Set library options (and KSLICE_MIN_ROWS = 1 for K-slice-major weights) and restore the defaults on the way out."""
    from convdr_amd import _lib
    from convdr_amd.model import models as MM
    L = _lib.lib()
    old_ks = MM.KSLICE_MIN_ROWS
    try:
        for k, v in kw.items():
            assert k in DEFAULTS, k
            _lib.check(L.convdr_set_option(k.encode(), int(v)), "convdr_set_option")
            _opts[k] = int(v)
        if kslice:
            MM.KSLICE_MIN_ROWS = 1
        yield
    finally:
        MM.KSLICE_MIN_ROWS = old_ks
        for k in kw:
            L.convdr_set_option(k.encode(), DEFAULTS[k])
            _opts[k] = DEFAULTS[k]


def _fused(rows, H, K):
    return H == 768 and rows >= _opts["fused_ln_min_rows"] and K % 32 == 0 and K <= _opts["fused_ln_max_k"]


def layouts(rows, H, I):
    """Which hand-offs the library keeps blocked under the current options (csrc/encoder.hip:encoder_layer_forward), whether
    FFN2 + LayerNorm is the fused kernel, and whether Y holds the FFN2 pre-LayerNorm sums."""
    blk = _opts["hm_blocked"] != 0
    qk = blk and _fused(rows, H, H)
    hm = blk and _fused(rows, H, I) and I % 256 == 0 and (I // 256) * ((rows + 255) // 256) >= 192
    split = _opts["ffn2_splitk"] != 0 and H == 768 and I >= 2048 and rows <= 42 * 128
    return dict(qk=qk, ctx=qk, hm=hm, y_live=not _fused(rows, H, I) and not split)


def make_inputs(lens, vocab, seed, pads=()):
    """Right-padded int64 ids [B, max(lens)] (CLS id 0 first, ids >= 3 elsewhere, 0 behind the sequence) and int32 lens;
    pads: (sequence, position) pairs that get RoBERTa's pad id 1 inside a sequence."""
    rs = np.random.RandomState(seed)
    lens = np.asarray(lens, np.int32)
    ids = rs.randint(3, vocab, size=(len(lens), int(lens.max()))).astype(np.int64)
    ids[:, 0] = 0
    ids *= (np.arange(ids.shape[1])[None, :] < lens[:, None])
    for b, j in pads:
        assert 0 < j < lens[b]
        ids[b, j] = 1
    return ids, lens


def run_layers(tower, ids, lens, l, cls=False, ragged=False, kslice=False, head=None):
    """The library's forward cut off after `l` layers, called as EncoderTower.embed does but on a copy of the packed config
    with layers = l, out_dim = 0 and pool_mean = 1 (every layer a full all-token layer; cls=True: pool_mean = 0, the last
    layer's CLS tail) and on a workspace of the library's own size pre-filled with 0xFF (every bf16 / fp32 a NaN).
    -> dict of fp64 CPU tensors for the LIVE rows only: tok_id, tok_pos, X, Q, K, V, ctx, Hm, (Y), out; 'X_bits' = the raw
    bf16 bits of X.  After l layers Q .. Hm (Y) are layer l's intermediates and X = X_l.
    head = (Linear, LayerNorm): packed with that head and out_dim kept, so the run ends in the head GEMM + LayerNorm; then
    also 'cls_b' [B, H] (the pooled row the head consumed, bf16) and 'head_y' [B, out_dim] (its fp32 sums), out [B, out_dim]."""
    from convdr_amd import _lib
    L_ = _lib.lib()
    dev = torch.device("cuda")
    lens = np.asarray(lens, np.int32)
    B = len(lens)
    cu = np.zeros(B + 1, np.int32)
    np.cumsum((lens + 7) // 8 * 8, out=cu[1:])
    rows, max_len = int(cu[-1]), int(lens.max())
    live = torch.from_numpy(np.concatenate([cu[b] + np.arange(lens[b]) for b in range(B)]).astype(np.int64))
    with torch.cuda.device(dev):
        c0, w, keep = tower.packed(head)
        if not kslice and w.layers[0].w2_ks:      # an earlier run built the K-slice-major copies: pack afresh without them
            tower.invalidate_packed()
            c0, w, keep = tower.packed(head)
        if kslice:
            from convdr_amd.model import models as MM
            assert MM.KSLICE_MIN_ROWS <= rows, "run under options(kslice=True)"
            tower._ensure_kslice(c0, w, keep, rows, dev)
            assert w.layers[0].w2_ks
        c = _lib.EncoderConfig.from_buffer_copy(c0)
        assert 0 <= l <= c0.layers
        c.layers, c.pool_mean = l, 0 if cls else 1
        if head is None:
            c.out_dim = 0
        else:
            assert c.out_dim == head[0].out_features and l >= 1
        H, I = c.hidden, c.intermediate
        need = L_.convdr_encoder_workspace_bytes(C.byref(c), rows, B)
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
        out = torch.full((B, c.out_dim or H), float("nan"), dtype=torch.float32, device=dev)
        cu_d, lens_d = torch.from_numpy(cu).to(dev), torch.from_numpy(lens).to(dev)
        if ragged:
            tok = torch.from_numpy(np.concatenate([ids[b, :lens[b]] for b in range(B)]).astype(np.int32)).to(dev)
            off = np.zeros(B + 1, np.int32)
            np.cumsum(lens, out=off[1:])
            off_d = torch.from_numpy(off).to(dev)
            _lib.check(L_.convdr_encoder_forward_ragged(C.byref(c), C.byref(w), _lib.ptr(tok), tok.numel(), _lib.ptr(off_d), B,
                                                        _lib.ptr(cu_d), _lib.ptr(lens_d), rows, max_len, _lib.ptr(ws), ws.numel(),
                                                        _lib.ptr(out), _lib.stream_ptr()), "convdr_encoder_forward_ragged")
        else:
            ids_d = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(dev)
            _lib.check(L_.convdr_encoder_forward(C.byref(c), C.byref(w), _lib.ptr(ids_d), 0, None, B, ids_d.shape[1],
                                                 _lib.ptr(cu_d), _lib.ptr(lens_d), rows, max_len, _lib.ptr(ws), ws.numel(),
                                                 _lib.ptr(out), _lib.stream_ptr()), "convdr_encoder_forward")
        torch.cuda.synchronize()
        lay = (C.c_int64 * 14)()
        _lib.check(L_.convdr_encoder_debug_layout(C.byref(c), rows, B, lay), "convdr_encoder_debug_layout")
    names = ("tok_id", "tok_pos", "X", "Q", "K", "Vt", "ctx", "Hm", "Y")
    off = dict(zip(names, list(lay)[:9]))
    ldt = int(lay[13])
    assert int(ws[:4].view(torch.int32)[0]) == 0, "status word"
    rows32 = (rows + 31) // 32 * 32

    def buf(name, n, dtype):
        size = n * torch.empty((), dtype=dtype).element_size()
        assert off[name] + size <= need
        return ws[off[name]:off[name] + size].view(dtype).cpu()
    lo = layouts(rows, H, I)
    r = {"rows": rows, "live": live, "layout": lo, "out": out.cpu().to(F64)}
    if head is not None:
        for name, slot, dtype, n in (("cls_b", 9, torch.bfloat16, H), ("head_y", 12, torch.float32, c.out_dim)):   # (debug_layout's order)
            o, size = int(lay[slot]), B * n * torch.empty((), dtype=dtype).element_size()
            assert o + size <= need
            r[name] = ws[o:o + size].view(dtype).cpu().view(B, n).to(F64)
    r["tok_id"], r["tok_pos"] = buf("tok_id", rows, torch.int32)[live], buf("tok_pos", rows, torch.int32)[live]
    xb = decode_rowmajor(buf("X", rows * H, torch.bfloat16), rows, H)[live]
    r["X"], r["X_bits"] = xb.to(F64), xb.view(torch.int16).clone()
    if l >= 1 and not cls:
        for n, blocked in (("Q", lo["qk"]), ("K", lo["qk"]), ("ctx", lo["ctx"])):
            flat = buf(n, rows32 * H, torch.bfloat16)
            r[n] = (decode_blocked(flat, rows, H) if blocked else decode_rowmajor(flat, rows, H))[live].to(F64)
        r["V"] = decode_featmajor(buf("Vt", H * ldt, torch.bfloat16), rows, H, ldt)[live].to(F64)
        flat = buf("Hm", rows32 * I, torch.bfloat16)
        r["Hm"] = (decode_blocked(flat, rows, I) if lo["hm"] else decode_rowmajor(flat, rows, I))[live].to(F64)
        if lo["y_live"]:
            r["Y"] = decode_rowmajor(buf("Y", rows * H, torch.float32), rows, H)[live].to(F64)
    for k, v in r.items():
        if torch.is_tensor(v) and v.dtype.is_floating_point and (k != "out" or cls or l >= 1):
            assert bool(torch.isfinite(v).all()), "%s: a live row is not finite (layers=%d)" % (k, l)
    return r


# ---- the models and inputs both test files use ----------------------------------------------------------------------------
# hidden / intermediate of every model shape (heads = hidden / 64).  W and N are the two the stage files grew up with; the
# ENVELOPE shapes are the other six hidden sizes check_config / check_train_config admit, each with an intermediate size that
# takes a path of its own:
#   H128   I = 64: half a feature tile, FFN2 a single K step           H640  I = 448: H % 256 != 0, 2.5 LayerNorm groups
#   H256   I = 192: no multiple of 128; QKV thirds one 256-tile wide   H896  I = 2304: I % 256 == 0 with H % 256 != 0
#   H512   I = 1024: thirds two tiles wide                             H1024 I = 4096: every upper limit at once
SHAPES = dict(W=(768, 3072), N=(384, 320), H128=(128, 64), H256=(256, 192), H512=(512, 1024), H640=(640, 448),
              H896=(896, 2304), H1024=(1024, 4096))
ENVELOPE = ["H128", "H256", "H512", "H640", "H896", "H1024"]


def make_model(shape, stats):
    """shape 'W': 768 / 12 heads / 3072, 'N': 384 / 6 heads / 320 (N = 1152 is no multiple of 256, I = 2.5 feature tiles, the
    general LayerNorm), or one of ENVELOPE (SHAPES above); 2 layers, vocabulary 1000.  stats 'init': N(0, 0.02) + the bias and
    gain noise of the other parity tests, 'trained': tests.helpers.trained_like_.  CPU model (rdot_nll class); its tower is
    `.roberta`."""
    from convdr_amd.model.models import MSMarcoConfigDict, RobertaConfig
    from tests.helpers import trained_like_
    H, I = SHAPES[shape]
    dims = dict(hidden_size=H, num_attention_heads=H // 64, intermediate_size=I)
    torch.manual_seed(11)
    model = MSMarcoConfigDict["rdot_nll"].model_class(RobertaConfig(vocab_size=1000, num_hidden_layers=2, **dims))
    if stats == "trained":
        assert shape == "W"
        trained_like_(model, seed=5)
    else:
        with torch.no_grad():
            for n, p in model.named_parameters():
                if n.endswith("bias"):
                    p.normal_(0, 0.02)
                elif "LayerNorm.weight" in n or n == "norm.weight":
                    p.add_(torch.randn_like(p) * 0.05)
    return model.eval()


def input_s():
    """Input S: LENS_S with RoBERTa's pad id planted inside two sequences."""
    return make_inputs(LENS_S, 1000, 0, pads=((8, 5), (15, 300)))


def input_m():
    """Input M (test_blocked_ffn_activation_layout_is_result_neutral's): 44 sequences of 40..128 tokens, >= 3842 packed rows,
    no multiple of 32 -- enough for the blocked FFN activation hand-off."""
    rs = np.random.RandomState(5)
    lens = rs.randint(40, 129, size=44)
    lens[:3] = (128, 41, 127)
    rows = int(((lens + 7) // 8 * 8).sum())
    assert rows % 32 != 0 and rows >= 3842
    return make_inputs(lens, 1000, 6)


def host_tokens(ids, lens):
    """tok_id, tok_pos of the live rows as k_seq_pack writes them (RoBERTa positions), computed on the host."""
    from oracle.encoder import roberta_position_ids
    t = torch.from_numpy(ids)
    pos = roberta_position_ids(t, 1)
    keep = torch.arange(t.shape[1])[None, :] < torch.as_tensor(np.asarray(lens))[:, None]
    return t[keep].to(torch.int32), pos[keep].to(torch.int32)


# ---- memo: references depend only on (weights, stage, inputs) -----------------------------------------------------------
_MEMO = {}


def memo(tag, tensors, fn):
    """fn() cached on the bytes of `tensors`: option variants that hand a stage the same bits share one reference."""
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.contiguous().numpy().tobytes())
    key = (tag, h.hexdigest())
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]
