"""Stage-wise, teacher-forced references for the TRAINING forward and backward (csrc/train.hip) -- helper module, no GPU
needed to import.  The manner is tests/encoder_stages.py's: every stage is compared, per element and for every live token,
with an fp64 reference computed from the bytes the GPU itself handed that stage, so every bound is one stage deep.

How a stage's inputs are seen.  The forward keeps everything (LayerSave, the compact c_* rows of the CLS tail): one run shows
all of it (`convdr_encoder_train_debug_layout`).  The backward rewrites G0 / G1 / dXb1 / dXb2 / dctx in every layer, so it is
run once per layer with the option "train_bwd_stop_layer" = NL, NL - 1, .., 0 on the same forward: the run stopped at l shows
layer l's outputs, the run stopped at l + 1 what layer l consumed (G0 + dXb2).  The backward is bitwise deterministic; the
premise -- the per-layer buffers above the stop are byte-equal between two runs -- is asserted in run_train.
u = 2^-8 (bf16), e24 = 2^-24 (fp32); K = contraction length.

  TRAINING FORWARD (all from one run)
  stage   inputs (GPU's own)       output            bound on |gpu - ref|                                       kind
  A       tok_id, tok_pos          Xin_0             u |ref| + (1 + u) e32, mask DROP_SITE_EMB                  derived (ln_fp32_err)
  B       Xin                      QKV               u (|y| + acc) + acc                                        derived (proj_ref)
  C       QKV                      ctx, c_ctx        attention_ref's bound (no probability dropout)             derived
  LSE     QKV                      LSE (base 2)      lse_ref: score, exponent, sum and log2 terms               derived
  Y1      ctx, Xin                 Y1, c_Y1          (K + s + 2) e24 (m (|ctx| |Wo|^T + |bo|) + |Xin|)          derived; the mask m on
                                                     the dense output, not on the residual; s = slab slices (compact rows)
  E       Y1 / Y2 / cls_y / head_y X1, Xin_{l+1}, Xout, cls_f, cls_b, out    u |ref| + (1 + u) e32              derived (ln_fp32_err)
  H       X1                       Hm, Hpre          Hpre: proj_ref (gelu_gp 0) or gelu' image, u |g'| + 4e-5 + 0.8 acc (gelu_gp 1)
                                                     Hm: u |ref| + 1.13 acc + 8 e24 (|pre| + 1)                 derived
  Y2      Hm, X1                   Y2, cls_y         as Y1                                                      derived
  pool    Xout                     cls_f, cls_b      (len + 2) e24 mean|x|                                      derived
  head    cls_b                    head_y            (K + 2) e24 (|x| |W|^T + |b|)                              derived

  BACKWARD (run stopped at l; inputs from the run stopped at l + 1 where the table says "above")
  LN'     dYa (+ dYb), Y           dXf (fp32), dXb   ln_bwd_ref: e32 elementwise; dXb: u |m ref| + (1 + u) m e32, mask m
          head: d_out, head_y -> dhead_y, dhead_yb;  CLS: dcls, cls_y -> dcls_y;  LN2': G0 + dXb2 (above), Y2 -> G1, dYb;
          LN1': G1 + dXb1, Y1 -> G0, dYb2;  compact LN1': c_dX1f, c_Y1 -> c_dY1, c_dYb2 with the mask row cu[r]    derived
  sums    the same                 dbias, dgamma, dbeta (b2 / ln2_g / ln2_b, bo / ln1_g / ln1_b, head_b / head_ln_g / _b)
                                                     sum of the elementwise bounds + depth e24 sum|terms|       derived
  dgrad   dY, W^T                  dhead -> dcls_f (fp32), dHpre (gelu_gp 1: x the saved gelu' image), dXb1, dctx, dXb2, c_dctx
                                                     u (|y| + acc) + acc,  acc = (K + 1) e24 |dY| |W|           derived
  dgelu   dYb, W2^T, Hpre          dHpre (gelu_gp 0), c_dHpre: through the bf16 dgrad output k_dgelu_colsum rewrites in place
                                                     dgelu_ref: two roundings deep against s gelu'(Hpre), ~2 u |ref|       derived
                                                     (no measured pair: both members of such a pair differ only by rare bf16
                                                     flips, a handful per case, and one pair's maximum over them is no scale)
  c_dX1   c_dHpre, dcls_y          c_dX1f            (K + s + 2) e24 (|dHpre| |W1| + |dcls_y|)                  derived
  cast    dcls_y                   c_dYb             bf16(fp32(v m)), mask row cu[r]: bit-exact                 exact
  scatter c_dctx, c_dY1            dctx, G0, dQKV    the CLS rows equal, every other row zero                   exact
  mean'   dcls                     G0                3 e24 |ref| on the tokens, zero on the alignment rows      derived
  wgrad   dY, X (all packed rows)  w1, w2, wqkv, wo, head_w      (rows + slices + 2) e24 |dY|^T |X|             derived
  colsum  dHpre, dQKV, c_dYb       b1, bqkv (all three thirds), the last layer's b2 under dropout
                                                     depth e24 sum|terms|                                       derived

  att'    QKV, dctx, LSE, ctx      dQKV              per (token, head, Q / K / V) slice: c <= 4 c_ref, f <= max(10 f_ref, 1 %)
                                                     measured (pair: attn_bwd_chain in fp64 / fp32; P and dS rounded to bf16, D from
                                                     the bf16 ctx as in the kernels)
  att'tail QKV, c_dctx, LSE, c_ctx32 dQKV            the CLS tail: one live query per sequence, dK / dV single products -- a pair
                                                     there differs by a handful of bf16 flips only (as dgelu); attn_bwd_tail_ref  derived

  Under probability dropout stages C and att' take the oracle's mask (att_mask_seq; attention_ref_drop: the denominator is the
  undropped row's); where the forward kept its bits (Mbits, max_len <= 256) they are decoded and must equal that mask bit for bit.
  emb'    G0 + dXb2 behind layer 0, ids, mask EMB -> word_emb, pos_emb, type_emb[0], emb_ln_g / b of the full run
                                                     rows' LayerNorm' bounds + (count + 1) e24 sum|dx| per table row       derived

The stand-in "kernels" (`acc=F32`) are the same code with fp32 accumulation and the kernels' rounding points; the CPU test
uses them to show that every bound holds for a correct implementation and that planted faults break them."""
import ctypes as C
import math

import numpy as np
import torch

from oracle import dropout as OD
from oracle.encoder import gelu_tail_fit
from tests import encoder_stages as ES
from tests.encoder_stages import E24, F32, F64, U, bf16r

BF16 = torch.bfloat16
GP_FIT_ERR = 4e-5       # max |gelu' fit - gelu'| of gelu_tail2_gp / gelu_grad (3.6e-5 / 3.9e-5: tests/test_gelu_fit_cpu.py)
LN_BWD_BLOCKS, COLSUM_CHUNKS, CLS_MAX_SPLIT = 768, 64, 16


# ---- dropout masks ---------------------------------------------------------------------------------------------------
def mask_rows(drop, site, layer, rows, H):
    """fp64 [len(rows), H] multipliers of a hidden-state site for the PACKED rows `rows` (oracle/dropout.py's definition).
    drop = (p_hidden, p_attention, seed) or None."""
    rows = np.asarray(rows, np.int64)
    if drop is None or drop[0] <= 0:
        return torch.ones(len(rows), H, dtype=F64)
    key, thresh, scale = OD.site_params(drop[2], site, layer, drop[0])
    with np.errstate(over="ignore"):
        pair = rows.astype(np.uint32)[:, None] * np.uint32(H // 2) + np.arange(H // 2, dtype=np.uint32)[None, :]
    even, odd = OD._pair_multipliers(pair, key, thresh, scale)
    m = np.empty((len(rows), H), np.float32)
    m[:, 0::2], m[:, 1::2] = even, odd
    return torch.from_numpy(m).to(F64)


def att_mask_seq(drop, layer, base_row, n, heads):
    """fp64 [heads, n, n] multipliers (query, key) of the attention probabilities of the sequence whose first packed row is
    base_row (oracle/dropout.py's definition); ones without probability dropout."""
    if drop is None or drop[1] <= 0:
        return torch.ones(heads, n, n, dtype=F64)
    key, thresh, scale = OD.site_params(drop[2], OD.SITE_ATT_PROBS, layer, drop[1])
    rows = (base_row + np.arange(n)).astype(np.uint32)
    kp = np.arange((n + 1) // 2, dtype=np.uint32)
    out = np.empty((heads, n, 2 * len(kp)), np.float32)
    with np.errstate(over="ignore"):
        for h in range(heads):
            base = (rows * np.uint32(heads) + np.uint32(h)) << np.uint32(9)
            out[h, :, 0::2], out[h, :, 1::2] = OD._pair_multipliers(base[:, None] + kp[None, :], key, thresh, scale)
    return torch.from_numpy(out[:, :, :n]).to(F64)


def decode_mbits(mbits, base_row, n):
    """The forward's kept dropout bits (csrc/attention_train.hpp, ATTM_PIECES) of one sequence: mbits int32 [heads, 8, ldt] ->
    bool [heads, n, n] (query, key).  word (head, piece 2 (key >> 6) + ((key >> 3) & 1), query row), bit
    16 ((key >> 5) & 1) + 8 ((key >> 4) & 1) + (key & 7)."""
    key = torch.arange(n)
    piece = 2 * (key >> 6) + ((key >> 3) & 1)
    bit = 16 * ((key >> 5) & 1) + 8 * ((key >> 4) & 1) + (key & 7)
    words = mbits[:, :, base_row:base_row + n].to(torch.int64) & 0xffffffff        # [heads, 8, n queries]
    w = words[:, piece, :].transpose(1, 2)                                          # [heads, query, key]
    return ((w >> bit[None, None, :]) & 1).bool()


def attention_ref_drop(q, k, v, heads, mask):
    """ES.attention_ref with the probability mask (k_attention_train_fwd<true>): the denominator is the undropped row's, the
    unnormalised p_j is multiplied by m_j (0 or 1 / keep: one more fp32 rounding) before its bf16 rounding.
    -> (ref, bound, lse-free) as attention_ref: ref = (P m) V, A = (P m) |V|."""
    n, H = q.shape
    d = H // heads
    qh, kh, vh = (t.view(n, heads, d).transpose(0, 1) for t in (q, k, v))
    s = 0.125 * (qh @ kh.transpose(1, 2))
    P = torch.softmax(s, dim=-1)
    PM = P * mask
    ref = PM @ vh
    A = PM @ vh.abs()
    s2 = s * ES.LOG2E
    ep = 0.125 * 65 * E24 * (qh.abs() @ kh.abs().transpose(1, 2)) \
        + math.log(2.0) * 2 * E24 * (s2.abs() + s2.max(dim=-1, keepdim=True).values.abs()) + 4 * E24
    f32 = (PM * (ep + E24)) @ vh.abs() + ref.abs() * (P * ep).sum(-1, keepdim=True) + 2 * (n + 8) * E24 * A
    bound = U * (ref.abs() + A) + (1 + U) * f32
    back = lambda t: t.transpose(0, 1).reshape(n, H)
    return back(ref), back(bound)


# ---- gelu' -------------------------------------------------------------------------------------------------------------
def gelu_grad_exact(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def gelu_grad_fit(x):
    """gelu_grad of csrc/gemm_kernel.hpp (the tail fit's Q(t) and x phi(x)) in x's dtype."""
    t = x.abs().clamp(max=9.0)
    p = ((t * 0.0041585 - 0.04571999) * t - 0.46495319) * t - 1.14955714
    q = torch.exp2(p * t - 1.0)
    cdf = torch.where(x >= 0, 1.0 - q, q)
    return x * 0.3989422804014327 * torch.exp2(-0.7213475204444817 * x * x) + cdf


# ---- forward stages -----------------------------------------------------------------------------------------------------
def resid_ref(x, w, b, resid, mask=None, slices=0):
    """Y = m (x W^T + b) + resid as ONE fp32 sum -> (ref, bound): EPI_RESID_F32 / k_slab_finish."""
    mask = 1.0 if mask is None else mask
    y = mask * (x @ w.T + b) + resid
    a = mask * ((x.abs().to(F32) @ w.abs().to(F32).T).to(F64) * 1.001 + b.abs()) + resid.abs()
    return y, (x.shape[1] + slices + 2) * E24 * a


def resid_sim(x, w, b, resid, mask=None, acc=F32):
    mask = 1.0 if mask is None else mask
    return ((ES.lin(x, w, b, acc).to(F32) * torch.as_tensor(mask).to(F32)) + resid.to(F32)).to(F64)


def ln_out_ratio(got_b, got_f, y, g, b, eps):
    """Stage E from an fp32 input y: bf16 and / or fp32 LayerNorm outputs -> max ratio."""
    ref, e32 = ES.ln(y, g, b, eps), ES.ln_fp32_err(y, g, b, eps)
    r = 0.0
    if got_b is not None:
        r = max(r, ES.ratio_bf16_of_fp32(got_b, ref, e32))
    if got_f is not None:
        r = max(r, float(((got_f - ref).abs() / e32).max()))
    return r


def ffn1_ref(x1, w1, b1):
    """-> dict: pre (exact), acc, Hm ref / bound, gelu' ref / bound, Hpre bound (EPI_GELU_SAVE / EPI_GELU_GP)."""
    pre = x1 @ w1.T + b1
    acc = (x1.shape[1] + 1) * E24 * ((x1.abs().to(F32) @ w1.abs().to(F32).T).to(F64) * 1.001 + b1.abs())
    hm = gelu_tail_fit(pre)
    gp = gelu_grad_exact(pre)
    return dict(pre=pre, pre_bound=U * (pre.abs() + acc) + acc,
                hm=hm, hm_bound=U * hm.abs() + (1 + U) * (1.13 * acc + 8 * E24 * (pre.abs() + 1)),
                gp=gp, gp_bound=U * gp.abs() + (1 + U) * (GP_FIT_ERR + 0.8 * acc))


def ffn1_sim(x1, w1, b1, acc=F32, rnd=bf16r):
    pre = ES.lin(x1, w1, b1, acc)
    return rnd(gelu_tail_fit(pre.to(acc)).to(F64)), rnd(pre), rnd(gelu_grad_fit(pre.to(acc)).to(F64))


def lse_ref(q, k, heads, scale=0.125):
    """One sequence: base-2 log of the softmax denominator per (head, query) -> (ref, bound) [heads, len].
    k_attention_train_fwd: lse = m c + log2(l), c = scale log2(e), l = sum_j exp2(fma(s_j, c, -m c)) over tiles with rescaling.
      score s_j: a 64-term fp32 dot product, |ds_j| <= 65 e24 (|q| |k|^T)_j          -> c |ds_j| in the exponent
      exponent fma(s, c, -fl(m c)): 2 e24 (|s_j c| + |m c|); v_exp_f32: 2 e24 relative  -> relative error ep_j of p_j (in l: its
      P-weighted mean <= max_j), the fp32 sum of len terms + the tile rescalings: (len + 8) e24 relative; all / ln 2 in log2
      log2(l), l in [1, len]: 2^-21 absolute + 2 e24 relative (v_log_f32);  fl(m c) and the final sum: e24 (|m c| + |lse|)."""
    n, H = q.shape
    d = H // heads
    qh, kh = (t.view(n, heads, d).transpose(0, 1) for t in (q, k))
    c = scale * ES.LOG2E
    s2 = c * (qh @ kh.transpose(1, 2))
    m = s2.max(-1).values
    l = torch.exp2(s2 - m[..., None]).sum(-1)
    ref = m + torch.log2(l)
    ep = c * 65 * E24 * (qh.abs() @ kh.abs().transpose(1, 2)) + math.log(2.0) * 2 * E24 * (s2.abs() + m.abs()[..., None]) + 2 * E24
    rel = ep.max(-1).values + (n + 8) * E24
    bound = rel / math.log(2.0) + 2.0 ** -21 + 2 * E24 * torch.log2(l) + E24 * (m.abs() + ref.abs()) + E24 * m.abs()
    return ref, bound


def lse_sim(q, k, heads, scale=0.125):
    n, H = q.shape
    d = H // heads
    qh, kh = (t.to(F32).view(n, heads, d).transpose(0, 1) for t in (q, k))
    c = np.float32(scale * ES.LOG2E)
    s = qh @ kh.transpose(1, 2)
    m = s.max(-1).values
    l = torch.exp2(s * c - (m * c)[..., None]).sum(-1)
    return (m * c + torch.log2(l)).to(F64)


# ---- LayerNorm backward -------------------------------------------------------------------------------------------------
def ln_bwd_ref(dya, dyb, y, g, eps, mask=None, in_mask=None, y_err=None):
    """LayerNorm backward of fp32 rows y (the pre-LayerNorm sums), incoming gradient dya (fp32) + dyb (bf16, optional):
         xh = (y - mean) rstd,  gd = g d,  dx = rstd (gd - mean(gd) - xh mean(gd xh)),  dXb = bf16(m dx)
       -> dict(dx, e32 [elementwise bound on the fp32 dx], sums (dbias = sum m dx, dgamma = sum d xh, dbeta = sum d), sums_err,
               sums_abs [sum of |terms|: the summation-order part of the sums' bound]).
    fp32 error model of k_layernorm_bwd / k_layernorm_bwd_rows, first order, D = H / 64 + 6 additions per row sum:
      d = dya + dyb             dd_i  = e24 |d_i| (one addition; 0 without dyb)
      xh                        exh_i = rstd ed_i + |xh_i| (er + e24), ed / er as in ln_fp32_err (mean, y - mean, variance, rsqrt)
      gd_i = d_i g_i            egd_i = |g_i| dd_i + e24 |gd_i|
      m1 = mean(gd)             em1   = mean(egd) + (D + 1) e24 mean|gd|
      m2 = mean(gd xh)          em2   = mean(egd |xh| + |gd| exh + e24 |gd xh|) + (D + 1) e24 mean|gd xh|
      t_i = gd_i - m1 - xh_i m2 et_i  = egd_i + em1 + exh_i |m2| + |xh_i| em2 + 3 e24 (|gd_i| + |m1| + |xh_i m2|)
      dx_i = rstd t_i           e32_i = rstd et_i + |dx_i| (er + e24)
      dgamma terms d_i xh_i: dd_i |xh_i| + |d_i| exh_i + e24 |d_i xh_i|;  dbeta terms d_i: dd_i;  dbias terms m dx: m e32 + e24 |m dx|."""
    H = y.shape[-1]
    D = H // 64 + 6
    mask = torch.ones_like(y) if mask is None else mask
    d = dya if dyb is None else dya + dyb
    dd = torch.zeros_like(d) if dyb is None else E24 * d.abs()
    if in_mask is not None:   # (the embedding backward: the incoming gradient goes through the embedding dropout first)
        d = d * in_mask
        dd = dd * in_mask + E24 * d.abs()
    mu = y.mean(-1, keepdim=True)
    c = y - mu
    y_err = torch.zeros_like(y) if y_err is None else y_err   # (what the kernel's fp32 y already carries: the embedding sum)
    em = D * E24 * y.abs().mean(-1, keepdim=True) + y_err.mean(-1, keepdim=True)
    ed = y_err + em + E24 * c.abs()
    var = (c * c).mean(-1, keepdim=True) + eps
    rstd = 1.0 / torch.sqrt(var)
    er = 0.5 * ((D + 3) * E24 + 2 * (c.abs() * ed).sum(-1, keepdim=True) / H / var) + 2 * E24
    xh = c * rstd
    exh = rstd * ed + xh.abs() * (er + E24)
    gd = d * g
    egd = g.abs() * dd + E24 * gd.abs()
    m1 = gd.mean(-1, keepdim=True)
    em1 = egd.mean(-1, keepdim=True) + (D + 1) * E24 * gd.abs().mean(-1, keepdim=True)
    gx = gd * xh
    m2 = gx.mean(-1, keepdim=True)
    em2 = (egd * xh.abs() + gd.abs() * exh + E24 * gx.abs()).mean(-1, keepdim=True) + (D + 1) * E24 * gx.abs().mean(-1, keepdim=True)
    t = gd - m1 - xh * m2
    et = egd + em1 + exh * m2.abs() + xh.abs() * em2 + 3 * E24 * (gd.abs() + m1.abs() + (xh * m2).abs())
    dx = rstd * t
    e32 = rstd * et + dx.abs() * (er + E24)
    dxh = d * xh
    return dict(dx=dx, e32=e32, mask=mask,
                sums=torch.stack([(mask * dx).sum(0), dxh.sum(0), d.sum(0)]),
                sums_err=torch.stack([(mask * e32 + E24 * (mask * dx).abs()).sum(0),
                                      (dd * xh.abs() + d.abs() * exh + E24 * dxh.abs()).sum(0), dd.sum(0)]),
                sums_abs=torch.stack([(mask * dx).abs().sum(0), dxh.abs().sum(0), d.abs().sum(0)]))


# ---- embedding backward -------------------------------------------------------------------------------------------------
EMB_BWD_BLOCKS = 512


def embed_bwd_ref(W, tok_id, tok_pos, dya, dyb, in_mask):
    """k_embed_bwd (+ k_embed_scatter_det) on the live rows: d = (G0 + dXb2) m, y = word + pos + type recomputed in fp32 (two
    roundings), dx = LayerNorm backward; word[id] += dx, pos[p] += dx, type[0] = sum dx, emb_ln_g = sum d xh, emb_ln_b = sum d.
    -> dict name -> (ref, bound).  Table rows: the sum of the rows' elementwise bounds + (count + 1) e24 sum|dx| -- any order of
    `count` additions (atomics or the owner's row order); the three column sums: depth e24 sum|terms| as for LayerNorm'."""
    a, c, t = W.word[tok_id.long()], W.pos[tok_pos.long()], W.type0
    y = a + c + t
    r = ln_bwd_ref(dya, dyb, y, W.emb_g, W.eps, in_mask=in_mask, y_err=2 * E24 * (a.abs() + c.abs() + t.abs()))
    dx, e32 = r["dx"], r["e32"]
    out = {}
    for name, idx, n in (("word_emb", tok_id.long(), W.word.shape[0]), ("pos_emb", tok_pos.long(), W.pos.shape[0])):
        z = lambda: torch.zeros(n, dx.shape[1], dtype=F64)
        ref, err, ab = z().index_add_(0, idx, dx), z().index_add_(0, idx, e32), z().index_add_(0, idx, dx.abs())
        cnt = torch.zeros(n, dtype=F64).index_add_(0, idx, torch.ones(len(idx), dtype=F64))[:, None]
        out[name] = (ref, err + (cnt + 1) * E24 * ab + 1e-300)
    rows = len(tok_id)
    blocks = min((rows + 3) // 4, EMB_BWD_BLOCKS)
    depth = -(-rows // (4 * blocks)) + 3 + -(-blocks // 16) + 16 + 1
    bound = r["sums_err"] + depth * E24 * r["sums_abs"] + 1e-300
    for i, name in ((0, "type_emb0"), (1, "emb_ln_g"), (2, "emb_ln_b")):
        out[name] = (r["sums"][i], bound[i])
    return out


def embed_bwd_sim(W, tok_id, tok_pos, dya, dyb, in_mask, count_once=False):
    """fp32 stand-in.  count_once: planted fault -- a repeated token id counted once in the word-table gradient."""
    y = ((W.word[tok_id.long()].to(F32) + W.pos[tok_pos.long()].to(F32)) + W.type0.to(F32)).to(F64)
    d = ((dya.to(F32) + dyb.to(F32)) * in_mask.to(F32)).to(F64)
    dx, _, sums = ln_bwd_sim(d, None, y, W.emb_g, W.eps)
    word = torch.zeros(W.word.shape, dtype=F32)
    if count_once:
        word[tok_id.long()] = dx.to(F32)
    else:
        word.index_add_(0, tok_id.long(), dx.to(F32))
    pos = torch.zeros(W.pos.shape, dtype=F32).index_add_(0, tok_pos.long(), dx.to(F32))
    return dict(word_emb=word.to(F64), pos_emb=pos.to(F64), type_emb0=sums[0], emb_ln_g=sums[1], emb_ln_b=sums[2])


def ln_bwd_sim(dya, dyb, y, g, eps, mask=None, rnd=bf16r, add_b=True, skip_row=None, mask_for_sums=None):
    """The kernel's arithmetic in fp32 -> (dXf, dXb, sums [3, H]).  Planted faults: add_b=False (the bf16 half of the incoming
    gradient not added), skip_row (one row not processed: its outputs stay as they were = NaN here, the sums lack it)."""
    f = lambda t: t.to(F32)
    d = f(dya) if (dyb is None or not add_b) else f(dya) + f(dyb)
    y, g = f(y), f(g)
    H = y.shape[-1]
    c = y - y.sum(-1, keepdim=True) / H
    rstd = torch.rsqrt((c * c).sum(-1, keepdim=True) / H + np.float32(eps))
    xh = c * rstd
    gd = d * g
    m1, m2 = gd.sum(-1, keepdim=True) / H, (gd * xh).sum(-1, keepdim=True) / H
    dx = rstd * (gd - m1 - xh * m2)
    mk = torch.ones_like(dx) if mask is None else f(mask)
    dm = dx * mk
    keep = torch.ones(y.shape[0], dtype=torch.bool)
    if skip_row is not None:
        keep[skip_row] = False
    k = keep[:, None].to(F32)
    sums = torch.stack([(dm * k).sum(0), (d * xh * k).sum(0), (d * k).sum(0)]).to(F64)
    dxf, dxb = dx.to(F64), rnd(dm.to(F64))
    if skip_row is not None:
        dxf[skip_row], dxb[skip_row] = float("nan"), float("nan")
    return dxf, dxb, sums


def ln_sum_depth(rows):
    """Longest chain of fp32 additions behind one LayerNorm-backward partial sum: a wave's rows in sequence, the four waves of a
    workgroup, k_reduce_multi's 16 thread rows over the workgroups' partials, their fold, the add into the gradient."""
    blocks = min((rows + 3) // 4, LN_BWD_BLOCKS)
    return -(-rows // (4 * blocks)) + 3 + -(-blocks // 16) + 16 + 1


def colsum_depth(rows, chunks):
    """k_colsum_bf16 / k_dgelu_colsum: 8 row lanes over a chunk's rows, their fold, k_reduce_multi over the chunks."""
    return -(-(-(-rows // chunks)) // 8) + 8 + -(-chunks // 16) + 16 + 1


def colsum_chunks(rows):
    return COLSUM_CHUNKS if rows >= 2048 else 8


def nan_max(t):
    """max that does not hide a NaN."""
    return float("inf") if bool(torch.isnan(t).any()) else float(t.max())


def ln_bwd_ratios(ref, dxf, dxb, sums, rows):
    """-> dict of ratios (each must be < 1) of a LayerNorm backward's outputs against ln_bwd_ref's result."""
    r = {}
    if dxf is not None:
        r["dXf"] = nan_max((dxf - ref["dx"]).abs() / (ref["e32"] + 1e-300))
    if dxb is not None:
        m = ref["mask"]
        r["dXb"] = nan_max((dxb - m * ref["dx"]).abs() / (U * (m * ref["dx"]).abs() + (1 + U) * m * ref["e32"] + 1e-300))
    if sums is not None:
        bound = ref["sums_err"] + ln_sum_depth(rows) * E24 * ref["sums_abs"]
        for i, n in enumerate(("dbias", "dgamma", "dbeta")):
            if sums[i] is not None:
                r[n] = nan_max((sums[i] - ref["sums"][i]).abs() / (bound[i] + 1e-300))
    return r


# ---- data-gradient GEMMs ------------------------------------------------------------------------------------------------
def dgrad_ref(dy, w, gp=None):
    """dX = dY W (W [N_out_of_forward, K_in]: the forward's weight; the kernel reads its transposed bf16 copy), optionally times the
    saved gelu' image -> (ref, bound) for ONE bf16 rounding of the fp32 result."""
    y = dy @ w
    acc = (dy.shape[1] + 1) * E24 * (dy.abs().to(F32) @ w.abs().to(F32)).to(F64) * 1.001
    if gp is not None:
        y = y * gp
        acc = acc * gp.abs() + E24 * y.abs()
    return y, U * (y.abs() + acc) + acc


def dgrad_sim(dy, w, gp=None, acc=F32, rnd=bf16r):
    y = (dy.to(acc) @ w.to(acc))
    if gp is not None:
        y = y * gp.to(acc)
    return rnd(y.to(F64))


def dgelu_chain(dyb, w2, hpre, acc=F64, rnd=bf16r, grad_of=None):
    """gelu_gp 0 and the CLS tail: t = bf16(dYb W2) (unobservable: rewritten in place), dHpre = bf16(t gelu'(Hpre)).
    grad_of: planted fault -- gelu' of another tensor (Hm) instead of the pre-activation."""
    t = rnd((dyb.to(acc) @ w2.to(acc)).to(F64))
    x = hpre if grad_of is None else grad_of
    return rnd((t.to(acc) * gelu_grad_fit(x.to(acc))).to(F64))


def dgelu_ref(dyb, w2, hpre):
    """The same chain against the exact product s gelu'(Hpre), s = dYb W2 -> (ref, bound), two roundings deep:
      t = bf16(fp32 s):        |t - s| <= u (|s| + acc) + acc =: bt,  acc = (K + 1) e24 |dYb| |W2|
      g = the fp32 gelu' fit:   |g - gelu'| <= 4e-5 (GP_FIT_ERR)
      p = fl(t g):              |p - ref| <= bt (|gelu'| + 4e-5) + |s| 4e-5 + e24 |ref| =: e;   out = bf16(p): u (|ref| + e) + e."""
    s = dyb @ w2
    acc = (dyb.shape[1] + 1) * E24 * (dyb.abs().to(F32) @ w2.abs().to(F32)).to(F64) * 1.001
    bt = U * (s.abs() + acc) + acc
    g = gelu_grad_exact(hpre)
    ref = s * g
    e = bt * (g.abs() + GP_FIT_ERR) + s.abs() * GP_FIT_ERR + E24 * ref.abs()
    return ref, U * (ref.abs() + e) + e + 1e-300


def f32_sum_ref(x, w, addend, slices):
    """addend + x W as one fp32 sum cut into `slices` slab slices (the compact dX1) -> (ref, bound)."""
    y = x @ w + addend
    a = (x.abs().to(F32) @ w.abs().to(F32)).to(F64) * 1.001 + addend.abs()
    return y, (x.shape[1] + slices + 2) * E24 * a


# ---- attention backward ----------------------------------------------------------------------------------------------------
def attn_bwd_chain(q, k, v, do, lse2, o, heads, acc=F64, o32_row0=None, scale=0.125, fault=None, mask=None, perm=None):
    """One sequence through k_attention_bwd_dq / dkv / fused (no probability dropout): q, k, v, do, o [n, H] (the kernel's bf16
    operands), lse2 [n, heads] (the forward's saved base-2 LSE) -> dQKV [n, 3H], with the kernels' rounding points:
       p = exp2(s c - lse2),  D = do . o (o: the bf16 ctx; query 0 from the fp32 row o32_row0 in the CLS tail),
       dS = bf16(p (do v^T - D) scale),  dQ = bf16(dS k),  dK = bf16(dS^T q),  dV = bf16(bf16(p)^T do);  sums in `acc`.
    mask [heads, n, n] (probability dropout, 0 or 1 / keep): dV from bf16(p m), dS from p (m do v^T - D); D = do . o as before
    (o is the dropped forward's output).  perm: the sequence's tokens processed in this order (same function, another fp32
    summation order over keys and queries; the result comes back in the original order).
    fault: 'd_other_head' (D from the next head's ctx), 'no_scale' (scale missing on dS), 'kv_tile' (keys 64..127 missing from
    dK / dV)."""
    n, H = q.shape
    d = H // heads
    if perm is not None:
        inv = torch.argsort(perm)
        m2 = None if mask is None else mask[:, perm][:, :, perm]
        return attn_bwd_chain(q[perm], k[perm], v[perm], do[perm], lse2[perm], o[perm], heads, acc,
                              None if o32_row0 is None else o32_row0, scale, fault, m2, None)[inv] if o32_row0 is None or int(perm[0]) == 0 \
            else None
    hd = lambda t: t.to(acc).view(n, heads, d).transpose(0, 1)
    qh, kh, vh, doh, oh = (hd(t) for t in (q, k, v, do, o))
    if fault == "d_other_head":
        oh = oh.roll(1, 0)
    c = scale * ES.LOG2E
    p = torch.exp2((qh @ kh.transpose(1, 2)) * c - lse2.to(acc).T[..., None])
    D = (doh * oh).sum(-1)
    if o32_row0 is not None:
        D[:, 0] = (doh[:, 0] * o32_row0.to(acc).view(heads, d)).sum(-1)
    dp = doh @ vh.transpose(1, 2)
    pd = p
    if mask is not None:
        dp, pd = dp * mask.to(acc), p * mask.to(acc)
    ds = p * (dp - D[..., None])
    if fault != "no_scale":
        ds = ds * scale
    rb = lambda t: t.to(BF16).to(acc)
    ds, pb = rb(ds), rb(pd)
    dq, dk, dv = ds @ kh, ds.transpose(1, 2) @ qh, pb.transpose(1, 2) @ doh
    if fault == "kv_tile" and n > 64:
        dk[:, 64:128], dv[:, 64:128] = 0, 0
    back = lambda t: bf16r(t.transpose(0, 1).reshape(n, H).to(F64))
    return torch.cat([back(dq), back(dk), back(dv)], 1)


def attn_bwd_all(qkv, dctx, lse, ctx, lens, heads, acc=F64, c_ctx32=None, fault=None, masks=None, reorder=False):
    """attn_bwd_chain over the sequences of the live-row matrices; lse [rows_live, heads]; c_ctx32 [B, H] in the CLS tail;
    masks: per sequence [heads, n, n] or None; reorder: every sequence's tokens in reversed order but the first (another fp32
    summation order: what the stand-in kernel uses, so that it is not the reference pair's own fp32 member)."""
    H = ctx.shape[1]
    outs, o = [], 0
    for b, n in enumerate(lens):
        sl = slice(o, o + n)
        perm = torch.cat([torch.zeros(1, dtype=torch.long), torch.arange(n - 1, 0, -1)]) if reorder and n > 2 else None
        outs.append(attn_bwd_chain(qkv[sl, :H], qkv[sl, H:2 * H], qkv[sl, 2 * H:], dctx[sl], lse[sl], ctx[sl], heads, acc,
                                   None if c_ctx32 is None else c_ctx32[b], fault=fault,
                                   mask=None if masks is None else masks[b], perm=perm))
        o += n
    return torch.cat(outs, 0)


def attn_bwd_tail_ref(qkv, do0, lse0, o32, heads, mask0=None, scale=0.125):
    """The attention backward of the CLS tail for one sequence: only query 0 carries gradient, so dK and dV are single products
    (no sum to average a rounding away) and a reference pair would differ by rare bf16 flips only: the bound is derived.
    qkv [n, 3H], do0 / o32 [H] (dO and the fp32 context row of query 0), lse0 [heads], mask0 [heads, n] -> (ref, bound) [n, 3H].
      p_k = exp2(s_k c - lse):  relative ep_k = c 65 e24 (|q0| |k_k|) + ln2 2 e24 (|s_k c| + |lse|) + 2 e24
      dp_k = do0 . v_k (64-term fp32 dot): 65 e24 (|do0| |v_k|), times m_k: + e24;   D = do0 . o32: 130 e24 (|do0| |o32|)
      dS_k = p_k (m_k dp_k - D) scale: eds_k = scale p_k (ep_k |t_k| + et_k) + 2 e24 |dS_k|;  bf16: bds_k = u |dS_k| + (1 + u) eds_k
      dK_k = bf16(dS_k q0):  u |ref| + (1 + u) bds_k |q0|;   dV_k = bf16(bf16(p_k m_k) do0) likewise with p m (ep_k + e24)
      dQ_0 = bf16(sum_k dS_k k_k):  u |ref| + (1 + u) (sum_k bds_k |k_k| + (n + 1) e24 sum_k |dS_k| |k_k|);  every other dQ row: 0."""
    n, H3 = qkv.shape
    H = H3 // 3
    d = H // heads
    hd = lambda t: t.view(n, heads, d).transpose(0, 1)                    # [h, n, d]
    kh, vh = hd(qkv[:, H:2 * H]), hd(qkv[:, 2 * H:])
    q0, g0, o0 = qkv[0, :H].view(heads, 1, d), do0.view(heads, 1, d), o32.view(heads, 1, d)
    m = torch.ones(heads, n, dtype=F64) if mask0 is None else mask0
    c = scale * ES.LOG2E
    dot = lambda a, b: (a * b).sum(-1)                                    # [h, 1, d] x [h, n, d] -> [h, n]
    s2 = c * dot(q0, kh)
    l0 = lse0.view(heads, 1)
    p = torch.exp2(s2 - l0)
    ep = c * 65 * E24 * dot(q0.abs(), kh.abs()) + math.log(2.0) * 2 * E24 * (s2.abs() + l0.abs()) + 2 * E24
    dpm = dot(g0, vh) * m
    edpm = 65 * E24 * dot(g0.abs(), vh.abs()) * m + E24 * dpm.abs()
    D = dot(g0, o0)                                                       # [h, 1]
    eD = 130 * E24 * dot(g0.abs(), o0.abs())
    t = dpm - D
    et = edpm + eD + E24 * t.abs()
    ds = p * t * scale
    bds = U * ds.abs() + (1 + U) * (scale * p * (ep * t.abs() + et) + 2 * E24 * ds.abs())
    pd = p * m
    bpd = U * pd + (1 + U) * pd * (ep + E24)
    # fp32 underflow: v_exp_f32 returns 0 below 2^-126 where fp64 keeps 1e-40 (saturated heads: p = exp2(-140)), and products of
    # such values leave the bf16 range; with |t|, |q0|, |do0|, |k| < 2^8 what a flushed factor can move is below 2^-100 absolute
    two = lambda ref, b: U * ref.abs() + (1 + U) * b + 2.0 ** -100
    dk, dv = ds[..., None] * q0, pd[..., None] * g0                       # [h, n, d]
    bk, bv = two(dk, bds[..., None] * q0.abs()), two(dv, bpd[..., None] * g0.abs())
    dq0 = (ds[..., None] * kh).sum(1)                                     # [h, d]
    bq0 = two(dq0, (bds[..., None] * kh.abs()).sum(1) + (n + 1) * E24 * (ds.abs()[..., None] * kh.abs()).sum(1))
    back = lambda x: x.transpose(0, 1).reshape(n, H)
    dq, bq = torch.zeros(n, H, dtype=F64), torch.zeros(n, H, dtype=F64)
    dq[0], bq[0] = dq0.reshape(H), bq0.reshape(H)
    return torch.cat([dq, back(dk), back(dv)], 1), torch.cat([bq, back(bk), back(bv)], 1)


def slice_metrics(got, ref, rel=2 * U, width=64):
    """tail_metrics normalised per (token, head, Q / K / V third) slice of `width` elements: one wrong slice shows instead of
    being averaged into its row.  The scale of a slice is its reference's rms, but no less than one bf16 roundoff (u) of its
    token's whole row: a slice that is nothing but cancellation noise (dS = P (dP - D) of a one-token sequence or a saturated
    head is exactly zero in fp64 and a few fp32 ulps of D otherwise) is measured on the scale its neighbours are rounded at."""
    n = ref.shape[0]
    g, r = got.reshape(n, -1, width), ref.reshape(n, -1, width)
    rms = r.pow(2).mean(-1, keepdim=True).sqrt()
    row = ref.pow(2).mean(-1).sqrt()[:, None, None]
    scale = torch.maximum(rms, U * row) + 1e-300
    if bool(torch.isnan(g).any()):
        return float("inf"), float("inf")
    c = float((((g - r).abs() - rel * r.abs()).clamp(min=0) / scale).max())
    return c, float((g != r).double().mean())


# ---- parameter gradients ------------------------------------------------------------------------------------------------
def wgrad_ref(dy, x, slices=1):
    """dW = dY^T X over ALL packed rows -> (ref, bound = (rows + slices + 2) e24 |dY|^T |X|)."""
    ref = dy.T @ x
    a = (dy.abs().to(F32).T @ x.abs().to(F32)).to(F64) * 1.001
    return ref, (dy.shape[0] + slices + 2) * E24 * a + 1e-300


def wgrad_slices(rows, tail_split=0):
    """Slab slices of wgrad_launch (csrc/train.hip) below 512 K steps of 64 rows: 1, or for the last batch of the pass
    (layer 0's four matrices, tail_split = 2) min(2, steps / 32)."""
    steps = -(-rows // 64)
    assert steps < 512
    return max(1, min(tail_split, steps // 32)) if tail_split > 1 else 1


def wgrad_sim(dy, x, skip=None, trunc_octet=None):
    """fp32 product; planted faults: skip = (first row, rows) of the contraction left out; trunc_octet = (n, k0): 8 elements lost."""
    if skip is not None:
        keep = torch.ones(dy.shape[0], dtype=torch.bool)
        keep[skip[0]:skip[0] + skip[1]] = False
        dy, x = dy[keep], x[keep]
    o = (dy.to(F32).T @ x.to(F32)).to(F64)
    if trunc_octet is not None:
        o[trunc_octet[0], trunc_octet[1]:trunc_octet[1] + 8] = 0
    return o


def colsum_ref(m, chunks):
    ref = m.sum(0)
    return ref, colsum_depth(m.shape[0], chunks) * E24 * m.abs().sum(0) + 1e-300


def ratio(got, ref, bound):
    return nan_max((got - ref).abs() / (bound + 1e-300))


# ---- the library under the stages (GPU) ------------------------------------------------------------------------------------
TRAIN_DEFAULTS = dict(gelu_gp=1, attn_bwd_fused=1, ln_bwd_rows=2, embed_bwd_deterministic=0, gemm_tile_policy=0,
                      train_bwd_stop_layer=-1)
LAYER_SAVE = ("Xin", "QKV", "ctx", "LSE", "Mbits", "X1", "Hpre", "Hm", "Y1", "Y2")
LAYER_BWD = ("dYb", "dHpre", "dYb2", "dQKV")
GLOBALS = ("Xout", "cls_b", "cls_y", "cls_f", "head_y", "G0", "G1", "Drow", "dcls_y", "dcls_f", "dhead_y", "dhead_yb", "dXb1", "dXb2",
           "dctx", "c_ctx", "c_xin", "c_X1", "c_Hpre", "c_Hm", "c_Y1", "c_ctx32", "c_dYb", "c_dHpre", "c_dYb2", "c_dctx", "c_dX1f",
           "c_dY1")


def train_layout(c, rows, B):
    """{name: byte offset} from convdr_encoder_train_debug_layout; per-layer regions as 'Xin/0', 'dYb/1', ...; 'ldt', 'Tp'."""
    from convdr_amd import _lib
    n = 3 + 14 * c.layers + len(GLOBALS) + 2
    lay = (C.c_int64 * n)()
    got = _lib.lib().convdr_encoder_train_debug_layout(C.byref(c), rows, B, lay, n)
    assert got == n, (got, n, _lib.lib().convdr_last_error())
    names = ["tok_id", "tok_pos", "order"]
    names += ["%s/%d" % (k, l) for l in range(c.layers) for k in LAYER_SAVE]
    names += ["%s/%d" % (k, l) for l in range(c.layers) for k in LAYER_BWD]
    names += list(GLOBALS) + ["ldt", "Tp"]
    return dict(zip(names, list(lay)))


def set_options(**kw):
    from convdr_amd import _lib
    for k, v in kw.items():
        assert k in TRAIN_DEFAULTS, k
        _lib.check(_lib.lib().convdr_set_option(k.encode(), int(v)), "convdr_set_option")


def grad_param_names(NL):
    names = ["word_emb", "pos_emb", "type_emb", "emb_ln_g", "emb_ln_b"]
    for l in range(NL):
        names += ["%s/%d" % (k, l) for k in ("wq", "wk", "wv", "bq", "bk", "bv", "wo", "bo", "ln1_g", "ln1_b", "w1", "b1", "w2", "b2",
                                             "ln2_g", "ln2_b")]
    return names + ["head_w", "head_b", "head_ln_g", "head_ln_b"]


def run_train(model, ids, lens, pool_mean, drop=None, opts=(), seed=0):
    """One training forward and NL + 2 backwards of `model` (RobertaDot_NLL_LN on the GPU) through the C ABI with packed weights:
    the forward on a workspace pre-filled with 0xFF bytes; convdr_encoder_backward_fresh stopped at NL, .., 0 into gradient buffers
    of random contents (embedding tables zero: those accumulate always); one full convdr_encoder_backward into zeros.
    -> dict: 'fwd' {name: tensor} (all packed rows; fp64, Mbits int32), 'bwd' {stop: {name: tensor}}, 'grads' {stop or 'full':
    {param: fp64}}, 'd_out', 'live', 'cu', 'rows', 'cfg' (H, I, heads, NL, E).  Asserts the determinism premise."""
    from convdr_amd import _lib
    from convdr_amd.train import _packed_t, _tower_params
    L_ = _lib.lib()
    dev = torch.device("cuda")
    tower, head = model.roberta, (model.embeddingHead, model.norm)
    lens = np.asarray(lens, np.int32)
    B = len(lens)
    cu = np.zeros(B + 1, np.int32)
    np.cumsum((lens + 7) // 8 * 8, out=cu[1:])
    rows, max_len = int(cu[-1]), int(lens.max())
    live = torch.from_numpy(np.concatenate([cu[b] + np.arange(lens[b]) for b in range(B)]).astype(np.int64))
    o = dict(TRAIN_DEFAULTS)
    o.update(dict(opts))
    res = {"bwd": {}, "grads": {}, "live": live, "cu": cu, "rows": rows}
    try:
        with torch.cuda.device(dev):
            set_options(**o)
            c0, w, keep = tower.packed(head)
            wt, head_t = _packed_t(tower, head)
            c = _lib.EncoderConfig.from_buffer_copy(c0)
            c.pool_mean = int(pool_mean)
            H, I, NL, E, heads = c.hidden, c.intermediate, c.layers, c.out_dim, c.heads
            res["cfg"] = dict(H=H, I=I, NL=NL, E=E, heads=heads, pool_mean=bool(pool_mean))
            need = L_.convdr_encoder_train_workspace_bytes(C.byref(c), rows, B)
            ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
            out = torch.full((B, E), float("nan"), dtype=torch.float32, device=dev)
            cu_d, lens_d = torch.from_numpy(cu).to(dev), torch.from_numpy(lens).to(dev)
            ids_d = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(dev)
            dr = None if drop is None else C.byref(_lib.Dropout(float(drop[0]), float(drop[1]), int(drop[2]) & 0xffffffff))
            _lib.check(L_.convdr_encoder_train_forward(C.byref(c), C.byref(w), _lib.ptr(ids_d), 0, None, B, ids_d.shape[1],
                                                       _lib.ptr(cu_d), _lib.ptr(lens_d), rows, max_len, _lib.ptr(ws), ws.numel(),
                                                       _lib.ptr(out), dr, _lib.stream_ptr()), "convdr_encoder_train_forward")
            torch.cuda.synchronize()
            assert int(ws[:4].view(torch.int32)[0]) == 0, "status word"
            lay = train_layout(c, rows, B)
            ldt = int(lay["ldt"])

            def buf(name, n, dtype, raw=False):
                off = lay[name]
                assert off > 0, name
                size = n * torch.empty((), dtype=dtype).element_size()
                assert off + size <= need, name
                t = ws[off:off + size].view(dtype).cpu()
                return t if raw else t.to(F64)

            Bp = B
            f = res["fwd"] = {"out": out.cpu().to(F64)}
            f["tok_id"], f["tok_pos"] = buf("tok_id", rows, torch.int32, True), buf("tok_pos", rows, torch.int32, True)
            for l in range(NL):
                tail = l == NL - 1 and not pool_mean
                f["Xin/%d" % l] = buf("Xin/%d" % l, rows * H, BF16).view(rows, H)
                f["QKV/%d" % l] = buf("QKV/%d" % l, rows * 3 * H, BF16).view(rows, 3 * H)
                f["ctx/%d" % l] = buf("ctx/%d" % l, rows * H, BF16).view(rows, H)
                f["LSE/%d" % l] = buf("LSE/%d" % l, heads * ldt, torch.float32).view(heads, ldt)[:, :rows]
                if drop is not None and drop[1] > 0 and max_len <= 256:   # (ATTF_MAX_LEN: the forward keeps its dropout bits)
                    f["Mbits/%d" % l] = buf("Mbits/%d" % l, heads * 8 * ldt, torch.int32, raw=True).view(heads, 8, ldt)
                if tail:
                    assert all(lay["%s/%d" % (k, l)] == -1 for k in ("X1", "Hpre", "Hm", "Y1", "Y2"))
                    continue
                f["X1/%d" % l] = buf("X1/%d" % l, rows * H, BF16).view(rows, H)
                f["Hm/%d" % l] = buf("Hm/%d" % l, rows * I, BF16).view(rows, I)
                if o["gelu_gp"]:
                    f["Gp/%d" % l] = ES.decode_blocked(buf("Hpre/%d" % l, (rows + 31) // 32 * 32 * I, BF16), rows, I)
                else:
                    f["Hpre/%d" % l] = buf("Hpre/%d" % l, rows * I, BF16).view(rows, I)
                f["Y1/%d" % l] = buf("Y1/%d" % l, rows * H, torch.float32).view(rows, H)
                f["Y2/%d" % l] = buf("Y2/%d" % l, rows * H, torch.float32).view(rows, H)
            f["cls_b"], f["cls_f"] = buf("cls_b", Bp * H, BF16).view(B, H), buf("cls_f", Bp * H, torch.float32).view(B, H)
            f["head_y"] = buf("head_y", Bp * E, torch.float32).view(B, E)
            if pool_mean:
                f["Xout"] = buf("Xout", rows * H, BF16).view(rows, H)
            else:
                f["cls_y"] = buf("cls_y", Bp * H, torch.float32).view(B, H)
                for k, n, dt in (("c_ctx", H, BF16), ("c_xin", H, BF16), ("c_X1", H, BF16), ("c_Hpre", I, BF16), ("c_Hm", I, BF16),
                                 ("c_Y1", H, torch.float32), ("c_ctx32", H, torch.float32)):
                    f[k] = buf(k, B * n, dt).view(B, n)

            # ---- backwards ----
            g0 = torch.Generator().manual_seed(seed + 1)
            d_out = (torch.randn(B, E, generator=g0) * 0.05).float()
            res["d_out"] = d_out.to(F64)
            d_out_d = d_out.to(dev)
            params = _tower_params(tower, head)
            names = grad_param_names(NL)
            assert len(names) == len(params)
            sizes = [p.numel() for p in params]

            def backward(stop, fresh):
                set_options(train_bwd_stop_layer=stop)
                arena = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
                if fresh:   # every stored gradient must overwrite this
                    arena[sum(sizes[:5]):] = torch.randn(sum(sizes[5:]), generator=torch.Generator().manual_seed(seed + 2)).to(dev)
                views = list(arena.split_with_sizes(sizes))
                ptr = [v.data_ptr() for v in views]
                lg = (_lib.LayerGrads * NL)()
                for i in range(NL):
                    b, g = 5 + 16 * i, lg[i]
                    g.wqkv, g.bqkv = ptr[b], ptr[b + 3]
                    g.wo, g.bo, g.ln1_g, g.ln1_b = ptr[b + 6], ptr[b + 7], ptr[b + 8], ptr[b + 9]
                    g.w1, g.b1, g.w2, g.b2 = ptr[b + 10], ptr[b + 11], ptr[b + 12], ptr[b + 13]
                    g.ln2_g, g.ln2_b = ptr[b + 14], ptr[b + 15]
                gr = _lib.EncoderGrads()
                gr.word_emb, gr.pos_emb, gr.type_emb, gr.emb_ln_g, gr.emb_ln_b = ptr[:5]
                gr.layers = C.cast(lg, C.POINTER(_lib.LayerGrads))
                b = 5 + 16 * NL
                gr.head_w, gr.head_b, gr.head_ln_g, gr.head_ln_b = ptr[b:b + 4]
                fn = L_.convdr_encoder_backward_fresh if fresh else L_.convdr_encoder_backward
                _lib.check(fn(C.byref(c), C.byref(w), wt, _lib.ptr(cu_d), _lib.ptr(lens_d), C.c_void_p(head_t), B, rows, max_len,
                              _lib.ptr(ws), ws.numel(), _lib.ptr(d_out_d), C.byref(gr), dr, _lib.stream_ptr()), "convdr_encoder_backward")
                torch.cuda.synchronize()
                set_options(train_bwd_stop_layer=-1)
                return {n: v.view(p.shape).cpu().to(F64) for n, v, p in zip(names, views, params)}

            def snap(stop):
                s = {}
                for k, n, dt in (("G0", H, torch.float32), ("G1", H, torch.float32), ("dXb1", H, BF16), ("dXb2", H, BF16), ("dctx", H, BF16)):
                    s[k] = buf(k, rows * n, dt).view(rows, n)
                for l in range(max(stop, 0), NL):
                    tail = l == NL - 1 and not pool_mean
                    for k, n in (("dYb", H), ("dHpre", I), ("dYb2", H), ("dQKV", 3 * H)):
                        if tail and k != "dQKV":
                            continue
                        s["%s/%d" % (k, l)] = buf("%s/%d" % (k, l), rows * n, BF16, raw=True).view(rows, n)
                for k, n, dt in (("dhead_y", E, torch.float32), ("dhead_yb", E, BF16), ("dcls_f", H, torch.float32)):
                    s[k] = buf(k, B * n, dt).view(B, n)
                if not pool_mean:
                    for k, n, dt in (("dcls_y", H, torch.float32), ("c_dYb", H, BF16), ("c_dHpre", I, BF16), ("c_dYb2", H, BF16),
                                     ("c_dctx", H, BF16), ("c_dX1f", H, torch.float32), ("c_dY1", H, torch.float32)):
                        s[k] = buf(k, B * n, dt).view(B, n)
                return s

            prev = None
            for stop in range(NL, -1, -1):
                res["grads"][stop] = backward(stop, fresh=True)
                s = res["bwd"][stop] = snap(stop)
                if prev is not None:   # the premise of teacher forcing: what the run above left in the per-layer buffers is what
                    for k, v in prev.items():   # this run's layers above the stop wrote again, byte for byte
                        if "/" in k:
                            assert torch.equal(v.view(torch.int16), s[k].view(torch.int16)), "backward not deterministic: %s" % k
                prev = s
            res["grads"]["full"] = backward(-1, fresh=False)
            for s in res["bwd"].values():
                for k in list(s):
                    if "/" in k:
                        s[k] = s[k].to(F64)
    finally:
        set_options(**TRAIN_DEFAULTS)
    return res


# ---- the walk over the stages of one run ---------------------------------------------------------------------------------
class Head:
    """fp64 copies of the packed head: Linear (bf16 weight) + LayerNorm."""

    def __init__(self, model):
        d = lambda p: p.detach().cpu().float().to(F64)
        self.w, self.b = bf16r(d(model.embeddingHead.weight)), d(model.embeddingHead.bias)
        self.g, self.beta, self.eps = d(model.norm.weight), d(model.norm.bias), float(np.float32(model.norm.eps))


class Report:
    """Collected checks: derived ratios (bar 1), measured pairs (value, bar) and exact equalities."""

    def __init__(self):
        self.items = []

    def derived(self, name, value):
        self.items.append((name, float(value), 1.0))

    def measured(self, name, value, bar):
        self.items.append((name, float(value), float(bar)))

    def exact(self, name, ok):
        self.items.append((name, 0.0 if ok else float("inf"), 0.5))

    def failures(self):
        return [(n, v, b) for n, v, b in self.items if not v < b]


def _bf16_ratio(got, ref, e32):
    return nan_max((got - ref).abs() / (U * ref.abs() + (1 + U) * e32 + 1e-300))


def check_forward(res, W, HD, lens, drop, rep, memo_key=None):
    """Every forward stage of run `res` against its reference (W: ES.Weights, HD: Head)."""
    f, lv, cu, cfg = res["fwd"], res["live"], res["cu"], res["cfg"]
    H, I, NL, heads = cfg["H"], cfg["I"], cfg["NL"], cfg["heads"]
    lens = [int(n) for n in lens]
    starts = torch.as_tensor(cu[:-1].astype(np.int64))
    p_att = 0.0 if drop is None else drop[1]
    mk = lambda site, l, rows: mask_rows(drop, site, l, rows, H)
    M = lambda tag, ts, fn: ES.memo((tag, memo_key), ts, fn) if memo_key is not None else fn()
    # A
    ref, e32 = ES.embed_ref(W, f["tok_id"][lv], f["tok_pos"][lv])
    m = mk(OD.SITE_EMB, 0, lv.numpy())
    rep.derived("fwd/A", _bf16_ratio(f["Xin/0"][lv], m * ref, m * e32))
    # first 128 queries of every sequence (all the CLS tail's attention computes), as indices into the live rows
    q128 = torch.cat([o + torch.arange(min(n, 128)) for o, n in zip(np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)])
    for l in range(NL):
        L = W.layers[l]
        tail = l == NL - 1 and not cfg["pool_mean"]
        x, qkv, ctx = f["Xin/%d" % l][lv], f["QKV/%d" % l][lv], f["ctx/%d" % l][lv]
        y, bound = M("B%d" % l, [x], lambda: ES.proj_ref(x, L["wqkv"], L["bqkv"]))
        rep.derived("fwd/l%d/B" % l, ratio(qkv, y, bound))
        sel = q128 if tail else torch.arange(len(lv))
        lse, lse_b = M("LSE%d" % l, [qkv], lambda: ES.per_sequence(
            lens, lambda a: tuple(t.T for t in lse_ref(a[:, :H], a[:, H:2 * H], heads)), qkv))
        rep.derived("fwd/l%d/LSE" % l, ratio(f["LSE/%d" % l].T[lv][sel], lse[sel], lse_b[sel]))
        if p_att == 0:
            ref, bound, _ = M("C%d" % l, [qkv], lambda: ES.per_sequence(
                lens, lambda a: ES.attention_ref(a[:, :H], a[:, H:2 * H], a[:, 2 * H:], heads), qkv))
        else:   # the oracle's probability mask; where the forward kept its bits (Mbits), they must be the same mask bit for bit
            masks = [att_mask_seq(drop, l, int(cu[b]), n, heads) for b, n in enumerate(lens)]
            if "Mbits/%d" % l in f:
                nq = [min(n, 128) if tail else n for n in lens]
                rep.exact("fwd/l%d/Mbits" % l, all(torch.equal(decode_mbits(f["Mbits/%d" % l], int(cu[b]), n)[:, :nq[b]],
                                                               masks[b][:, :nq[b]] != 0) for b, n in enumerate(lens)))
            outs, o = [], 0
            for b, n in enumerate(lens):
                a = qkv[o:o + n]
                outs.append(attention_ref_drop(a[:, :H], a[:, H:2 * H], a[:, 2 * H:], heads, masks[b]))
                o += n
            ref, bound = torch.cat([x[0] for x in outs]), torch.cat([x[1] for x in outs])
        rep.derived("fwd/l%d/C" % l, ratio(ctx[sel], ref[sel], bound[sel]))
        if tail:
            rep.exact("fwd/l%d/c_xin" % l, torch.equal(f["c_xin"], f["Xin/%d" % l][starts]))
            rep.exact("fwd/l%d/c_ctx" % l, torch.equal(f["c_ctx"], f["ctx/%d" % l][starts]))
            rep.exact("fwd/l%d/c_ctx32" % l, torch.equal(bf16r(f["c_ctx32"]), f["c_ctx"]))
            rows_c = cu[:-1]
            ctx, x, s = f["c_ctx"], f["c_xin"], CLS_MAX_SPLIT
            Y1, X1, Hm, Hpre, Gp, Y2 = f["c_Y1"], f["c_X1"], f["c_Hm"], f["c_Hpre"], None, f["cls_y"]
        else:
            rows_c, s = lv.numpy(), 0
            Y1, X1, Hm, Y2 = (f["%s/%d" % (k, l)][lv] for k in ("Y1", "X1", "Hm", "Y2"))
            Hpre = f["Hpre/%d" % l][lv] if "Hpre/%d" % l in f else None
            Gp = f["Gp/%d" % l][lv] if "Gp/%d" % l in f else None
        m1, m2 = mk(OD.SITE_ATTN_OUT, l, rows_c), mk(OD.SITE_FFN_OUT, l, rows_c)
        ref, bound = M("Y1%d" % l, [ctx, x, m1], lambda: resid_ref(ctx, L["wo"], L["bo"], x, m1, s))
        rep.derived("fwd/l%d/Y1" % l, ratio(Y1, ref, bound))
        rep.derived("fwd/l%d/X1" % l, ln_out_ratio(X1, None, Y1, L["ln1_g"], L["ln1_b"], W.eps))
        r = M("H%d" % l, [X1], lambda: ffn1_ref(X1, L["w1"], L["b1"]))
        rep.derived("fwd/l%d/Hm" % l, ratio(Hm, r["hm"], r["hm_bound"]))
        if Hpre is not None:
            rep.derived("fwd/l%d/Hpre" % l, ratio(Hpre, r["pre"], r["pre_bound"]))
        if Gp is not None:
            rep.derived("fwd/l%d/Gp" % l, ratio(Gp, r["gp"], r["gp_bound"]))
        ref, bound = M("Y2%d" % l, [Hm, X1, m2], lambda: resid_ref(Hm, L["w2"], L["b2"], X1, m2, s))
        rep.derived("fwd/l%d/Y2" % l, ratio(Y2, ref, bound))
        if tail:
            rep.derived("fwd/l%d/cls" % l, ln_out_ratio(f["cls_b"], f["cls_f"], Y2, L["ln2_g"], L["ln2_b"], W.eps))
        else:
            nxt = f["Xin/%d" % (l + 1)][lv] if l + 1 < NL else f["Xout"][lv]
            rep.derived("fwd/l%d/Xnext" % l, ln_out_ratio(nxt, None, Y2, L["ln2_g"], L["ln2_b"], W.eps))
    if cfg["pool_mean"]:
        xs = ES.per_sequence(lens, lambda t: (t.mean(0, keepdim=True), t.abs().mean(0, keepdim=True) * (t.shape[0] + 2) * E24), f["Xout"][lv])
        rep.derived("fwd/pool_f", ratio(f["cls_f"], xs[0], xs[1] + 1e-300))
        rep.derived("fwd/pool_b", _bf16_ratio(f["cls_b"], xs[0], xs[1]))
    y = f["cls_b"] @ HD.w.T + HD.b
    rep.derived("fwd/head_y", ratio(f["head_y"], y, (H + 2) * E24 * (f["cls_b"].abs() @ HD.w.abs().T + HD.b.abs())))
    rep.derived("fwd/out", ln_out_ratio(None, f["out"], f["head_y"], HD.g, HD.beta, HD.eps))


def _ln_stage(rep, name, ref, dxf, dxb, grads3, rows):
    for k, v in ln_bwd_ratios(ref, dxf, dxb, grads3, rows).items():
        rep.derived("%s/%s" % (name, k), v)


def check_backward(res, W, HD, lens, drop, rep, gelu_gp, dq_rows, which="all", memo_key=None):
    """Every backward stage (but the attention's and the embeddings') of run `res`.  which = 'all', or 'sums': only the LayerNorm
    backward, column-sum and weight-gradient stages (the large input M)."""
    f, lv, cu, cfg, S, G = res["fwd"], res["live"], res["cu"], res["cfg"], res["bwd"], res["grads"]
    H, I, NL, heads, rows = cfg["H"], cfg["I"], cfg["NL"], cfg["heads"], res["rows"]
    B = len(lens)
    lens = [int(n) for n in lens]
    allr = np.arange(rows)
    starts = torch.as_tensor(cu[:-1].astype(np.int64))
    full = which == "all"
    mk = lambda site, l, r: mask_rows(drop, site, l, r, H)
    M = lambda tag, ts, fn: ES.memo((tag, memo_key), ts, fn) if memo_key is not None else fn()

    def wg(name, l, dy, x, key):
        # slices as wgrad_launch cuts them: layer 0's batch of four (not the CLS tail's) goes out with tail_split = 2.
        # What the bound still catches at input M (3,920 rows): a lost 32-row K step is 32 / 3,920 = 8e-3 of |dY|^T |X| where
        # the terms do not cancel, a lost octet all of it, against (3,920 + 4) e24 = 2.3e-4 -- test_wgrad_bound_at_many_rows.
        split = 2 if (l == 0 and dy.shape[0] == rows and NL > 0 and not (l == NL - 1 and not cfg["pool_mean"])) else 0
        ref, bound = M(name, [dy, x], lambda: wgrad_ref(dy, x, wgrad_slices(dy.shape[0], split)))
        for run in (l, "full"):
            g = G[run]
            got = torch.cat([g["wq/%d" % l], g["wk/%d" % l], g["wv/%d" % l]], 0) if key == "wqkv" else g["%s/%d" % (key, l)] if l is not None else g[key]
            rep.derived("%s/%s" % (name, run), ratio(got, ref, bound))

    def sums3(l, keys, run):
        return [None if k is None else (G[run]["%s/%d" % (k, l)] if l is not None else G[run][k]) for k in keys]

    # ---- head ----
    top = S[NL]
    ref = ln_bwd_ref(res["d_out"], None, f["head_y"], HD.g, HD.eps)
    for run in (NL, "full"):
        _ln_stage(rep, "bwd/head_ln/%s" % run, ref, top["dhead_y"], top["dhead_yb"], sums3(None, ("head_b", "head_ln_g", "head_ln_b"), run), B)
    y = top["dhead_yb"] @ HD.w
    rep.derived("bwd/head_dgrad", ratio(top["dcls_f"], y, (HD.w.shape[0] + 2) * E24 * (top["dhead_yb"].abs() @ HD.w.abs()) + 1e-300))
    ref_w, bound_w = wgrad_ref(top["dhead_yb"], f["cls_b"], 1)
    for run in (NL, "full"):
        rep.derived("bwd/head_w/%s" % run, ratio(G[run]["head_w"], ref_w, bound_w))
    dcls = top["dcls_f"]
    if cfg["pool_mean"]:
        g0 = torch.zeros(rows, H, dtype=F64)
        for b, n in enumerate(lens):
            g0[cu[b]:cu[b] + n] = dcls[b] / n
        rep.derived("bwd/mean", nan_max((top["G0"] - g0).abs() / (3 * E24 * g0.abs() + 1e-300) * ((top["G0"] != g0) | torch.isnan(top["G0"]))))
    for l in range(NL - 1, -1, -1):
        L = W.layers[l]
        s = S[l]
        tail = l == NL - 1 and not cfg["pool_mean"]
        nm = "bwd/l%d" % l
        dqkv = s["dQKV/%d" % l]
        if not tail:
            if l == NL - 1:
                dya, dyb = S[NL]["G0"], None
            else:
                dya, dyb = S[l + 1]["G0"], S[l + 1]["dXb2"]
            Y2, Y1, X1, Hm, xin, ctx = (f["%s/%d" % (k, l)] for k in ("Y2", "Y1", "X1", "Hm", "Xin", "ctx"))
            dYb, dHpre, dYb2 = s["dYb/%d" % l], s["dHpre/%d" % l], s["dYb2/%d" % l]
            # LN2'
            m2 = mk(OD.SITE_FFN_OUT, l, allr)
            ref = M("LN2'%d" % l, [dya, Y2, m2] + ([dyb] if dyb is not None else []), lambda: ln_bwd_ref(dya, dyb, Y2, L["ln2_g"], W.eps, m2))
            refl = dict(dx=ref["dx"][lv], e32=ref["e32"][lv], mask=ref["mask"][lv])
            _ln_stage(rep, nm + "/LN2'", refl, s["G1"][lv], dYb[lv], None, rows)
            for run in (l, "full"):
                _ln_stage(rep, nm + "/LN2'/%s" % run, ref, None, None, sums3(l, ("b2", "ln2_g", "ln2_b"), run), rows)
            # FFN2 dgrad x gelu'
            if full:
                if gelu_gp:
                    gp = f["Gp/%d" % l][lv]
                    y, bound = M("dHpre%d" % l, [dYb[lv], gp], lambda: dgrad_ref(dYb[lv], L["w2"], gp))
                    rep.derived(nm + "/dHpre", ratio(dHpre[lv], y, bound))
                else:
                    hp = f["Hpre/%d" % l][lv]
                    y, bound = M("dgelu_d%d" % l, [dYb[lv], hp], lambda: dgelu_ref(dYb[lv], L["w2"], hp))
                    rep.derived(nm + "/dHpre_2r", ratio(dHpre[lv], y, bound))
                y, bound = M("dXb1%d" % l, [dHpre[lv]], lambda: dgrad_ref(dHpre[lv], L["w1"]))
                rep.derived(nm + "/dXb1", ratio(s["dXb1"][lv], y, bound))
            # LN1'
            m1 = mk(OD.SITE_ATTN_OUT, l, allr)
            ref = M("LN1'%d" % l, [s["G1"], s["dXb1"], Y1, m1], lambda: ln_bwd_ref(s["G1"], s["dXb1"], Y1, L["ln1_g"], W.eps, m1))
            refl = dict(dx=ref["dx"][lv], e32=ref["e32"][lv], mask=ref["mask"][lv])
            _ln_stage(rep, nm + "/LN1'", refl, s["G0"][lv], dYb2[lv], None, rows)
            for run in (l, "full"):
                _ln_stage(rep, nm + "/LN1'/%s" % run, ref, None, None, sums3(l, ("bo", "ln1_g", "ln1_b"), run), rows)
            if full:
                y, bound = M("dctx%d" % l, [dYb2[lv]], lambda: dgrad_ref(dYb2[lv], L["wo"]))
                rep.derived(nm + "/dctx", ratio(s["dctx"][lv], y, bound))
            cs, cb = colsum_ref(dHpre, colsum_chunks(rows))
            for run in (l, "full"):
                rep.derived(nm + "/b1/%s" % run, ratio(G[run]["b1/%d" % l], cs, cb))
            wg(nm + "/w1", l, dHpre, X1, "w1")
            wg(nm + "/w2", l, dYb, Hm, "w2")
            wg(nm + "/wo", l, dYb2, ctx, "wo")
        else:
            rows_c = cu[:-1]
            m2, m1 = mk(OD.SITE_FFN_OUT, l, rows_c), mk(OD.SITE_ATTN_OUT, l, rows_c)
            p_hid = 0.0 if drop is None else drop[0]
            ref = ln_bwd_ref(dcls, None, f["cls_y"], L["ln2_g"], W.eps)
            _ln_stage(rep, nm + "/cLN2'", ref, s["dcls_y"], None, None, B)
            for run in (l, "full"):
                _ln_stage(rep, nm + "/cLN2'/%s" % run, ref, None, None, sums3(l, (None if p_hid > 0 else "b2", "ln2_g", "ln2_b"), run), B)
            want = (s["dcls_y"].to(F32) * m2.to(F32)).to(BF16).to(F64)
            rep.exact(nm + "/c_dYb", torch.equal(want, s["c_dYb"]))
            if p_hid > 0:
                cs, cb = colsum_ref(s["c_dYb"], colsum_chunks(B))
                for run in (l, "full"):
                    rep.derived(nm + "/b2_colsum/%s" % run, ratio(G[run]["b2/%d" % l], cs, cb))
            y, bound = dgelu_ref(s["c_dYb"], L["w2"], f["c_Hpre"])
            rep.derived(nm + "/c_dHpre_2r", ratio(s["c_dHpre"], y, bound))
            y, bound = f32_sum_ref(s["c_dHpre"], L["w1"], s["dcls_y"], CLS_MAX_SPLIT)
            rep.derived(nm + "/c_dX1f", ratio(s["c_dX1f"], y, bound + 1e-300))
            ref = ln_bwd_ref(s["c_dX1f"], None, f["c_Y1"], L["ln1_g"], W.eps, m1)
            _ln_stage(rep, nm + "/cLN1'", ref, s["c_dY1"], s["c_dYb2"], None, B)
            for run in (l, "full"):
                _ln_stage(rep, nm + "/cLN1'/%s" % run, ref, None, None, sums3(l, ("bo", "ln1_g", "ln1_b"), run), B)
            y, bound = dgrad_ref(s["c_dYb2"], L["wo"])
            rep.derived(nm + "/c_dctx", ratio(s["c_dctx"], y, bound))
            # k_cls_tail_scatter
            g0 = torch.zeros(rows, H, dtype=F64)
            g0[starts] = s["c_dY1"]
            rep.exact(nm + "/scatter_G0", torch.equal(s["G0"], g0))
            first = torch.cat([torch.arange(cu[b], min(cu[b] + 128, cu[b + 1])) for b in range(B)])
            dc = torch.zeros(rows, H, dtype=F64)
            dc[starts] = s["c_dctx"]
            rep.exact(nm + "/scatter_dctx", torch.equal(s["dctx"][first], dc[first]))
            beyond = [torch.arange(cu[b] + dq_rows, cu[b + 1]) for b in range(B) if cu[b] + dq_rows < cu[b + 1]]
            if beyond:
                rep.exact(nm + "/scatter_dQ", bool((dqkv[torch.cat(beyond), :H] == 0).all()))
            cs, cb = colsum_ref(s["c_dHpre"], colsum_chunks(B))
            for run in (l, "full"):
                rep.derived(nm + "/b1/%s" % run, ratio(G[run]["b1/%d" % l], cs, cb))
            wg(nm + "/w1", l, s["c_dHpre"], f["c_X1"], "w1")
            wg(nm + "/w2", l, s["c_dYb"], f["c_Hm"], "w2")
            wg(nm + "/wo", l, s["c_dYb2"], f["c_ctx"], "wo")
            xin = f["Xin/%d" % l]
        # attention': dQKV per (token, head, third) slice, against the reference pair on the GPU's own QKV, dctx, LSE, ctx
        if full:
            masks = None if (drop is None or drop[1] == 0) else [att_mask_seq(drop, l, int(cu[b]), n, heads) for b, n in enumerate(lens)]
            if tail:
                do = torch.zeros(rows, H, dtype=F64)
                do[starts] = s["c_dctx"]
                do, o32 = do[lv], f["c_ctx32"]
            else:
                do, o32 = s["dctx"][lv], None
            # (the CLS tail's forward ran the first query tile only: LSE and ctx of the later queries were never written, and with
            #  dO = 0 those queries contribute nothing -- P = 0 for them here)
            a_in = [f["QKV/%d" % l][lv], do, f["LSE/%d" % l].T[lv].nan_to_num(1e30).contiguous(), f["ctx/%d" % l][lv].nan_to_num(0.0)]
        if full and tail:   # one live query per sequence: products, not sums -- a derived bound (attn_bwd_tail_ref), no pair
            outs, o = [], 0
            for b, n in enumerate(lens):
                outs.append(attn_bwd_tail_ref(a_in[0][o:o + n], s["c_dctx"][b], a_in[2][o], o32[b], heads,
                                              None if masks is None else masks[b][:, 0]))
                o += n
            rep.derived(nm + "/att'_tail", ratio(dqkv[lv], torch.cat([x[0] for x in outs]), torch.cat([x[1] for x in outs])))
        elif full:
                r64, r32 = M("att'%d" % l, a_in + ([o32] if tail else []) + ([] if masks is None else [torch.tensor([float(drop[2]), l])]),
                             lambda: tuple(attn_bwd_all(*a_in, lens, heads, acc=a, c_ctx32=o32, masks=masks) for a in (F64, F32)))
                c_ref, f_ref = slice_metrics(r32, r64)
                c_bar, f_cap = ES.tail_bars(c_ref, f_ref)
                c, fr = slice_metrics(dqkv[lv], r64)
                rep.items.append((nm + "/att'_c_floor", c_ref, float("inf")))
                rep.items.append((nm + "/att'_f_floor", f_ref, float("inf")))
                rep.measured(nm + "/att'_c", c, c_bar * (1 + 1e-9) + 1e-300)
                rep.measured(nm + "/att'_f", fr, f_cap)
        # QKV: data gradient, bias column sums (all three thirds), weight gradient
        if full:
            y, bound = M("dXb2%d" % l, [dqkv[lv]], lambda: dgrad_ref(dqkv[lv], L["wqkv"]))
            rep.derived(nm + "/dXb2", ratio(s["dXb2"][lv], y, bound))
        cs, cb = colsum_ref(dqkv, colsum_chunks(rows))
        for run in (l, "full"):
            got = torch.cat([G[run]["%s/%d" % (k, l)] for k in ("bq", "bk", "bv")])
            rep.derived(nm + "/bqkv/%s" % run, ratio(got, cs, cb))
            rep.derived(nm + "/bk/%s" % run, ratio(got[H:2 * H], cs[H:2 * H], cb[H:2 * H]))
        wg(nm + "/wqkv", l, dqkv, xin, "wqkv")
    # ---- embedding': the full (unstopped) run's tables and sums, from G0 + dXb2 behind layer 0 and the ids ----
    tid, tpos = f["tok_id"][lv], f["tok_pos"][lv]
    em = mk(OD.SITE_EMB, 0, lv.numpy())
    e = M("emb'", [S[0]["G0"][lv], S[0]["dXb2"][lv], em, tid, tpos], lambda: embed_bwd_ref(W, tid, tpos, S[0]["G0"][lv], S[0]["dXb2"][lv], em))
    g = G["full"]
    got = dict(word_emb=g["word_emb"], pos_emb=g["pos_emb"], type_emb0=g["type_emb"][0], emb_ln_g=g["emb_ln_g"], emb_ln_b=g["emb_ln_b"])
    for k, (ref, bound) in e.items():
        rep.derived("bwd/emb/%s" % k, ratio(got[k], ref, bound))
    if g["type_emb"].shape[0] > 1:
        rep.exact("bwd/emb/type_emb_rest", bool((g["type_emb"][1:] == 0).all()))


# ---- a stand-in for the library: the same run, computed on the CPU with the kernels' accumulation width and rounding points ---
FAULTS = ("dgrad_trunc", "ln_no_resid_half", "ln_skip_row", "mask_compact_row", "gelu_of_hm", "wgrad_skip_kstep", "wgrad_lost_octet",
          "bk_zero", "y1_mask_on_resid", "lse_natural", "gp_of_hm", "scatter_row", "mean_pad_rows", "b1_unrounded", "head_trunc",
          "cast_no_mask", "c_dx1_no_resid", "att_d_other_head", "att_no_scale", "att_kv_tile", "att_mask_other_layer", "att_mask_transposed",
          "mbits_bit", "emb_count_once")


def sim_run(W, HD, ids, lens, pool_mean, drop=None, gelu_gp=1, fault=None, seed=0):
    """A `res` like run_train's from stand-in kernels (fp32 accumulation, bf16 round-to-nearest-even at the kernels' rounding
    points).  The attention backward is not among the checked stages: its output dQKV is random bf16 data (teacher forcing: the
    stages behind it are judged on the dQKV they are given).  fault: one of FAULTS, planted into the stage it names."""
    assert fault is None or fault in FAULTS, fault
    lens = np.asarray(lens, np.int32)
    B, H, I, heads, NL = len(lens), W.H, W.I, W.heads, len(W.layers)
    E = HD.w.shape[0]
    cu = np.zeros(B + 1, np.int32)
    np.cumsum((lens + 7) // 8 * 8, out=cu[1:])
    rows = int(cu[-1])
    lv = torch.from_numpy(np.concatenate([cu[b] + np.arange(lens[b]) for b in range(B)]).astype(np.int64))
    starts = torch.as_tensor(cu[:-1].astype(np.int64))
    ll = [int(n) for n in lens]
    allr = np.arange(rows)
    mk = lambda site, l, r: mask_rows(drop, site, l, r, H)
    r32 = lambda t: t.to(F32).to(F64)

    def pack(t, dtype=None):
        o = torch.zeros((rows,) + tuple(t.shape[1:]), dtype=t.dtype)
        o[lv] = t
        return o
    f = {}
    tid, tpos = ES.host_tokens(ids, lens)
    f["tok_id"], f["tok_pos"] = pack(tid), pack(tpos)
    x = bf16r(r32(ES.ln(r32(r32(W.word[tid.long()] + W.pos[tpos.long()]) + W.type0), W.emb_g, W.emb_b, W.eps, F32)
                  * mk(OD.SITE_EMB, 0, lv.numpy())))
    for l in range(NL):
        L = W.layers[l]
        tail = l == NL - 1 and not pool_mean
        f["Xin/%d" % l] = pack(x)
        qkv = ES.qkv_sim(W, l + 1, x)
        f["QKV/%d" % l] = pack(qkv)
        p_att = 0.0 if drop is None else drop[1]
        if p_att > 0:
            from oracle.encoder import _attention_bf16
            amasks = [att_mask_seq(drop, l, int(cu[b]), n, heads) for b, n in enumerate(ll)]
            if fault == "att_mask_other_layer":
                amasks = [att_mask_seq(drop, l + 1, int(cu[b]), n, heads) for b, n in enumerate(ll)]
            outs, o = [], 0
            for b, n in enumerate(ll):
                a = qkv[o:o + n].to(F32)
                hd = lambda t: t.view(1, n, heads, H // heads).transpose(1, 2)
                r = _attention_bf16(hd(a[:, :H]), hd(a[:, H:2 * H]), hd(a[:, 2 * H:]), [n], 0.125, amasks[b][None].to(F32))
                outs.append(bf16r(r.transpose(1, 2).reshape(n, H).to(F64)))
                o += n
            ctx = torch.cat(outs)
            if max(ll) <= 256:   # the kept bits, in the kernel's layout
                mb = torch.zeros(heads, 8, rows + 128, dtype=torch.int64)
                for b, n in enumerate(ll):
                    key = torch.arange(n)
                    piece, bit = 2 * (key >> 6) + ((key >> 3) & 1), 16 * ((key >> 5) & 1) + 8 * ((key >> 4) & 1) + (key & 7)
                    keep = (amasks[b] != 0).to(torch.int64) << bit[None, None, :]                 # [heads, query, key]
                    for pc in range(8):
                        mb[:, pc, int(cu[b]):int(cu[b]) + n] = keep[:, :, piece == pc].sum(-1)
                if fault == "mbits_bit":
                    mb[1, 0, int(cu[2]) + 3] ^= 1 << 9
                f["Mbits/%d" % l] = mb.to(torch.int32)
        else:
            ctx = ES.per_sequence(ll, lambda a: ES.attention_sim(a[:, :H], a[:, H:2 * H], a[:, 2 * H:], heads), qkv)
        f["ctx/%d" % l] = pack(ctx)
        lse = ES.per_sequence(ll, lambda a: lse_sim(a[:, :H], a[:, H:2 * H], heads).T, qkv)
        if fault == "lse_natural":
            lse = lse * math.log(2.0)
        f["LSE/%d" % l] = pack(lse).T
        if tail:
            ctx, x = ctx[torch.as_tensor(np.concatenate([[0], np.cumsum(ll)[:-1]]))], x[torch.as_tensor(np.concatenate([[0], np.cumsum(ll)[:-1]]))]
            rc = cu[:-1]
            f["c_ctx"], f["c_xin"], f["c_ctx32"] = ctx, x, ctx.clone()
        else:
            rc = lv.numpy()
        m1, m2 = mk(OD.SITE_ATTN_OUT, l, rc), mk(OD.SITE_FFN_OUT, l, rc)
        if fault == "y1_mask_on_resid" and l == 0:
            y1 = r32((ES.lin(ctx, L["wo"], L["bo"], F32) + x) * (m1 if drop else 1.0 + 2.0 ** -10))
        else:
            y1 = resid_sim(ctx, L["wo"], L["bo"], x, m1)
        x1 = bf16r(ES.ln(y1, L["ln1_g"], L["ln1_b"], W.eps, F32))
        hm, hpre, gp = ffn1_sim(x1, L["w1"], L["b1"])
        if fault == "gp_of_hm":
            gp = bf16r(gelu_grad_fit(hm.to(F32)).to(F64))
        y2 = resid_sim(hm, L["w2"], L["b2"], x1, m2)
        xn = ES.ln(y2, L["ln2_g"], L["ln2_b"], W.eps, F32)
        if tail:
            f["c_Y1"], f["c_X1"], f["c_Hm"], f["c_Hpre"], f["cls_y"] = y1, x1, hm, hpre, y2
            f["cls_f"], f["cls_b"] = xn, bf16r(xn)
        else:
            f["Y1/%d" % l], f["X1/%d" % l], f["Hm/%d" % l], f["Y2/%d" % l] = pack(y1), pack(x1), pack(hm), pack(y2)
            f["Gp/%d" % l if gelu_gp else "Hpre/%d" % l] = pack(gp if gelu_gp else hpre)
            x = bf16r(xn)
    if pool_mean:
        f["Xout"] = pack(x)
        pooled = ES.per_sequence(ll, lambda t: r32(t.to(F32).sum(0, keepdim=True) / t.shape[0]), x)
        f["cls_f"], f["cls_b"] = pooled, bf16r(pooled)
    f["head_y"] = ES.lin(f["cls_b"], HD.w, HD.b, F32)
    f["out"] = ES.ln(f["head_y"], HD.g, HD.beta, HD.eps, F32)

    # ---- backward ----
    gen = torch.Generator().manual_seed(seed + 1)
    d_out = r32(torch.randn(B, E, generator=gen) * 0.05)
    S, G = {}, {}
    grads = {}
    top = {}
    top["dhead_y"], top["dhead_yb"], sums = ln_bwd_sim(d_out, None, f["head_y"], HD.g, HD.eps,
                                                       rnd=ES.bf16_trunc if fault == "head_trunc" else bf16r)
    grads["head_b"], grads["head_ln_g"], grads["head_ln_b"] = sums
    grads["head_w"] = wgrad_sim(top["dhead_yb"], f["cls_b"])
    top["dcls_f"] = r32(top["dhead_yb"].to(F32) @ HD.w.to(F32))
    dcls = top["dcls_f"]
    cur_f, cur_b = None, None
    if pool_mean:
        g0 = torch.zeros(rows, H, dtype=F64)
        for b, n in enumerate(ll):
            g0[cu[b]:cu[b] + (int(cu[b + 1] - cu[b]) if fault == "mean_pad_rows" else n)] = r32(dcls[b].to(F32) * (np.float32(1) / np.float32(n)))
        cur_f = g0
    top["G0"] = cur_f if cur_f is not None else torch.full((rows, H), float("nan"), dtype=F64)
    nanb = lambda n: torch.full((rows, n), float("nan"), dtype=F64)
    top.update(G1=nanb(H), dXb1=nanb(H), dXb2=nanb(H), dctx=nanb(H))
    S[NL] = top
    prev = top
    for l in range(NL - 1, -1, -1):
        L = W.layers[l]
        tail = l == NL - 1 and not pool_mean
        s = {k: prev[k] for k in ("dhead_y", "dhead_yb", "dcls_f")}
        if not tail:
            Y2, Y1, X1, Hm, xin, ctx = (f["%s/%d" % (k, l)] for k in ("Y2", "Y1", "X1", "Hm", "Xin", "ctx"))
            m2, m1 = mk(OD.SITE_FFN_OUT, l, allr), mk(OD.SITE_ATTN_OUT, l, allr)
            dy2, dyb, sums = ln_bwd_sim(cur_f, cur_b, Y2, L["ln2_g"], W.eps, m2, add_b=fault != "ln_no_resid_half",
                                        skip_row=int(lv[5]) if fault == "ln_skip_row" and l == 0 else None)
            if fault == "ln_skip_row" and l == 0:   # (the skipped row keeps what the buffers held: finite, but not this row's)
                dy2[int(lv[5])], dyb[int(lv[5])] = 0.0, 0.0
            grads["b2/%d" % l], grads["ln2_g/%d" % l], grads["ln2_b/%d" % l] = sums
            if gelu_gp:
                dhpre = dgrad_sim(dyb, L["w2"], f["Gp/%d" % l])
            else:
                dhpre = dgelu_chain(dyb, L["w2"], f["Hpre/%d" % l], acc=F32, grad_of=Hm if fault == "gelu_of_hm" else None)
            dxb1 = dgrad_sim(dhpre, L["w1"], rnd=ES.bf16_trunc if fault == "dgrad_trunc" else bf16r)
            dy1, dyb2, sums = ln_bwd_sim(dy2, dxb1, Y1, L["ln1_g"], W.eps, m1)
            grads["bo/%d" % l], grads["ln1_g/%d" % l], grads["ln1_b/%d" % l] = sums
            dctx = dgrad_sim(dyb2, L["wo"])
            grads["b1/%d" % l] = r32(dhpre.to(F32).sum(0)) if fault != "b1_unrounded" else (dyb @ L["w2"] * (f["Gp/%d" % l] if gelu_gp else 1)).sum(0)
            grads["w1/%d" % l] = wgrad_sim(dhpre, X1, skip=(64, 32) if fault == "wgrad_skip_kstep" else None)
            grads["w2/%d" % l] = wgrad_sim(dyb, Hm, trunc_octet=(3, 16) if fault == "wgrad_lost_octet" else None)
            grads["wo/%d" % l] = wgrad_sim(dyb2, ctx)
            s.update({"dYb/%d" % l: dyb, "dHpre/%d" % l: dhpre, "dYb2/%d" % l: dyb2, "G1": dy2, "G0": dy1, "dXb1": dxb1, "dctx": dctx})
        else:
            rc = cu[:-1] if fault != "mask_compact_row" else np.arange(B)
            m2, m1 = mk(OD.SITE_FFN_OUT, l, rc), mk(OD.SITE_ATTN_OUT, l, rc)
            if fault == "cast_no_mask":
                m2 = torch.ones_like(m2) * (1.0 if drop else 1.0 + 2.0 ** -6)
            p_hid = 0.0 if drop is None else drop[0]
            dcls_y, _, sums = ln_bwd_sim(dcls, None, f["cls_y"], L["ln2_g"], W.eps)
            grads["b2/%d" % l], grads["ln2_g/%d" % l], grads["ln2_b/%d" % l] = sums
            c_dyb = (dcls_y.to(F32) * m2.to(F32)).to(BF16).to(F64)
            if p_hid > 0:
                grads["b2/%d" % l] = r32(c_dyb.to(F32).sum(0))
            c_dhpre = dgelu_chain(c_dyb, L["w2"], f["c_Hpre"], acc=F32, grad_of=f["c_Hm"] if fault == "gelu_of_hm" else None)
            c_dx1f = r32(c_dhpre.to(F32) @ L["w1"].to(F32) + (0 if fault == "c_dx1_no_resid" else dcls_y.to(F32)))
            c_dy1, c_dyb2, sums = ln_bwd_sim(c_dx1f, None, f["c_Y1"], L["ln1_g"], W.eps, m1)
            grads["bo/%d" % l], grads["ln1_g/%d" % l], grads["ln1_b/%d" % l] = sums
            c_dctx = dgrad_sim(c_dyb2, L["wo"])
            g0 = torch.zeros(rows, H, dtype=F64)
            g0[starts] = c_dy1
            dctx = torch.zeros(rows, H, dtype=F64)
            dctx[starts] = c_dctx
            if fault == "scatter_row":
                g0[starts[1] + 1] = c_dy1[1]
            grads["b1/%d" % l] = r32(c_dhpre.to(F32).sum(0))
            grads["w1/%d" % l], grads["w2/%d" % l] = wgrad_sim(c_dhpre, f["c_X1"]), wgrad_sim(c_dyb, f["c_Hm"])
            grads["wo/%d" % l] = wgrad_sim(c_dyb2, f["c_ctx"])
            s.update(dcls_y=dcls_y, c_dYb=c_dyb, c_dHpre=c_dhpre, c_dX1f=c_dx1f, c_dY1=c_dy1, c_dYb2=c_dyb2, c_dctx=c_dctx,
                     G0=g0, dctx=dctx, G1=prev["G1"], dXb1=prev["dXb1"])
            dy1, xin = g0, f["Xin/%d" % l]
        att_fault = fault[4:] if fault is not None and fault.startswith("att_") else None
        amasks = None if (drop is None or drop[1] <= 0) else [att_mask_seq(drop, l, int(cu[b]), n, heads) for b, n in enumerate(ll)]
        if att_fault == "mask_transposed":
            amasks, att_fault = [m.transpose(1, 2) for m in amasks], None
        dqkv = attn_bwd_all(f["QKV/%d" % l][lv], s["dctx"][lv], f["LSE/%d" % l].T[lv].contiguous(), f["ctx/%d" % l][lv], ll, heads,
                            acc=F32, c_ctx32=f["c_ctx32"] if tail else None, fault=att_fault, masks=amasks, reorder=True)
        dqkv = pack(dqkv)
        s["dQKV/%d" % l] = dqkv
        bq = r32(dqkv.to(F32).sum(0))
        if fault == "bk_zero":
            bq[H:2 * H] = 0
        grads["bq/%d" % l], grads["bk/%d" % l], grads["bv/%d" % l] = bq[:H], bq[H:2 * H], bq[2 * H:]
        wq = wgrad_sim(dqkv, xin)
        grads["wq/%d" % l], grads["wk/%d" % l], grads["wv/%d" % l] = wq[:H], wq[H:2 * H], wq[2 * H:]
        s["dXb2"] = dgrad_sim(dqkv, L["wqkv"])
        cur_f, cur_b = dy1, s["dXb2"]
        S[l] = s
        prev = s
    e = embed_bwd_sim(W, tid, tpos, S[0]["G0"][lv], S[0]["dXb2"][lv], mk(OD.SITE_EMB, 0, lv.numpy()), count_once=fault == "emb_count_once")
    grads["word_emb"], grads["pos_emb"], grads["emb_ln_g"], grads["emb_ln_b"] = e["word_emb"], e["pos_emb"], e["emb_ln_g"], e["emb_ln_b"]
    grads["type_emb"] = torch.cat([e["type_emb0"][None], torch.zeros(1, H, dtype=F64)])
    for stop in list(S) + ["full"]:
        G[stop] = grads
    return {"fwd": f, "bwd": S, "grads": G, "d_out": d_out, "live": lv, "cu": cu, "rows": rows,
            "cfg": dict(H=H, I=I, NL=NL, E=E, heads=heads, pool_mean=bool(pool_mean))}
