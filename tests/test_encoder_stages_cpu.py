"""The stage references and bounds of tests/encoder_stages.py, checked without a GPU on the GPU test's own inputs:
  * chained from token ids they reproduce the bf16-emulating oracle (they cannot drift from it);
  * a correct stand-in kernel (the same stage with fp32 accumulation, the oracle's kernel-arithmetic attention) holds every
    derived bound (ratio < 1) and yields the floors c_ref / f_ref of the measured ones;
  * every planted fault breaks its stage's check (ratio > 1, c above its bar, or f above its cap);
  * the same for the head (stage G) at out_dim 4, 132 and 1024 on the 640- and 1024-wide models;
  * ES.layouts(), the mirror of encoder_layer_forward's dispatch, answers "nothing blocked, Y live" for every admitted hidden size
    off 768 at input S.
Models: W (768 / 12 / 3072), N (384 / 6 / 320) and the six ES.ENVELOPE shapes (128 / 64, 256 / 192, 512 / 1024, 640 / 448,
896 / 2304, 1024 / 4096), two layers each, all on input S.
Run with -s to see the ratios and floors."""
import numpy as np
import pytest
import torch

from tests import encoder_stages as ES
from tests.encoder_stages import F32, F64, LENS_S


class Sim:
    """Layer 1 of a model on input S through the stand-in kernels, each stage's buffers kept."""

    def __init__(self, shape, stats):
        self.W = ES.Weights(ES.make_model(shape, stats).roberta)
        ids, lens = ES.input_s()
        self.lens = [int(n) for n in lens]
        self.tok_id, self.tok_pos = ES.host_tokens(ids, lens)
        W = self.W
        self.H = W.H
        self.X0 = ES.embed_sim(W, self.tok_id, self.tok_pos)
        self.QKV = ES.qkv_sim(W, 1, self.X0)
        H = W.H
        self.ctx = ES.per_sequence(self.lens, lambda q, k, v: ES.attention_sim(q, k, v, W.heads),
                                   self.QKV[:, :H], self.QKV[:, H:2 * H], self.QKV[:, 2 * H:])
        self.Hm, self.X1, _ = ES.tail_chain(W, 1, self.ctx, self.X0, acc=F32)
        # references, teacher-forced on the stand-in's own buffers
        self.A_ref, self.A_e32 = ES.embed_ref(W, self.tok_id, self.tok_pos)
        L = W.layers[0]
        self.B_ref, self.B_bound = ES.proj_ref(self.X0, L["wqkv"], L["bqkv"])
        self.C_ref, self.C_bound, self.C_u = ES.per_sequence(
            self.lens, lambda q, k, v: ES.attention_ref(q, k, v, W.heads), self.QKV[:, :H], self.QKV[:, H:2 * H], self.QKV[:, 2 * H:])
        self.D_hm, self.D_x, _ = ES.tail_chain(W, 1, self.ctx, self.X0)
        self.starts = np.concatenate([[0], np.cumsum(self.lens)[:-1]])

    def ratio_B(self, got):
        return float(((got - self.B_ref).abs() / self.B_bound).max())

    def ratio_C(self, got, rows=slice(None)):
        return float(((got - self.C_ref[rows]).abs() / self.C_bound[rows]).max())

    def seq(self, n):
        b = LENS_S.index(n)
        return slice(int(self.starts[b]), int(self.starts[b]) + n)


_SIMS = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_sims():
    yield
    _SIMS.clear()


def sim(shape, stats):
    if (shape, stats) not in _SIMS:
        _SIMS[(shape, stats)] = Sim(shape, stats)
    return _SIMS[(shape, stats)]


CASES = [("W", "init"), ("W", "trained"), ("N", "init")] + [(sh, "init") for sh in ES.ENVELOPE]


def test_stage_references_chain_to_the_emulating_oracle():
    """Embedding -> 2 x (QKV, attention, tail) of the stage functions, chained from token ids with fp64 and with fp32
    accumulation, against oracle.encoder.encoder_hidden(emulate_bf16=True, return_all=True): per-token relative L2 within
    1e-2 at every layer (two accumulation orders of the emulation are 2.9e-3 apart after two layers; a wrong residual,
    activation or LayerNorm is 1e-1 and more)."""
    from oracle import encoder as OE
    model = ES.make_model("N", "init")
    W = ES.Weights(model.roberta)
    ids, lens = ES.make_inputs([1, 9, 64, 65, 130], 1000, 3, pads=((2, 4),))
    mask = (np.arange(ids.shape[1])[None, :] < lens[:, None]).astype(np.int64)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    hs = OE.encoder_hidden(sd, "roberta.", torch.from_numpy(ids), torch.from_numpy(mask), kind="roberta", num_layers=2,
                           num_heads=W.heads, eps=model.roberta.config.layer_norm_eps, return_all=True, emulate_bf16=True)
    keep = torch.from_numpy(mask).bool()
    tid, tpos = ES.host_tokens(ids, lens)
    H = W.H
    for acc in (F64, F32):
        x = ES.bf16r(ES.embed_ref(W, tid, tpos)[0]) if acc is F64 else ES.embed_sim(W, tid, tpos)
        xs = [x]
        for l in (1, 2):
            qkv = ES.qkv_sim(W, l, x, acc=acc)
            if acc is F64:
                ctx = ES.bf16r(ES.per_sequence(lens, lambda q, k, v: ES.attention_ref(q, k, v, W.heads)[0],
                                               qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]))
            else:
                ctx = ES.per_sequence(lens, lambda q, k, v: ES.attention_sim(q, k, v, W.heads), qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:])
            x = ES.tail_chain(W, l, ctx, x, acc=acc)[1]
            xs.append(x)
        for l, (mine, theirs) in enumerate(zip(xs, hs)):
            t = theirs[keep].double()
            rel = ((mine - t).norm(dim=-1) / t.norm(dim=-1)).max()
            print("chain acc=%s layer %d: worst per-token relative L2 %.3g" % (acc, l, rel))
            assert rel < 1e-2, (acc, l, float(rel))


@pytest.mark.parametrize("shape,stats", CASES)
def test_derived_bounds_hold_for_the_stand_in(shape, stats):
    """Stages A-C (and E: the LayerNorm bound applied to the stand-in's own pre-LayerNorm sums): max ratio < 1."""
    s = sim(shape, stats)
    W = s.W
    rA = ES.ratio_bf16_of_fp32(s.X0, s.A_ref, s.A_e32)
    rB = s.ratio_B(s.QKV)
    rC = s.ratio_C(s.ctx)
    rCu = float(((s.ctx - s.C_ref).abs() / s.C_u).max())
    y = (torch.randn(64, W.H, generator=torch.Generator().manual_seed(1)) * 3 + 0.5).to(F32).to(F64)
    L = W.layers[0]
    rE = ES.ratio_bf16_of_fp32(ES.bf16r(ES.ln(y, L["ln2_g"], L["ln2_b"], W.eps, F32)), ES.ln(y, L["ln2_g"], L["ln2_b"], W.eps),
                               ES.ln_fp32_err(y, L["ln2_g"], L["ln2_b"], W.eps))
    print("%s/%s ratios: A %.3f  B %.3f  C %.3f (of u(|ref| + A) alone: %.3f)  E %.3f" % (shape, stats, rA, rB, rC, rCu, rE))
    assert rA < 1 and rB < 1 and rC < 1 and rE < 1, (rA, rB, rC, rE)
    # the fp32 terms of the stage A / C bounds are small beside u: the bounds are as tight as bf16 allows
    assert float((s.A_e32 / (ES.U * s.A_ref.abs() + s.A_e32)).median()) < 0.05
    assert float(((s.C_bound - s.C_u) / s.C_u).max()) < 0.5


@pytest.mark.parametrize("shape,stats", CASES)
def test_measured_floors_of_the_tail(shape, stats):
    """Stage D: the fp32-accumulating chain against the fp64 one on the same inputs gives c_ref, f_ref; stage F likewise."""
    s = sim(shape, stats)
    c_h, f_h = ES.tail_metrics(s.Hm, s.D_hm)
    c_x, f_x = ES.tail_metrics(s.X1, s.D_x)
    print("%s/%s floors: Hm c %.3g f %.3g%%   X_l c %.3g f %.3g%%" % (shape, stats, c_h, 100 * f_h, c_x, 100 * f_x))
    assert c_h < 0.02 and c_x < 0.02 and f_h < 0.02 and f_x < 0.02      # flips, not a different function
    for fold in (True, False):
        ref = ES.cls_chain(s.W, 1, s.X0, s.lens, fold)
        got = ES.cls_chain(s.W, 1, s.X0, s.lens, fold, acc=F32)
        c, _ = ES.tail_metrics(got, ref, rel=0.0)
        print("%s/%s floor F (fold %d): c %.3g" % (shape, stats, fold, c))
        assert c < 0.02
    # the CLS rows of the all-token layer are the same function of the same inputs (own fp64 attention there: flips, no more)
    ref = ES.cls_chain(s.W, 1, s.X0, s.lens, False)
    full = s.D_x[torch.as_tensor(s.starts)]
    assert ES.tail_metrics(ES.bf16r(ref), full)[0] < 0.02


def _broken(c, f, c_ref, f_ref):
    c_bar, f_cap = ES.tail_bars(c_ref, f_ref)
    return c > c_bar or f > f_cap or not (c == c)


@pytest.mark.parametrize("shape,stats", CASES)
def test_planted_faults_break_their_stage(shape, stats):
    s = sim(shape, stats)
    W, H = s.W, s.H
    L = W.layers[0]
    seen = {}
    r128 = s.seq(128)

    # ---- stage B ----
    m = s.QKV.clone(); m[r128.start + 127] = m[r128.start + 126]
    seen["B row 127 := row 126"] = s.ratio_B(m)
    m = s.QKV.clone(); m[:, H - 8:H] = 0
    seen["B last octet of Q zeroed"] = s.ratio_B(m)
    b = L["bqkv"].clone(); b[-8:] = 0
    seen["B bias dropped for the last 8 features"] = s.ratio_B(ES.bf16r(ES.lin(s.X0, L["wqkv"], b, F32)))
    seen["B truncating conversion"] = s.ratio_B(ES.qkv_sim(W, 1, s.X0, rnd=ES.bf16_trunc))
    q = s.QKV[:, :H].contiguous()
    dec = ES.decode_blocked(ES.encode_blocked(q), q.shape[0], H)
    assert torch.equal(dec, q)                                                 # the blocked decoder inverts the layout
    sw = ES.decode_blocked(ES.encode_blocked(q), q.shape[0], H, swap_last_halves=True)
    assert q.shape[0] % 32 != 0
    seen["B blocked decode: halves of the ragged last block swapped"] = float(
        torch.nan_to_num(((sw - s.B_ref[:, :H]).abs() / s.B_bound[:, :H]), nan=float("inf")).max())
    # ---- stage A / E ----
    m = s.X0.clone(); m[:, -8:] = 0
    seen["A last octet zeroed"] = ES.ratio_bf16_of_fp32(m, s.A_ref, s.A_e32)
    seen["A truncating conversion"] = ES.ratio_bf16_of_fp32(ES.embed_sim(W, s.tok_id, s.tok_pos, rnd=ES.bf16_trunc), s.A_ref, s.A_e32)
    # ---- stage C ----
    Q, K, V = s.QKV[:, :H], s.QKV[:, H:2 * H], s.QKV[:, 2 * H:]
    for n in (65, 129):
        r = s.seq(n)
        seen["C last key of %d dropped" % n] = s.ratio_C(ES.attention_sim(Q[r], K[r], V[r], W.heads, n_keys=n - 1), r)
    r = s.seq(193)
    k2, v2 = K[r].clone(), V[r].clone()
    k2[128:192], v2[128:192] = K[r][64:128], V[r][64:128]
    seen["C key tile 1 used twice"] = s.ratio_C(ES.attention_sim(Q[r], k2, v2, W.heads), r)
    r = s.seq(65)
    zero = torch.zeros(7, H, dtype=F64)                                        # alignment rows [65, 72): X = 0 there after the embedding
    kv0 = ES.qkv_sim(W, 1, zero)
    seen["C alignment rows admitted as keys"] = s.ratio_C(
        ES.attention_sim(Q[r], torch.cat([K[r], kv0[:, H:2 * H]]), torch.cat([V[r], kv0[:, 2 * H:]]), W.heads), r)
    m = s.ctx.clone(); m[r128.start + 127] = m[r128.start + 126]
    seen["C row 127 := row 126"] = s.ratio_C(m)
    for name, ratio in seen.items():
        print("%s/%s  %-60s ratio %.3g" % (shape, stats, name, ratio))
        assert ratio > 1, (name, ratio)

    # ---- stage D ----
    ch, fh = ES.tail_metrics(s.Hm, s.D_hm)
    cx, fx = ES.tail_metrics(s.X1, s.D_x)
    assert not _broken(ch, fh, ch, fh) and not _broken(cx, fx, cx, fx)           # the unmutated stand-in passes
    faults = {}
    hm_t, x_t, _ = ES.tail_chain(W, 1, s.ctx, s.X0, acc=F32, rnd=ES.bf16_trunc)
    faults["D truncating conversion (Hm)"] = (hm_t, s.D_hm, ch, fh)
    faults["D truncating conversion (X_l)"] = (x_t, s.D_x, cx, fx)
    faults["D residual from X1"] = (ES.tail_chain(W, 1, s.ctx, s.X0, acc=F32, resid_from_x1=True)[1], s.D_x, cx, fx)
    m = s.X1.clone(); m[r128.start + 127] = m[r128.start + 126]
    faults["D row 127 := row 126 (X_l)"] = (m, s.D_x, cx, fx)
    m = s.X1.clone(); m[:, -8:] = 0
    faults["D last octet zeroed (X_l)"] = (m, s.D_x, cx, fx)
    m = s.Hm.clone(); m[:, -8:] = 0
    faults["D last octet zeroed (Hm)"] = (m, s.D_hm, ch, fh)
    m = s.Hm.clone(); m[r128.start + 127] = m[r128.start + 126]
    faults["D row 127 := row 126 (Hm)"] = (m, s.D_hm, ch, fh)
    for name, (got, ref, c_ref, f_ref) in faults.items():
        c, f = ES.tail_metrics(got, ref)
        print("%s/%s  %-60s c %.3g (bar %.3g)  f %.3g%% (cap %.3g%%)" % ((shape, stats, name, c) + (ES.tail_bars(c_ref, f_ref)[0], 100 * f,
                                                                                                    100 * ES.tail_bars(c_ref, f_ref)[1])))
        assert _broken(c, f, c_ref, f_ref), name


@pytest.mark.parametrize("E", [4, 132, 1024])
@pytest.mark.parametrize("shape", ["H640", "H1024"])
def test_head_stage_bounds_and_faults(shape, E):
    """Stage G on the CLS rows of the stand-in's X_1: the stand-in head holds both derived bounds; head_y or out with its last 4
    columns dropped (at E = 4: all of them) breaks the check of the value it was planted in, and only that one."""
    s = sim(shape, "init")
    HW = ES.HeadWeights(*ES.make_head(s.H, E))
    cls_b = s.X1[torch.as_tensor(s.starts)]
    y, out = ES.head_sim(HW, cls_b)
    rY, rO = ES.head_ratios(HW, cls_b, y, out)
    print("%s E %d: G ratios head_y %.3f  out %.3f" % (shape, E, rY, rO))
    assert rY < 1 and rO < 1, (rY, rO)
    m = y.clone(); m[:, -4:] = 0
    fY, fO = ES.head_ratios(HW, cls_b, m, ES.ln(m, HW.g, HW.beta, HW.eps, F32))      # teacher-forced: out follows the faulty head_y
    assert fY > 1 and fO < 1, (fY, fO)
    m = out.clone(); m[:, -4:] = 0
    fY, fO = ES.head_ratios(HW, cls_b, y, m)
    assert fY < 1 and fO > 1, (fY, fO)
    # a weight that was not rounded to bf16 on the way in is another product: the bound is fp32-tight
    lin_mod = ES.make_head(s.H, E)[0]
    y32 = ES.lin(cls_b, lin_mod.weight.detach().double(), HW.b, F32)
    assert ES.head_ratios(HW, cls_b, y32, out)[0] > 1


@pytest.mark.parametrize("H", [128, 256, 384, 512, 640, 768, 896, 1024])
def test_layouts_mirror_at_input_s(H):
    """ES.layouts() restates csrc/encoder.hip:encoder_layer_forward's dispatch.  At input S (2,064 rows) under the default options
    every hand-off is row-major for every admitted hidden size; Y holds FFN2's pre-LayerNorm sums everywhere but at 768 with a
    long contraction, where the split-contraction slab takes its place.  The envelope GPU test asserts this answer per run; here
    it is pinned for all eight sizes so that the mirror cannot rot silently."""
    rows = int(((np.asarray(LENS_S) + 7) // 8 * 8).sum())
    assert rows == 2064 and dict(ES._opts) == dict(ES.DEFAULTS)
    for I in (64, 192, 320, 448, 1024, 2304, 3072, 4096):
        lo = ES.layouts(rows, H, I)
        assert lo == dict(qk=False, ctx=False, hm=False, y_live=not (H == 768 and I >= 2048)), (H, I, lo)
    # the fused kernel is keyed on H == 768 alone: lowering its row threshold changes nothing elsewhere
    ES._opts["fused_ln_min_rows"] = 1
    try:
        lo = ES.layouts(rows, H, 1024)
        assert (lo["qk"], lo["ctx"], lo["y_live"]) == ((True, True, False) if H == 768 else (False, False, True))
    finally:
        ES._opts["fused_ln_min_rows"] = ES.DEFAULTS["fused_ln_min_rows"]
