"""The inference forward (csrc/encoder.hip) stage by stage, every live token, every path -- see tests/encoder_stages.py for
the mechanism, the stage table and the bounds, tests/test_encoder_stages_cpu.py for what the bounds were shown to catch.

Which case runs which path (rows = packed rows; S = 2,064 rows, M = 3,9xx rows):
  default W/S, N/S     128 x 128 tiles everywhere (N/S: N = 1152 and I = 320 with a partial feature tile, K = 320), row-major
                       Q / K / ctx / Hm, k_attention_fwd<false>, W: 4-slice split-contraction FFN2 + k_slab_finish_ln,
                       attention-output GEMM + k_layernorm_rows<3>; N: whole-contraction GEMMs + the general k_layernorm (Y live)
  ffn2_splitk 0        whole-contraction FFN2 (EPI_RESID_F32) + k_layernorm_rows<3>; + ln_rows 0: the general k_layernorm
  gemm_tile_policy     1: 256 x 256, 2: 256 x 128, 3: 128 x 128 tiles, ragged last token tile (2,064 = 8 x 256 + 16)
  fused S / M          k_gemm_resid_ln at K = 768 and K = 3072 (row-major and K-slice-major weights), blocked Q / K / ctx,
                       k_attention_fwd<false, true, true>; M: blocked Hm (EPI_GELU_BLK) with hm_blocked 1, all row-major with 0
  cls (stage F)        the last layer's CLS tail: fold (k_cls_key_fold / k_cls_pool / k_cls_value_fold) and no fold
                       (K / V-only projection + k_attention_fwd<true>; with the fused options k_attention_fwd<true, false, true>)
  ragged               convdr_encoder_forward_ragged: bit-equal X_l
gemm_tile_policy: the X_l bytes may NOT differ between tile shapes -- every tile shape walks the contraction in the same order
per output element -- so equality is recorded, not asserted against; that the policy reaches the launcher is the business of
the launcher's own selection code, read in csrc/gemm_launch.hpp."""
import numpy as np
import pytest
import torch

from tests import encoder_stages as ES
from tests.encoder_stages import F32
from tests.helpers import margin

pytestmark = pytest.mark.gpu

_TOWERS, _RUNS = {}, {}
FUSED = dict(fused_ln_min_rows=1, fused_ln_max_k=1 << 20)


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    """The runs and references are shared between the cases of this module and dropped behind it."""
    yield
    _TOWERS.clear()
    _RUNS.clear()
    ES._MEMO.clear()


def tower(shape, stats):
    if (shape, stats) not in _TOWERS:
        model = ES.make_model(shape, stats)
        W = ES.Weights(model.roberta)
        _TOWERS[(shape, stats)] = (model.cuda().eval().roberta, W)
    return _TOWERS[(shape, stats)]


def inputs(name):
    return ES.input_s() if name == "S" else ES.input_m()


def run(shape, stats, inp, l, opts=(), **kw):
    """run_layers under the options `opts` (a tuple of (name, value)), cached: X_{l-1} of one case is layer l's input."""
    key = (shape, stats, inp, l, opts, tuple(sorted(kw.items())))
    if key not in _RUNS:
        ids, lens = inputs(inp)
        o = dict(opts)
        with ES.options(kslice=kw.get("kslice", False), **o):
            _RUNS[key] = ES.run_layers(tower(shape, stats)[0], ids, lens, l, **kw)
    return _RUNS[key]


def d_refs(W, l, ctx, x):
    """The reference pair of stage D on the inputs (ctx, X_{l-1}): the fp64 chain and the fp32-accumulating one."""
    return ES.memo(("D", id(W), l), [ctx, x], lambda: (ES.tail_chain(W, l, ctx, x), ES.tail_chain(W, l, ctx, x, acc=F32)))


def check_layer(tag, W, lens, l, prev, cur, root="stages", other=None):
    """Stages A (l = 0) or B, C, D, E (l >= 1) of one run; prev = the run cut off one layer earlier.  Margins go under
    `root`/`tag`/.
    other: () -> (l', prev', cur') of the model's other all-token layer on the same input.  The stage D floor c_ref is the sample
    maximum of a rare event (a flip in X1 or Hm that reaches the output beyond its 2 u allowance: at 128 x 2,064 elements the
    pair of one layer shows one such element, or none).  A pair that sampled none has c_ref = 0 and would make the bar 0 -- a
    statement about the sample, not about the function: a correct kernel with another summation order has its own flips, as
    the pair's fp32 member has on the other layer.  Then, and only then, c_ref is taken from the same chain's pair on the
    other layer's GPU inputs (the same weights' statistics, the same rows, the same metric; nothing of the output under test
    enters it).  If that pair is 0 too, the bar stays 0."""
    H = W.H
    if l == 0:
        ref, e32 = ES.embed_ref(W, cur["tok_id"], cur["tok_pos"])
        r = ES.ratio_bf16_of_fp32(cur["X"], ref, e32)
        print("%s A ratio %.3f" % (tag, r))
        margin(root + "/%s/A_ratio" % tag, r, 1.0)
        assert r < 1
        return
    L = W.layers[l - 1]
    x = prev["X"]
    # B
    y, bound = ES.memo(("B", id(W), l), [x], lambda: ES.proj_ref(x, L["wqkv"], L["bqkv"]))
    got = torch.cat([cur["Q"], cur["K"], cur["V"]], 1)
    rB = float(((got - y).abs() / bound).max())
    # C
    ref, bound, _ = ES.memo(("C", id(W), l), [got], lambda: ES.per_sequence(
        lens, lambda q, k, v: ES.attention_ref(q, k, v, W.heads), cur["Q"], cur["K"], cur["V"]))
    rC = float(((cur["ctx"] - ref).abs() / bound).max())
    print("%s B ratio %.3f  C ratio %.3f" % (tag, rB, rC))
    margin(root + "/%s/B_ratio" % tag, rB, 1.0)
    margin(root + "/%s/C_ratio" % tag, rC, 1.0)
    assert rB < 1 and rC < 1
    # D: floors from the reference pair on the GPU's own inputs, bars from the floors
    (hm64, x64, _), (hm32, x32, _) = d_refs(W, l, cur["ctx"], x)
    for name, g, r64, r32 in (("Hm", cur["Hm"], hm64, hm32), ("X", cur["X"], x64, x32)):
        c_ref, f_ref = ES.tail_metrics(r32, r64)
        if c_ref == 0 and other is not None:
            lo, po, co = other()
            pair = dict(zip(("Hm", "X"), zip(*[t[:2] for t in d_refs(W, lo, co["ctx"], po["X"])])))[name]
            c_ref = ES.tail_metrics(pair[1], pair[0])[0]
            print("%s D %s: the pair of layer %d sampled no flip beyond 2 u; floor %.3g of layer %d's pair" % (tag, name, l, c_ref, lo))
        c_bar, f_cap = ES.tail_bars(c_ref, f_ref)
        c, f = ES.tail_metrics(g, r64)
        print("%s D %s: c %.3g (floor %.3g, bar %.3g)  f %.3g%% (floor %.3g%%, cap %.3g%%)" % (tag, name, c, c_ref, c_bar, 100 * f,
                                                                                              100 * f_ref, 100 * f_cap))
        margin(root + "/%s/D_%s_c" % (tag, name), c, c_bar)
        margin(root + "/%s/D_%s_f" % (tag, name), f, f_cap)
    # the pooled output of a pool_mean run: k_masked_mean adds the sequence's rows of X_l in fp32, in order
    xs = ES.per_sequence(lens, lambda t: (t.mean(0, keepdim=True), t.abs().mean(0, keepdim=True) * (t.shape[0] + 2) * ES.E24), cur["X"])
    rM = float(((cur["out"] - xs[0]).abs() / (xs[1] + 1e-300)).max())
    margin(root + "/%s/mean_ratio" % tag, rM, 1.0)
    # E
    if "Y" in cur:
        yv = cur["Y"]
        ref, e32 = ES.ln(yv, L["ln2_g"], L["ln2_b"], W.eps), ES.ln_fp32_err(yv, L["ln2_g"], L["ln2_b"], W.eps)
        rE = ES.ratio_bf16_of_fp32(cur["X"], ref, e32)
        print("%s E ratio %.3f" % (tag, rE))
        margin(root + "/%s/E_ratio" % tag, rE, 1.0)
        assert rE < 1


def check_case(shape, stats, inp, l, opts=(), tag=None, root="stages", zero_floor_from_other_layer=False, **kw):
    W = tower(shape, stats)[1]
    lens = [int(n) for n in inputs(inp)[1]]
    cur = run(shape, stats, inp, l, opts, **kw)
    prev = run(shape, stats, inp, l - 1, opts, **kw) if l else None
    tag = "%s-%s-%s/%s/l%d" % (shape, stats, inp, tag or "default", l)
    other = None
    if zero_floor_from_other_layer and l >= 1:   # (two-layer models: the other all-token layer of 1 is 2 and of 2 is 1; default options)
        other = lambda: (3 - l, run(shape, stats, inp, 2 - l), run(shape, stats, inp, 3 - l))
    check_layer(tag, W, lens, l, prev, cur, root, other)
    return cur


MODELS = [("W", "init"), ("W", "trained"), ("N", "init")]


@pytest.mark.parametrize("l", [0, 1, 2])
@pytest.mark.parametrize("shape,stats", MODELS)
def test_default_path_stage_by_stage(shape, stats, l):
    cur = check_case(shape, stats, "S", l)
    ids, lens = inputs("S")
    tid, tpos = ES.host_tokens(ids, lens)
    assert torch.equal(cur["tok_id"], tid) and torch.equal(cur["tok_pos"], tpos)          # (pad ids inside two sequences)
    # the premise of teacher forcing: the forward is bitwise deterministic, so X_{l-1} of the run cut off at l - 1 IS what
    # layer l consumed in the run cut off at l
    again = ES.run_layers(tower(shape, stats)[0], ids, lens, l)
    assert torch.equal(again["X_bits"], cur["X_bits"])
    if shape == "N":
        assert "Y" in cur or l == 0                                                        # stage E ran on the general LayerNorm


VARIANTS = {
    "whole-k": (("ffn2_splitk", 0),),
    "whole-k,ln-general": (("ffn2_splitk", 0), ("ln_rows", 0)),
    "tiles256": (("gemm_tile_policy", 1),),
    "tiles256x128": (("gemm_tile_policy", 2),),
    "tiles128": (("gemm_tile_policy", 3),),
    "tiles256,whole-k": (("gemm_tile_policy", 1), ("ffn2_splitk", 0)),
    "tiles256x128,whole-k": (("gemm_tile_policy", 2), ("ffn2_splitk", 0)),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_option_variants_stage_by_stage(variant):
    opts = VARIANTS[variant]
    cur = check_case("W", "init", "S", 1, opts, tag=variant)
    assert ("Y" in cur) == (dict(opts).get("ffn2_splitk", 1) == 0)                         # stage E ran where Y is live
    if "gemm_tile_policy" in dict(opts):
        base = run("W", "init", "S", 1, tuple(o for o in opts if o[0] != "gemm_tile_policy"))
        same = torch.equal(base["X_bits"], cur["X_bits"])
        print("%s: X_1 bytes %s the cost model's tiles'" % (variant, "equal" if same else "differ from"))
        margin("stages/W-init-S/%s/X_bits_equal_default_tiles" % variant, float(same), 1.0)


@pytest.mark.parametrize("stats,inp,l,blk,kslice", [("init", "S", 1, 1, False), ("init", "S", 2, 1, False), ("init", "S", 1, 1, True),
                                                     ("trained", "S", 1, 1, False), ("init", "M", 1, 1, False),
                                                     ("init", "M", 1, 1, True), ("init", "M", 1, 0, False)])
def test_fused_projection_layernorm_and_blocked_handoffs(stats, inp, l, blk, kslice):
    opts = tuple(FUSED.items()) + (("hm_blocked", blk),)
    cur = check_case("W", stats, inp, l, opts, tag="fused,blk%d,ks%d" % (blk, kslice), kslice=kslice)
    lo = cur["layout"]
    assert lo["qk"] == bool(blk) and lo["ctx"] == bool(blk) and lo["hm"] == (bool(blk) and inp == "M") and not lo["y_live"]
    if kslice or not blk:   # same arithmetic in the same order: only where the bytes come from / go to differs
        base = run("W", stats, inp, l, tuple(FUSED.items()) + (("hm_blocked", 1),))
        assert torch.equal(base["X_bits"], cur["X_bits"])


def check_cls_tail(shape, stats, fold, l, fused=False, root="stages"):
    """Stage F: out [B, H] of a run whose last layer is the CLS tail, against the fp64 chain from X_{l-1}.  -> the run."""
    W = tower(shape, stats)[1]
    lens = [int(n) for n in inputs("S")[1]]
    prev = run(shape, stats, "S", l - 1)
    cur = run(shape, stats, "S", l, (tuple(FUSED.items()) if fused else ()) + (("cls_fold", fold), ("cls_fold_min_rows", 1)), cls=True)
    ref, sim = ES.memo(("F", id(W), l, fold), [prev["X"]], lambda: (ES.cls_chain(W, l, prev["X"], lens, bool(fold)),
                                                                  ES.cls_chain(W, l, prev["X"], lens, bool(fold), acc=F32)))
    # floor: the pair on the CLS rows, and -- 16 rows sample the flip-driven maximum poorly (a pair without a single flip in X1 or
    # Hm sits at 5e-7) -- the same chain's pair on all rows of the all-token layer l, unrounded output, same metric
    full = run(shape, stats, "S", l)
    (_, _, xf64), (_, _, xf32) = d_refs(W, l, full["ctx"], prev["X"])
    c_ref = max(ES.tail_metrics(sim, ref, rel=0.0)[0], ES.tail_metrics(xf32, xf64, rel=0.0)[0])
    c, _ = ES.tail_metrics(cur["out"], ref, rel=0.0)
    tag = "%s-%s-S/cls,fold%d%s/l%d" % (shape, stats, fold, ",fused" if fused else "", l)
    print("%s F: c %.3g (floor %.3g, bar %.3g)" % (tag, c, c_ref, 4 * c_ref))
    margin(root + "/%s/F_c" % tag, c, 4 * c_ref)
    return cur


@pytest.mark.parametrize("shape,stats,fold,l,fused", [(sh, st, fold, l, False) for sh, st in MODELS for fold in (1, 0) for l in (1, 2)] +
                         [("W", "init", 0, 1, True), ("W", "init", 1, 1, True)])
def test_cls_tail(shape, stats, fold, l, fused):
    """Stage F (check_cls_tail).  fused: with the fused-kernel options K arrives blocked (k_attention_fwd<true, false, true>)
    when the fold is off."""
    check_cls_tail(shape, stats, fold, l, fused)


def test_ragged_entry_is_bit_equal():
    cur = run("W", "init", "S", 2)
    rag = run("W", "init", "S", 2, ragged=True)
    for k in ("X_bits", "tok_id", "tok_pos", "Hm", "ctx"):
        assert torch.equal(rag[k], cur[k]), k
