"""The inference forward (csrc/encoder.hip) at every model shape its check_config admits, stage by stage -- the six hidden sizes
besides 768 (model W) and 384 (model N), which tests/test_encoder_stages_gpu.py covers on every path.  Same mechanism, same
references, same bounds (tests/encoder_stages.py; shown to catch planted faults at these shapes by
tests/test_encoder_stages_cpu.py); the harness is test_encoder_stages_gpu's own.  Everything runs on input S (2,064 packed rows,
16 sequences: a smaller input leaves the stage D reference pair without a single flip at 128 and 256, i.e. a bar of 0).  The
training step at the same shapes: tests/test_train_stages_gpu.py::test_shape_envelope_training_step.

Which shape reaches which kernel (read from encoder.hip, gemm_launch.hpp, cls_fold.hpp, encoder_kernels.hpp; rows = 2,064):
  every shape          off 768 nothing is fused and nothing blocked: row-major Q / K / ctx / Hm (k_gemm<.., MSHAPE 0>, the 32x32x16
                       loop), k_attention_fwd<false>, whole-contraction attention-output and FFN2 GEMMs (EPI_RESID_F32) + the general
                       k_layernorm on Y (stage E), k_embed_ln / k_layernorm lanes own 256 j + 4 lane behind `e0 < H`, k_masked_mean
                       / k_gather_cls with thread t on columns 4 t
  shape  H / heads / I   QKV tiles (N = 3 H)              FFN1 (N = I)                 k_layernorm groups   k_cls_pool
  H128   128 /  2 /   64  128 (H % 256 != 0), 3 wide       half a 128-tile; FFN2 K = 64   0.5                  <1>  14 of 16 N lanes masked
  H256   256 /  4 /  192  128; policy 1: 256, third = 1    1.5 tiles of 128               1                    <2>
  H512   512 /  8 / 1024  128; policy 1: 256, third = 2    I % 256 == 0: cost model       2                    <4>
  H640   640 / 10 /  448  128 under every policy           3.5 tiles of 128               2.5                  <5>  HQ = 160
  H896   896 / 14 / 2304  128 under every policy           I % 256 == 0: cost model       3.5                  <7>  bounds (256, 1), HQ = 224
  H1024 1024 / 16 / 4096  128; policy 1: 256, third = 4    I % 256 == 0: cost model       4 (every lane live)  <8>  bounds (256, 1), no lane masked
  (with <3> at 384 and <6> at 768 in test_encoder_stages_gpu.py's test_cls_tail all eight k_cls_pool instantiations run)
  gemm_tile_policy     1 / 2 / 3 reach a GEMM only where N % 256 == 0 (QKV: and H % 256 == 0; 2 not at all for QKV): at 128, 640,
                       896 the QKV launcher must stay on 128-tiles; attention-output and FFN2 (N = H) follow H % 256, FFN1 I % 256.
                       With 256-tiles the V third is found by c.n0 + third0 * H >= 2 * H at one, two and four tiles per third
  cls (stage F)        fold 1: k_gather_cls, the B-row Q GEMM (EPI_BF16), k_cls_key_fold / k_cls_pool<H / 128> / k_cls_value_fold
                       (grid.y = heads, loops over H in steps of 128); fold 0: the K / V-only projection (N = 2 H, third0 = 1) +
                       k_attention_fwd<true>; then the B-row tail: attention-output + k_layernorm, FFN1, FFN2 (EPI_RESID_F32) and
                       k_layernorm(cls).  The fold needs B * heads * H * 4 bytes in the K and in the V^T buffer:
                       2 B heads <= rows + 64, i.e. 512 <= 2,128 at 16 heads -- asserted per case
  head (stage G)       launch_gemm<EPI_F32> with N = out_dim 4 (one quad of one 128-tile), 132 (a tile and a quad) and 1024, K = 640
                       and 1024, + k_layernorm with H = out_dim (4: one lane, one group); after the CLS tail and after k_masked_mean
  stale memory         layer 1 and both CLS tails a second time, workspace and output 0xFF-filled: identical bytes
  ragged               convdr_encoder_forward_ragged at 640 and 1024 (the code behind the packing kernel is shared): bit-equal
Stage D at 128: with 128 x 2,064 elements the reference pair of one layer holds at most one element beyond its 2 u allowance.  At
layer 2 the pair has none (c_ref = 0) while the GPU's X_2 has one at c = 1.84e-4; at layer 1 it is the other way round (pair
2.55e-4, GPU 0).  A floor of 0 would be a bar of 0, so for these cases a zero floor is replaced by the same pair's floor on the
other layer's inputs (check_layer's `other`; bar 1.02e-3 there).  No other shape or stage needs it.
Every ratio is recorded with tests.helpers.margin under envelope/<shape>-init-S/...; gemm_tile_policy: whether the X_1 bytes equal
the cost model's is recorded, not asserted (test_encoder_stages_gpu.py says why).  Off 768 this is the unfused, row-major path:
correct at every admitted shape is what these cases say, how fast it is nobody has measured."""
import pytest
import torch

from tests import encoder_stages as ES
from tests import test_encoder_stages_gpu as SG
from tests.helpers import margin

pytestmark = pytest.mark.gpu

ROOT = "envelope"
HC = {"H128": 1, "H256": 2, "H512": 4, "H640": 5, "H896": 7, "H1024": 8}     # the k_cls_pool<HC> a shape's folded CLS tail runs


def _drop(shape=None):
    """Forget the runs, references and the model of `shape` (None: of every shape): a 1024 / 4096 run is ~170 MB of fp64."""
    for k in [k for k in SG._RUNS if shape is None or k[0] == shape]:
        del SG._RUNS[k]
    for k in [k for k in SG._TOWERS if shape is None or k[0] == shape]:
        del SG._TOWERS[k]
    ES._MEMO.clear()


@pytest.fixture(scope="module", params=ES.ENVELOPE)
def shape(request):
    """Module-scoped, so that pytest runs the cases shape by shape and one shape's runs and references are shared by its cases."""
    yield request.param
    _drop(request.param)


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _drop()


@pytest.mark.parametrize("l", [0, 1, 2])
def test_default_path_stage_by_stage(shape, l):
    """Stages A (l = 0), B, C, D, E and the pooled mean (l = 1, 2) under the default options."""
    cur = SG.check_case(shape, "init", "S", l, root=ROOT, zero_floor_from_other_layer=True)
    ids, lens = SG.inputs("S")
    tid, tpos = ES.host_tokens(ids, lens)
    assert torch.equal(cur["tok_id"], tid) and torch.equal(cur["tok_pos"], tpos)
    assert cur["layout"] == dict(qk=False, ctx=False, hm=False, y_live=True)
    if l >= 1:
        assert "Y" in cur                                                                   # stage E ran on the general LayerNorm


@pytest.mark.parametrize("policy", [1, 2, 3])
def test_gemm_tile_policies(shape, policy):
    cur = SG.check_case(shape, "init", "S", 1, (("gemm_tile_policy", policy),), tag="tiles%d" % policy, root=ROOT,
                        zero_floor_from_other_layer=True)
    assert "Y" in cur
    base = SG.run(shape, "init", "S", 1)
    same = torch.equal(base["X_bits"], cur["X_bits"])
    print("%s tiles%d: X_1 bytes %s the cost model's tiles'" % (shape, policy, "equal" if same else "differ from"))
    margin("%s/%s-init-S/tiles%d/X_bits_equal_default_tiles" % (ROOT, shape, policy), float(same), 1.0)


@pytest.mark.parametrize("l", [1, 2])
@pytest.mark.parametrize("fold", [1, 0])
def test_cls_tail(shape, fold, l):
    """Stage F with the floor rule of test_encoder_stages_gpu.py::test_cls_tail.  fold 1 runs k_cls_pool<HC[shape]>: <1> at H128,
    <2> at H256, <4> at H512, <5> at H640, <7> at H896, <8> at H1024 -- provided the fold's buffers fit, which is
    encoder_layer_forward's own condition restated here."""
    H, _ = ES.SHAPES[shape]
    _, lens = SG.inputs("S")
    B, rows = len(lens), int(((lens + 7) // 8 * 8).sum())
    ldt = (rows + 64 + 7) // 8 * 8
    fold_bytes = B * (H // 64) * H * 4
    assert fold_bytes <= (rows + 128) * H * 2 and fold_bytes <= H * ldt * 2 and HC[shape] == H // 128
    SG.check_cls_tail(shape, "init", fold, l, root=ROOT)


def test_stale_memory(shape):
    """Layer 1 and both CLS tails twice, each run on a workspace and an output pre-filled with 0xFF bytes (every bf16 / fp32 a NaN;
    the second run's buffers come out of the allocator holding the first run's results until that fill): identical bytes, and
    run_layers itself refuses a live row that is not finite -- no element left unwritten, nothing read before it is written."""
    ids, lens = SG.inputs("S")
    tw = SG.tower(shape, "init")[0]
    a = SG.run(shape, "init", "S", 1)
    b = ES.run_layers(tw, ids, lens, 1)
    for k in ("X_bits", "Q", "K", "V", "ctx", "Hm", "Y", "out"):
        assert torch.equal(a[k], b[k]), k
    for fold in (1, 0):
        opts = (("cls_fold", fold), ("cls_fold_min_rows", 1))
        a = SG.run(shape, "init", "S", 1, opts, cls=True)
        with ES.options(**dict(opts)):
            b = ES.run_layers(tw, ids, lens, 1, cls=True)
        assert torch.equal(a["out"], b["out"]), fold


@pytest.mark.parametrize("shape", ["H640", "H1024"])
def test_ragged_entry_is_bit_equal(shape):
    cur = SG.run(shape, "init", "S", 2)
    rag = SG.run(shape, "init", "S", 2, ragged=True)
    for k in ("X_bits", "tok_id", "tok_pos", "Hm", "ctx"):
        assert torch.equal(rag[k], cur[k]), k


@pytest.mark.parametrize("cls", [True, False])
@pytest.mark.parametrize("E", [4, 132, 1024])
@pytest.mark.parametrize("shape", ["H640", "H1024"])
def test_head(shape, E, cls):
    """Stage G: the model's head replaced by Linear(H, E) + LayerNorm(E), teacher-forced on the GPU's own cls_b (the bf16 pooled
    row: of the CLS tail, or of k_masked_mean) and on its own head_y; both bounds derived (ES.head_ratios), ratio < 1."""
    H, _ = ES.SHAPES[shape]
    tw = SG.tower(shape, "init")[0]
    ids, lens = SG.inputs("S")
    lin_mod, ln_mod = ES.make_head(H, E)
    HW = ES.HeadWeights(lin_mod, ln_mod)
    head = (lin_mod.cuda(), ln_mod.cuda())
    tw.invalidate_packed()
    try:
        cur = ES.run_layers(tw, ids, lens, 2, cls=cls, head=head)
    finally:
        tw.invalidate_packed()
    assert cur["out"].shape == (len(lens), E) and cur["head_y"].shape == (len(lens), E)
    # cls_b is the pooled fp32 row of the run without a head, rounded to bf16
    assert torch.equal(cur["cls_b"], ES.bf16r(SG.run(shape, "init", "S", 2, cls=cls)["out"]))
    rY, rO = ES.head_ratios(HW, cur["cls_b"], cur["head_y"], cur["out"])
    tag = "%s/%s-init-S/head,E%d,%s" % (ROOT, shape, E, "cls" if cls else "mean")
    print("%s G: head_y ratio %.3g  out ratio %.3g" % (tag, rY, rO))
    margin(tag + "/G_head_y_ratio", rY, 1.0)
    margin(tag + "/G_out_ratio", rO, 1.0)
    assert rY < 1 and rO < 1
