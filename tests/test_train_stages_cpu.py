"""The stage references and bounds of tests/train_stages.py, checked without a GPU:
  * a correct stand-in for the library (TS.sim_run: every stage with fp32 accumulation and the kernels' rounding points, the
    oracle's kernel-arithmetic attention, the oracle's dropout masks) passes the very walk over the stages the GPU test does --
    every derived ratio < 1, the measured stage (the attention backward) inside the caps taken from its reference pair, the
    stand-in there being a THIRD computation (the fp32 chain over the tokens in another order), not the pair's own member;
  * every planted fault breaks the check of the stage it was planted in -- and of no stage in front of it;
  * the reference pair of the measured stage stays at flip level (c < 0.02, f < 2 %) on these inputs.
Models W (768 / 12 / 3072), N (384 / 6 / 320) and the six ES.ENVELOPE shapes (128 / 64, 256 / 192, 512 / 1024, 640 / 448,
896 / 2304, 1024 / 4096: the stand-in at all six, the planted faults at 640 / 448 and 1024 / 4096), two layers each; sequences on
both sides of 8 and 64 rows and one beyond 128.
Run with -s to see the ratios."""
import numpy as np
import pytest
import torch

from oracle import dropout as OD
from tests import encoder_stages as ES
from tests import train_stages as TS

LENS = [1, 9, 64, 65, 130]
DROP = (0.1, 0.1, 7)
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _MODELS.clear()
    ES._MEMO.clear()


def model(shape):
    if shape not in _MODELS:
        m = ES.make_model(shape, "init")
        _MODELS[shape] = (ES.Weights(m.roberta), TS.Head(m))
    return _MODELS[shape]


def walk(shape, pool_mean, gelu_gp, drop, fault=None):
    W, HD = model(shape)
    ids, lens = ES.make_inputs(LENS, 1000, 3)
    res = TS.sim_run(W, HD, ids, lens, pool_mean, drop, gelu_gp, fault)
    rep = TS.Report()
    TS.check_forward(res, W, HD, lens, drop, rep, memo_key=shape)
    TS.check_backward(res, W, HD, lens, drop, rep, gelu_gp, 64, memo_key=shape)
    return rep


@pytest.mark.parametrize("shape,pool_mean,gelu_gp,drop", [("W", 0, 1, None), ("W", 1, 0, None), ("W", 0, 0, DROP), ("W", 1, 1, DROP),
                                                          ("N", 0, 0, None), ("N", 1, 1, None), ("N", 0, 1, DROP), ("N", 1, 0, DROP)] +
                         [(sh,) + c for sh in ES.ENVELOPE for c in ((0, 1, None), (1, 0, DROP))])
def test_stand_in_passes_every_stage(shape, pool_mean, gelu_gp, drop):
    rep = walk(shape, pool_mean, gelu_gp, drop)
    for n, v, b in rep.items:
        print("%s %s %.4g (bar %.4g)" % (shape, n, v, b))
    assert not rep.failures(), rep.failures()
    names = [n for n, _, _ in rep.items]
    for must in ("fwd/A", "fwd/l0/LSE", "fwd/l0/Y1", "bwd/head_ln/2/dXb", "bwd/l0/LN1'/dXf", "bwd/l0/bk/full", "bwd/l0/wqkv/0", "bwd/l1/w2/full"):
        assert must in names, must
    # the reference pair of the measured stage stays inside its own caps: flips, not another function
    floors = [(n, v) for n, v, _ in rep.items if n.endswith("_c_floor") or n.endswith("_f_floor")]
    assert len(floors) == (4 if pool_mean else 2), floors
    for n, v in floors:
        assert v < 0.02, (n, v)


# fault -> (pool_mean, gelu_gp, dropout, the checks that must break: name prefixes)
FAULT_CASES = {
    "dgrad_trunc": (1, 1, None, ["bwd/l1/dXb1", "bwd/l0/dXb1"]),
    "head_trunc": (0, 1, None, ["bwd/head_ln/2/dXb"]),
    "ln_no_resid_half": (1, 1, None, ["bwd/l0/LN2'/dXf", "bwd/l0/LN2'/dXb", "bwd/l0/LN2'/0/dgamma"]),
    "ln_skip_row": (1, 1, DROP, ["bwd/l0/LN2'/dXf", "bwd/l0/LN2'/dXb", "bwd/l0/LN2'/full/dbias"]),
    "mask_compact_row": (0, 1, DROP, ["bwd/l1/c_dYb", "bwd/l1/cLN1'/dXb"]),
    "cast_no_mask": (0, 1, DROP, ["bwd/l1/c_dYb"]),
    "y1_mask_on_resid": (1, 1, DROP, ["fwd/l0/Y1"]),
    "gelu_of_hm": (0, 0, None, ["bwd/l1/c_dHpre_2r", "bwd/l0/dHpre_2r"]),
    "gp_of_hm": (1, 1, None, ["fwd/l0/Gp", "fwd/l1/Gp"]),
    "lse_natural": (0, 1, None, ["fwd/l0/LSE", "fwd/l1/LSE"]),
    "wgrad_skip_kstep": (1, 1, None, ["bwd/l0/w1/0", "bwd/l0/w1/full"]),
    "wgrad_lost_octet": (1, 1, None, ["bwd/l0/w2/0", "bwd/l1/w2/full"]),
    "bk_zero": (0, 1, None, ["bwd/l0/bk/0", "bwd/l1/bk/full", "bwd/l0/bqkv/full"]),
    "b1_unrounded": (1, 0, None, ["bwd/l0/b1/0"]),
    "scatter_row": (0, 1, None, ["bwd/l1/scatter_G0"]),
    "mean_pad_rows": (1, 1, None, ["bwd/mean"]),
    "c_dx1_no_resid": (0, 1, None, ["bwd/l1/c_dX1f"]),
    "att_d_other_head": (1, 1, None, ["bwd/l0/att'_c", "bwd/l1/att'_c"]),
    "att_no_scale": (0, 1, None, ["bwd/l0/att'_c", "bwd/l1/att'_tail"]),
    "att_kv_tile": (1, 1, None, ["bwd/l0/att'_c"]),
    "att_mask_other_layer": (1, 1, DROP, ["fwd/l0/C", "fwd/l0/Mbits"]),
    "att_mask_transposed": (0, 1, DROP, ["bwd/l0/att'_c", "bwd/l1/att'_tail"]),
    "mbits_bit": (0, 1, DROP, ["fwd/l0/Mbits"]),
    "emb_count_once": (0, 1, None, ["bwd/emb/word_emb"]),
}


# the checks a fault may break at all (substrings of their names): its own stage's
STAGE_OF = {"dgrad_trunc": ["/dXb1"], "head_trunc": ["/head_ln/"], "ln_no_resid_half": ["/LN2'"], "ln_skip_row": ["/LN2'"],
            "mask_compact_row": ["/c_dYb", "/cLN1'", "/b2_colsum"], "cast_no_mask": ["/c_dYb", "/b2_colsum"], "y1_mask_on_resid": ["/Y1"],
            "gelu_of_hm": ["dHpre"], "gp_of_hm": ["/Gp"], "lse_natural": ["/LSE"], "wgrad_skip_kstep": ["/w1/"],
            "wgrad_lost_octet": ["/w2/"], "bk_zero": ["/bk/", "/bqkv/"], "b1_unrounded": ["/b1/"], "scatter_row": ["/scatter_G0"],
            "mean_pad_rows": ["/mean"], "c_dx1_no_resid": ["/c_dX1f"], "att_d_other_head": ["/att'"], "att_no_scale": ["/att'"],
            "att_kv_tile": ["/att'"], "att_mask_other_layer": ["/C", "/Mbits"], "att_mask_transposed": ["/att'"],
            "mbits_bit": ["/Mbits"], "emb_count_once": ["/emb/word_emb"]}


def test_every_fault_has_a_case():
    assert sorted(FAULT_CASES) == sorted(TS.FAULTS)


@pytest.mark.parametrize("shape", ["W", "N", "H640", "H1024"])
@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_planted_fault_breaks_its_stage(fault, shape):
    pool_mean, gelu_gp, drop, must = FAULT_CASES[fault]
    rep = walk(shape, pool_mean, gelu_gp, drop, fault)
    failed = [n for n, _, _ in rep.failures()]
    print(fault, shape, [(n, "%.3g" % v) for n, v, _ in rep.failures()])
    for m in must:
        assert m in failed, (fault, m, failed)
    # teacher forcing: no other stage fails -- every stage is judged on the inputs it was given
    assert all(any(k in n for k in STAGE_OF[fault]) for n in failed), failed


def test_mask_rows_is_the_oracles_mask():
    lens = [3, 9, 17]
    H = 384
    want = OD.hidden_mask(DROP[2], OD.SITE_FFN_OUT, 1, DROP[0], lens, 17, H)
    cu = OD.packed_rows(lens)
    for b, n in enumerate(lens):
        got = TS.mask_rows(DROP, OD.SITE_FFN_OUT, 1, cu[b] + np.arange(n), H)
        assert np.array_equal(got.numpy().astype(np.float32), want[b, :n])
    assert not torch.equal(TS.mask_rows(DROP, OD.SITE_FFN_OUT, 1, [8], H), TS.mask_rows(DROP, OD.SITE_FFN_OUT, 1, [1], H))


def test_att_mask_seq_and_mbits_are_the_oracles_mask():
    lens, heads = [3, 70, 130], 6
    want = OD.attention_mask(DROP[2], 1, DROP[1], lens, 130, heads)
    cu = OD.packed_rows(lens)
    mb = torch.zeros(heads, 8, int(cu[-1]), dtype=torch.int64)
    for b, n in enumerate(lens):
        got = TS.att_mask_seq(DROP, 1, int(cu[b]), n, heads)
        assert np.array_equal(got.numpy().astype(np.float32), want[b, :, :n, :n])
        # the forward's words, written key by key from the layout's definition
        key = torch.arange(n)
        piece, bit = 2 * (key >> 6) + ((key >> 3) & 1), 16 * ((key >> 5) & 1) + 8 * ((key >> 4) & 1) + (key & 7)
        for h in range(heads):
            for k in range(n):
                mb[h, int(piece[k]), int(cu[b]):int(cu[b]) + n] |= (torch.from_numpy(want[b, h, :n, k] != 0).to(torch.int64) << int(bit[k]))
        assert torch.equal(TS.decode_mbits(mb.to(torch.int32), int(cu[b]), n), got != 0)


def test_wgrad_bound_at_many_rows():
    """At input M's row count the weight-gradient bound still sees one lost 32-row K step and one lost octet."""
    g = torch.Generator().manual_seed(3)
    dy, x = ES.bf16r(torch.randn(3920, 64, generator=g) * 1e-3), ES.bf16r(torch.randn(3920, 96, generator=g))
    ref, bound = TS.wgrad_ref(dy, x, TS.wgrad_slices(3920, 2))
    assert TS.wgrad_slices(3920, 2) == 1 and TS.wgrad_slices(1288, 2) == 1 and TS.wgrad_slices(4096, 2) == 2
    assert TS.ratio(TS.wgrad_sim(dy, x), ref, bound) < 1
    assert TS.ratio(TS.wgrad_sim(dy, x, skip=(1024, 32)), ref, bound) > 1
    assert TS.ratio(TS.wgrad_sim(dy, x, trunc_octet=(5, 8)), ref, bound) > 1


def test_gelu_grad_fit_is_within_its_stated_error():
    x = torch.linspace(-12, 12, 200001, dtype=torch.float64)
    assert float((TS.gelu_grad_fit(x) - TS.gelu_grad_exact(x)).abs().max()) < TS.GP_FIT_ERR
    assert float((TS.gelu_grad_fit(x.float()).double() - TS.gelu_grad_exact(x)).abs().max()) < TS.GP_FIT_ERR
    # the constants behind the forward bounds: |gelu'| <= 1.13, |gelu''| <= 0.8
    g = TS.gelu_grad_exact(x)
    assert float(g.abs().max()) < 1.13 and float(((g[1:] - g[:-1]) / (x[1] - x[0])).abs().max()) < 0.8


def test_layout_names_match_the_documented_count():
    assert len(TS.LAYER_SAVE) == 10 and len(TS.LAYER_BWD) == 4 and len(TS.GLOBALS) == 28
