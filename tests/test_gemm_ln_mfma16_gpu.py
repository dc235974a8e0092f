"""The fused projection + residual + LayerNorm kernel (csrc/gemm_ln.hpp k_gemm_resid_ln: main loop ln_mainloop on the 16x16x32
MFMA over an LDS image swizzled by ln_swz, the epilogue on 16 x 16 accumulator blocks) against the stage references of
tests/encoder_stages.py, every live token.

Options of every case: fused_ln_min_rows 1, fused_ln_max_k 2^20, gemm_tile_policy 1; K-slice-major weights unless a case says
otherwise.  Both launches of a layer are the kernel under test: attention output (K = 768, A = ctx) and FFN2 (K = 3,072,
A = Hm).  Hm is computed from the first launch's output X1, X_l by the second, so stage D on Hm and X_l covers both.
  S  (ES.input_s, 2,064 packed rows: 17 token tiles of 128, the last one 16 rows) -- ctx blocked, Hm row-major (the blocked
     FFN hand-off needs 192 FFN1 tiles), so the K = 3,072 launch streams row-major activations here.
  P  (7,768 packed rows, no multiple of 32: 61 token tiles, the last one 88 rows, its last 32-token block ends past `rows`)
     -- ctx and Hm blocked.  Variants: hm_blocked = 0 (row-major ctx and Hm) and row-major weights (Wks null).
Bars: the existing stage D ones (ES.tail_chain, ES.tail_bars: c <= 4 c_ref, f <= max(10 f_ref, 1 %) against the fp64 /
fp32-accumulating reference pair on the GPU's own inputs); margins are recorded with tests.helpers.margin, which asserts them.
The margin tags keep the "m1" of the time when a switch chose between this kernel (1) and a 32x32x16 one (0, retired).
"""
import numpy as np
import pytest
import torch

from tests import encoder_stages as ES
from tests.encoder_stages import F32
from tests.helpers import margin

pytestmark = pytest.mark.gpu

OPTS = dict(fused_ln_min_rows=1, fused_ln_max_k=1 << 20, gemm_tile_policy=1)
LENS_P = [128] * 59 + [127, 65, 9]
VARIANTS = {"base": (dict(), True), "rowmajor_a": (dict(hm_blocked=0), True), "rowmajor_w": (dict(), False)}
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _CACHE.clear()
    ES._MEMO.clear()


def tower():
    if "tower" not in _CACHE:
        model = ES.make_model("W", "init")
        W = ES.Weights(model.roberta)
        _CACHE["tower"] = (model.cuda().eval().roberta, W)
    return _CACHE["tower"]


def inputs(name):
    if name == "S":
        ids, lens = ES.input_s()
        rows = int(((np.asarray(lens) + 7) // 8 * 8).sum())
        assert rows == 2064 and (rows + 127) // 128 == 17 and rows % 128 == 16
        return ids, lens
    rows = int(((np.asarray(LENS_P) + 7) // 8 * 8).sum())
    assert rows == 7768 and rows % 32 != 0 and rows % 128 == 88
    return ES.make_inputs(LENS_P, 1000, 3)


def run(inp, l, variant="base", fresh=False):
    key = (inp, l, variant)
    if fresh or key not in _CACHE:
        ids, lens = inputs(inp)
        extra, kslice = VARIANTS[variant]
        with ES.options(kslice=kslice, **OPTS, **extra):
            r = ES.run_layers(tower()[0], ids, lens, l, kslice=kslice)
        if fresh:
            return r
        _CACHE[key] = r
    return _CACHE[key]


def check_tail(tag, l, prev, cur):
    """Stage D on Hm and X_l of layer l; prev = the run cut off one layer earlier (teacher forcing)."""
    W = tower()[1]
    x = prev["X"]
    (hm64, x64, _), (hm32, x32, _) = ES.memo(("D", id(W), l), [cur["ctx"], x], lambda: (
        ES.tail_chain(W, l, cur["ctx"], x), ES.tail_chain(W, l, cur["ctx"], x, acc=F32)))
    for name, g, r64, r32 in (("Hm", cur["Hm"], hm64, hm32), ("X", cur["X"], x64, x32)):
        c_ref, f_ref = ES.tail_metrics(r32, r64)
        c_bar, f_cap = ES.tail_bars(c_ref, f_ref)
        c, f = ES.tail_metrics(g, r64)
        print("%s D %s: c %.3g (floor %.3g, bar %.3g)  f %.3g%% (floor %.3g%%, cap %.3g%%)" % (tag, name, c, c_ref, c_bar, 100 * f,
                                                                                              100 * f_ref, 100 * f_cap))
        margin("ln_mfma16/%s/D_%s_c" % (tag, name), c, c_bar)
        margin("ln_mfma16/%s/D_%s_f" % (tag, name), f, f_cap)


@pytest.mark.parametrize("l", [1, 2])
@pytest.mark.parametrize("inp", ["S", "P"])
def test_tail_stages(inp, l):
    """Inputs S and P, layers 1 and 2, every live token: Hm (behind the K = 768 launch) and X_l (the K = 3,072 launch)."""
    cur = run(inp, l)
    lo = cur["layout"]
    assert lo["qk"] and lo["ctx"] and lo["hm"] == (inp == "P") and not lo["y_live"]
    check_tail("%s/m1/l%d" % (inp, l), l, run(inp, l - 1), cur)


@pytest.mark.parametrize("variant", ["rowmajor_a", "rowmajor_w"])
def test_operand_layouts(variant):
    """Input P, one layer, with row-major activations (hm_blocked = 0) and with row-major weights (no K-slice-major copy)."""
    cur = run("P", 1, variant)
    lo = cur["layout"]
    assert lo["hm"] == (variant != "rowmajor_a") and lo["ctx"] == lo["hm"] and not lo["y_live"]
    check_tail("P/%s/m1/l1" % variant, 1, run("P", 0, variant), cur)


def test_stale_memory():
    """Input P twice, each on a workspace and an output pre-filled with 0xFF bytes (every bf16 / fp32 a NaN; the second run's
    buffers come out of the allocator holding the first run's results until that fill): identical bytes, and run_layers
    itself refuses a live row that is not finite -- no element left unwritten, nothing read before it is written."""
    a = run("P", 1)
    b = run("P", 1, fresh=True)
    for k in ("X_bits", "Q", "K", "V", "ctx", "Hm", "out"):
        assert torch.equal(a[k], b[k]), k


def test_switch():
    """The switch between this kernel and the retired 32x32x16 one is gone: its name is an unknown option."""
    from convdr_amd import _lib
    assert _lib.lib().convdr_set_option(b"ln_mfma16", 1) != 0
