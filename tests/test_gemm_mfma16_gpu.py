"""The 16x16x32 MFMA main loop of the inference forward's 256 x 256 QKV and FFN1 tiles (k_gemm<EPI_QKV / EPI_GELU_BLK, Tile256, 1>:
csrc/gemm_nt.hpp gemm_nt_mainloop_r3_m16, the blocked and V-third epilogues of csrc/gemm_kernel.hpp) against the stage
references of tests/encoder_stages.py, every live token.

Options of every case: fused_ln_min_rows 1, fused_ln_max_k 2^20, gemm_tile_policy 1, hm_blocked 1 -- Q / K / ctx blocked and
256 x 256 tiles wherever the shape allows.  Which kernel a case reaches (csrc/encoder.hip, csrc/gemm_launch.hpp):
  S  (ES.input_s, 2,064 packed rows = 8 x 256 + 16: 9 token tiles, the last one 16 rows -- its 32-token blocks end past `rows`)
     QKV: 9 x 9 = 81 tiles, one per workgroup, Q / K blocked, V through the parked image to V^T.  FFN1 keeps its row-major
     128 x 128 kernel here (the blocked hand-off needs 192 tiles), so Hm / X_l of S show the QKV kernel's consumers only.
  P  (7,768 packed rows = 30 x 256 + 88, no multiple of 32: 31 token tiles)
     QKV: 31 x 9 = 279 tiles, FFN1 (EPI_GELU_BLK): 31 x 12 = 372 tiles on 256 workgroups: each of the 8 XCD chunks (34-35 /
     46-47 tiles) is walked by 32 workgroups with stride 32, so workgroups take ONE or TWO tiles (QKV: 3 workgroups per chunk
     take two, FFN1: 14-15) -- the slot state handed to the second tile, its parked bias slice, `landed`, and the epilogue
     running under the next prologue are all exercised; no workgroup reaches a third tile at this size on 256 CUs.
Bars: the existing ones, nothing new -- stage B (Q, K, V: one rounding of an fp32 sum, ratio < 1) and stage D (Hm, and X_l read
back through FFN2: c <= 4 c_ref, f <= max(10 f_ref, 1 %) against the fp64 / fp32-accumulating reference pair on the GPU's own
inputs); margins are recorded with tests.helpers.margin, which asserts them.
The margin tags keep the "m1" of the time when a switch chose between this main loop (1) and the 32x32x16 one (0, retired for
these tiles).
"""
import numpy as np
import pytest
import torch

from tests import encoder_stages as ES
from tests.encoder_stages import F32
from tests.helpers import margin

pytestmark = pytest.mark.gpu

OPTS = dict(fused_ln_min_rows=1, fused_ln_max_k=1 << 20, gemm_tile_policy=1, hm_blocked=1)
LENS_P = [128] * 59 + [127, 65, 9]
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
        return ES.input_s()
    rows = int(((np.asarray(LENS_P) + 7) // 8 * 8).sum())
    assert rows == 7768 and rows % 32 != 0 and (rows + 255) // 256 == 31
    return ES.make_inputs(LENS_P, 1000, 3)


def run(inp, l, fresh=False):
    key = (inp, l)
    if fresh or key not in _CACHE:
        ids, lens = inputs(inp)
        with ES.options(**OPTS):
            r = ES.run_layers(tower()[0], ids, lens, l)
        if fresh:
            return r
        _CACHE[key] = r
    return _CACHE[key]


def check_stages(tag, l, prev, cur, lens):
    """Stage B on Q, K, V and stage D on Hm and X_l of layer l; prev = the run cut off one layer earlier (teacher forcing)."""
    W = tower()[1]
    L = W.layers[l - 1]
    x = prev["X"]
    y, bound = ES.memo(("B", id(W), l), [x], lambda: ES.proj_ref(x, L["wqkv"], L["bqkv"]))
    H = W.H
    for i, name in enumerate(("Q", "K", "V")):
        r = float(((cur[name] - y[:, i * H:(i + 1) * H]).abs() / bound[:, i * H:(i + 1) * H]).max())
        print("%s B %s ratio %.3f" % (tag, name, r))
        margin("mfma16/%s/B_%s_ratio" % (tag, name), r, 1.0)
    (hm64, x64, _), (hm32, x32, _) = ES.memo(("D", id(W), l), [cur["ctx"], x], lambda: (
        ES.tail_chain(W, l, cur["ctx"], x), ES.tail_chain(W, l, cur["ctx"], x, acc=F32)))
    for name, g, r64, r32 in (("Hm", cur["Hm"], hm64, hm32), ("X", cur["X"], x64, x32)):
        c_ref, f_ref = ES.tail_metrics(r32, r64)
        c_bar, f_cap = ES.tail_bars(c_ref, f_ref)
        c, f = ES.tail_metrics(g, r64)
        print("%s D %s: c %.3g (floor %.3g, bar %.3g)  f %.3g%% (floor %.3g%%, cap %.3g%%)" % (tag, name, c, c_ref, c_bar, 100 * f,
                                                                                              100 * f_ref, 100 * f_cap))
        margin("mfma16/%s/D_%s_c" % (tag, name), c, c_bar)
        margin("mfma16/%s/D_%s_f" % (tag, name), f, f_cap)


@pytest.mark.parametrize("l", [0, 1, 2])
def test_single_tile_walk(l):
    """Input S, layers 0-2, every live token.  Layer 0 is the embedding (no GEMM): only its layout is checked."""
    cur = run("S", l)
    lo = cur["layout"]
    assert lo["qk"] and lo["ctx"] and not lo["hm"] and not lo["y_live"]
    if l == 0:
        return
    lens = [int(n) for n in inputs("S")[1]]
    check_stages("S/m1/l%d" % l, l, run("S", l - 1), cur, lens)


def test_persistent_walk():
    """Input P, one layer: 279 QKV tiles and 372 blocked FFN1 tiles on 256 workgroups, up to two tiles per workgroup."""
    cur = run("P", 1)
    lo = cur["layout"]
    assert lo["qk"] and lo["ctx"] and lo["hm"] and not lo["y_live"]
    lens = [int(n) for n in inputs("P")[1]]
    check_stages("P/m1/l1", 1, run("P", 0), cur, lens)


def test_stale_memory():
    """The persistent case twice, each on a workspace and an output pre-filled with 0xFF bytes (every bf16 / fp32 a NaN; the
    second run's buffers come out of the allocator holding the first run's results until that fill): identical bytes, and
    run_layers itself refuses a live row that is not finite -- no element left unwritten, nothing read before it is written."""
    a = run("P", 1)
    b = run("P", 1, fresh=True)
    for k in ("X_bits", "Q", "K", "V", "ctx", "Hm", "out"):
        assert torch.equal(a[k], b[k]), k


def test_switch():
    """The switch between this main loop and the 32x32x16 one is gone: its name is an unknown option."""
    from convdr_amd import _lib
    assert _lib.lib().convdr_set_option(b"mfma16", 1) != 0
