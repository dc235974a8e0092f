"""No result may depend on memory the call did not write itself.

Every hot entry point works inside a caller-owned scratch buffer that the hosts allocate once with torch.empty and reuse for
every later call, at offsets that move with `rows` and `B`: in production every call after the first sees, wherever it does
not write, the previous call's data at other offsets and of another type.  The forward is bitwise deterministic, the
backward is with "embed_bwd_deterministic", the search is bit-exact -- so "same inputs, other garbage in the scratch memory
-> identical bits out" needs no tolerance.  Each case runs with the scratch pre-filled with zeros (Z, the baseline, which
also has to meet the existing parity bar against the CPU oracle: "all fills equally wrong" cannot pass), bytes 0xFF (N: NaN
in every float format, -1 as an integer), seeded random bytes (R) and what a call of another shape left behind (S), and
proves that the buffer it filled is the one the call used (tests/helpers.py: assert_fills_agree).

Index buffers that live in scratch memory (a poisoned index is a wild address, so these were read before any poisoned run):

  buffer                    written by (same call, before any read)                       read by
  ------------------------  ------------------------------------------------------------  ---------------------------------------
  status (offset 0)         hipMemsetAsync(256 B) at the head of both forwards            k_seq_pack (atomicOr), host copy
  tok_id / tok_pos          k_seq_pack: rows [cu[b], cu[b] + len) from the ids, the        k_embed_ln, k_embed_bwd,
    [rows + 128]            alignment rows [cu[b] + len, cu[b + 1]) get -1 / 0; cu[B] ==   k_embed_scatter_det -- all of them
                            rows, so every row of [0, rows) is written                     only for row < rows
  order [B]                 k_len_order: the ranks are a permutation of [0, B)            k_attention_train_fwd, the attention
                            (ties broken by index), every entry written                    backward kernels: order[blockIdx] < B
  Mbits (dropout keep       k_attention_train_fwd for q < len                             k_attention_bwd_fused: bit masks, never
    words)                                                                                an address
  counts [nq_pad * stride]  k_rows_to_half (query preparation) zeroes all of them          scan (atomicAdd), k_ip_cut / k_ip_finish:
                                                                                          clamped to cap before any use as a length
  cand_id / cand_s          scan: every reserved slot < cap is stored (padding queries    k_ip_cut / k_ip_finish read [0, min(count,
    [nq, cap]               q >= nq run with tau = +inf and reserve nothing)              cap)) only; ids index P after that
  band m / counts_packed    k_ip_cut / k_ip_finish, thread 0 of query q                   k_ip_rescore / k_ip_select, debug getters
  tau [nq_pad]              k_tau_select, k_fill_f32 or the copy of tau_in: [0, nq)        scan for q < nq (else +inf), cut / finish

cu_seqlens, seq_lens, token ids and `pos` of the in-batch loss are inputs, not scratch.  The rows of the resident passage
block past n (FlatIPIndex.reserve) are data, not indices: the scan masks their scores to -inf.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import encoder as OE
from oracle import search as OS
from tests.golden.make_golden import synth_corpus
from tests.helpers import FILLS, assert_fills_agree, fill_bytes, margin
from tests.test_encoder_gpu import _check
from tests.test_train_gpu import _batch, _compare, _tiny, _tiny_dropout, _tiny_long

pytestmark = pytest.mark.gpu

GUARD = 64 << 10          # bytes of guard band on each side of a red-zoned buffer
GUARD_BYTE = 0xA5
SENTINEL_BYTE = 0x7F      # integer outputs: 0x7F7F... is no valid id / status (and is not the -1 padding)


# ------------------------------------------------------------------------------------------------------------------
# shared machinery
# ------------------------------------------------------------------------------------------------------------------
def _options(**kw):
    """convdr_set_option values for the duration of a `with`; the defaults come back in every case."""
    from contextlib import contextmanager
    from convdr_amd import _lib
    from convdr_amd.model import models as MM
    defaults = {"ffn2_splitk": 1, "fused_ln_min_rows": 128 * 192, "fused_ln_max_k": 1 << 30, "hm_blocked": 1,
                "attn_bwd_fused": 1, "embed_bwd_deterministic": 0, "gemm_tile_policy": 0, "gelu_gp": 1}
    kw = dict(kw)

    @contextmanager
    def cm():
        L = _lib.lib()
        kslice = kw.pop("KSLICE_MIN_ROWS", None)
        try:
            for k, v in kw.items():
                assert k in defaults, k
                _lib.check(L.convdr_set_option(k.encode(), v), "convdr_set_option")
            if kslice is not None:
                MM.KSLICE_MIN_ROWS = kslice
            yield
        finally:
            MM.KSLICE_MIN_ROWS = 24576
            for k in kw:
                L.convdr_set_option(k.encode(), defaults[k])
    return cm()


def _ids_mask(rs, lens, L, vocab):
    return _batch(rs, len(lens), L, lens, vocab=vocab)


def _packed_rows(lens):
    cu = np.zeros(len(lens) + 1, np.int64)
    np.cumsum((np.asarray(lens) + 7) // 8 * 8, out=cu[1:])
    return cu


def _assert_edges(lens, *, not32=True):
    """The conditions the inference cases rely on: the last sequence is shorter than any key tile, so its last key tile
    reaches past `rows`; the packed row count is ragged against the 32-row blocks and the 128-row tiles, B against 4 and 128."""
    cu = _packed_rows(lens)
    rows, B = int(cu[-1]), len(lens)
    assert lens[-1] in (1, 17) and rows - cu[-2] < 64
    assert B % 4 != 0 and B % 128 != 0
    if not32:
        assert rows % 32 != 0 and rows % 128 != 0
    return rows


EDGE17 = [128, 1, 7, 8, 9, 63, 64, 65, 127, 128, 100, 33, 17]      # 792 rows
EDGE1 = [128, 65, 9, 127, 64, 7, 1]                                 # 424 rows
SINGLE = [1]                                                        # 8 rows
_assert_edges(EDGE17)
_assert_edges(EDGE1)
assert _packed_rows(SINGLE)[-1] == 8


def _big_lens(seed=5, B=45, Lmax=128, last=17):
    rs = np.random.RandomState(seed)
    lens = rs.randint(40, Lmax + 1, size=B)
    lens[:3] = (128, 41, 127)
    lens[B - 2] = 128
    lens[-1] = last
    while _packed_rows(lens)[-1] % 32 == 0 or _packed_rows(lens)[-1] < 3842:
        lens[3] = lens[3] + 8 if lens[3] <= 112 else 48
    return [int(x) for x in lens]


BIG = _big_lens()
BIG2 = _big_lens(seed=9, B=47, last=1)
for _l in (BIG, BIG2):
    _r = _assert_edges(_l, not32=False)
    assert _r >= 3842 and _r % 256 != 0 and _r % 32 != 0       # enough rows for 256-row tiles, with a ragged last one


def _rb768(layers=2, seed=0, use_mean=False):
    from convdr_amd.model.models import MSMarcoConfigDict, RobertaConfig
    torch.manual_seed(seed)
    kw = {"model_argobj": SimpleNamespace(use_mean=True)} if use_mean else {}
    model = MSMarcoConfigDict["rdot_nll"].model_class(RobertaConfig(vocab_size=1000, num_hidden_layers=layers), **kw)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.02)
            elif "LayerNorm.weight" in n or n == "norm.weight":
                p.add_(torch.randn_like(p) * 0.05)
    return model


def _dpr_tiny(seed=4):
    from convdr_amd.model.models import MSMarcoConfigDict, BertConfig
    torch.manual_seed(seed)
    cfg = BertConfig(vocab_size=200, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=64, type_vocab_size=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = MSMarcoConfigDict["dpr"].model_class(type("A", (), {"bert_config": cfg})())
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.05)
            elif "LayerNorm.weight" in n:
                p.add_(torch.randn_like(p) * 0.1)
            elif p.dim() == 2:
                p.normal_(0, 0.05)
    return model


def _sd(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def _inference_towers(model):
    return [m for m in model.modules() if getattr(m, "_ws", None) is not None]


def _ws_ptrs(towers):
    return tuple(t._ws.data_ptr() for t in towers)


def _fill_inference(towers, kind, seed=0):
    for i, t in enumerate(towers):
        fill_bytes(t._ws, kind, seed + i)
    return _ws_ptrs(towers)


def _forward_under_fills(call, model, what, stale=(), fills=FILLS):
    """call() -> embeddings through the product surface.  `stale`: calls of other shapes (most rows first) whose leftovers
    are fill S.  The warm-up runs the largest shape first, so the host allocates once and every later call reuses it."""
    with torch.no_grad():
        for s in stale:
            s()
        call()
        towers = _inference_towers(model)
        assert towers, what
        runs = {}
        for i, f in enumerate(fills):
            filled = _fill_inference(towers, f, seed=11 + i)
            runs[f] = ({"emb": call().clone()}, filled, _ws_ptrs(towers))
        if stale:
            filled = _ws_ptrs(towers)
            for s in stale:
                s()
            runs["S"] = ({"emb": call().clone()}, filled, _ws_ptrs(towers))
    assert_fills_agree(runs, what)
    return runs["Z"][0]["emb"]


_ORACLE = {}


def _oracle_emb(key, fn):
    if key not in _ORACLE:
        with torch.no_grad():
            _ORACLE[key] = fn().numpy()
    return _ORACLE[key]


# ------------------------------------------------------------------------------------------------------------------
# A. inference forward
# ------------------------------------------------------------------------------------------------------------------
FUSED = {"fused_ln_min_rows": 1, "fused_ln_max_k": 1 << 20}
PATHS = {
    "default": {},                                                       # GEMM + LayerNorm, split-K FFN2 with its slabs
    "whole_k_ffn2": {"ffn2_splitk": 0},
    "fused_ln": dict(FUSED),                                             # row-major weights, blocked hand-off where it applies
    "fused_ln_kslice": dict(FUSED, KSLICE_MIN_ROWS=1),
    "fused_ln_rowmajor_handoff": dict(FUSED, hm_blocked=0),
    "fused_ln_kslice_rowmajor_handoff": dict(FUSED, KSLICE_MIN_ROWS=1, hm_blocked=0),
}
BATCHES = {"edge17": EDGE17, "edge1": EDGE1, "single": SINGLE, "big": BIG}


def _rb_batch(name):
    lens = BATCHES[name]
    return _ids_mask(np.random.RandomState(len(lens)), lens, 128, 1000)


@pytest.mark.parametrize("batch", ["edge17", "edge1", "single", "big"])
@pytest.mark.parametrize("path", list(PATHS))
def test_inference_forward_paths(path, batch):
    """roberta-base width (768 / 12 heads / 3072, 2 layers, CLS tail): every GEMM + LayerNorm route of the inference forward."""
    model = _rb768()
    sd = _sd(model)
    ids, mask = _rb_batch(batch)
    ref = _oracle_emb(("rb768", batch), lambda: OE.rdot_nll_emb(sd, ids, mask, num_layers=2, num_heads=12))
    model = model.cuda().eval()
    ids_d, mask_d = ids.cuda(), mask.cuda()
    more = [x.cuda() for x in _rb_batch("big" if batch != "big" else "edge17")]
    fewer = [x.cuda() for x in _rb_batch("single" if batch != "single" else "edge1")]
    if batch == "big":          # (more rows than `big`: the same batch twice)
        more = [torch.cat([ids_d, ids_d]), torch.cat([mask_d, mask_d])]
    stale = [lambda: model.body_emb(*more), lambda: model.body_emb(*fewer)]
    with _options(**PATHS[path]):
        emb = _forward_under_fills(lambda: model.body_emb(ids_d, mask_d), model, "A/%s/%s" % (path, batch), stale=stale)
        if "KSLICE_MIN_ROWS" in PATHS[path]:
            assert model.roberta.packed((model.embeddingHead, model.norm))[1].layers[0].w2_ks
        q = _forward_under_fills(lambda: model.query_emb(ids_d, mask_d), model, "A/%s/%s/query" % (path, batch), fills=("Z", "N"))
    _check(emb, ref, "A/%s/%s" % (path, batch))
    assert torch.equal(q, emb)


@pytest.mark.parametrize("path", ["default", "fused_ln"])
@pytest.mark.parametrize("batch", ["edge17", "edge1", "single"])
def test_inference_forward_use_mean(batch, path):
    """use_mean = True: the whole last layer is live and k_masked_mean pools it."""
    model = _rb768(seed=1, use_mean=True)
    sd = _sd(model)
    ids, mask = _rb_batch(batch)
    ref = _oracle_emb(("rb768_mean", batch), lambda: OE.rdot_nll_emb(sd, ids, mask, num_layers=2, num_heads=12, use_mean=True))
    model = model.cuda().eval()
    ids_d, mask_d = ids.cuda(), mask.cuda()
    more = [x.cuda() for x in _rb_batch("big")]
    fewer = [x.cuda() for x in _rb_batch("single" if batch != "single" else "edge1")]
    stale = [lambda: model.body_emb(*more), lambda: model.body_emb(*fewer)]
    with _options(**PATHS[path]):
        emb = _forward_under_fills(lambda: model.body_emb(ids_d, mask_d), model, "A/use_mean/%s/%s" % (path, batch), stale=stale)
    _check(emb, ref, "A/use_mean/%s/%s" % (path, batch))


@pytest.mark.parametrize("lens", [EDGE17, EDGE1, SINGLE], ids=["edge17", "edge1", "single"])
def test_inference_forward_tiny_128_wide(lens):
    model = _tiny()
    sd = _sd(model)
    rs = np.random.RandomState(len(lens))
    ids, mask = _ids_mask(rs, lens, 128, 200)
    with torch.no_grad():
        ref = OE.rdot_nll_emb(sd, ids, mask, num_layers=2, num_heads=2).numpy()
    model = model.cuda().eval()
    ids_d, mask_d = ids.cuda(), mask.cuda()
    more = [x.cuda() for x in _ids_mask(rs, BIG, 128, 200)]
    fewer = [x.cuda() for x in _ids_mask(rs, [9, 1], 128, 200)]
    stale = [lambda: model.body_emb(*more), lambda: model.body_emb(*fewer)]
    emb = _forward_under_fills(lambda: model.body_emb(ids_d, mask_d), model, "A/tiny/%d" % len(lens), stale=stale)
    _check(emb, ref, "A/tiny/%d" % len(lens))


def test_inference_forward_dpr_towers():
    """BERT position ids, raw CLS output (out_dim = 0), both towers."""
    lens = [64, 1, 7, 8, 9, 63, 33, 40, 17]
    _assert_edges(lens)
    model = _dpr_tiny()
    sd = _sd(model)
    rs = np.random.RandomState(9)
    ids, mask = _ids_mask(rs, lens, 64, 200)
    more = [x.cuda() for x in _ids_mask(rs, [64] * 30 + [33, 1], 64, 200)]
    fewer = [x.cuda() for x in _ids_mask(rs, [5], 64, 200)]
    model = model.cuda().eval()
    ids_d, mask_d = ids.cuda(), mask.cuda()
    for name, fn, tower in (("query", model.query_emb, "question_model"), ("body", model.body_emb, "ctx_model")):
        with torch.no_grad():
            ref = OE.dpr_emb(sd, ids, mask, tower=tower, num_layers=2, num_heads=2).numpy()
        stale = [lambda: fn(*more), lambda: fn(*fewer)]
        emb = _forward_under_fills(lambda: fn(ids_d, mask_d), model, "A/dpr/" + name, stale=stale)
        _check(emb, ref, "A/dpr/" + name)


@pytest.mark.parametrize("wide", [True, False], ids=["768", "128"])
def test_inference_forward_int32_ids_without_mask(wide):
    """The token-cache path: int32 ids, attention_mask = NULL, host lengths."""
    model = _rb768() if wide else _tiny()
    vocab, heads = (1000, 12) if wide else (200, 2)
    sd = _sd(model)
    rs = np.random.RandomState(17)
    ids, mask = _ids_mask(rs, EDGE17, 128, vocab)
    more = _ids_mask(rs, BIG, 128, vocab)
    fewer = _ids_mask(rs, SINGLE, 128, vocab)
    with torch.no_grad():
        ref = OE.rdot_nll_emb(sd, ids, mask, num_layers=2, num_heads=heads).numpy()
    model = model.cuda().eval()

    def call(b, lens):
        i32 = b[0].to(torch.int32).cuda()
        return lambda: model.body_emb(i32, None, seq_lens=np.asarray(lens, np.int32))
    emb = _forward_under_fills(call((ids, mask), EDGE17), model, "A/int32/%s" % wide, stale=[call(more, BIG), call(fewer, SINGLE)])
    _check(emb, ref, "A/int32/%s" % wide)
    with torch.no_grad():
        assert torch.equal(emb, model.body_emb(ids.cuda(), mask.cuda()))


@pytest.mark.parametrize("kind", ["768", "768_fused", "128"])
def test_encode_loop_reuses_one_workspace(kind):
    """The production case itself: one tower, batches of (many rows) -> (few) -> (many, other lengths) -> (few); each result is
    the one the same batch gives on a zero-filled workspace."""
    wide = kind != "128"
    model = (_rb768() if wide else _tiny())
    vocab, heads = (1000, 12) if wide else (200, 2)
    sd = _sd(model)
    rs = np.random.RandomState(23)
    seq = [BIG2, EDGE1, BIG, SINGLE]
    assert _packed_rows(BIG2)[-1] >= _packed_rows(BIG)[-1]
    batches = [_ids_mask(rs, lens, 128, vocab) for lens in seq]
    model = model.cuda().eval()
    dev = [(i.cuda(), m.cuda()) for i, m in batches]
    with _options(**(FUSED if kind == "768_fused" else {})), torch.no_grad():
        model.body_emb(*dev[0])                       # the largest first: one allocation
        towers = _inference_towers(model)
        base = _ws_ptrs(towers)
        zero = []
        for b in dev:
            assert _fill_inference(towers, "Z") == base
            zero.append(model.body_emb(*b).clone())
        for rnd in range(2):
            for j, b in enumerate(dev):
                out = model.body_emb(*b)
                assert_fills_agree({"Z": ({"emb": zero[j]}, base, base), "S": ({"emb": out}, base, _ws_ptrs(towers))},
                                   "A/loop/%s/round%d/batch%d" % (kind, rnd, j))
    for j in (1, 3):
        with torch.no_grad():
            ref = OE.rdot_nll_emb(sd, batches[j][0], batches[j][1], num_layers=2, num_heads=heads).numpy()
        _check(zero[j], ref, "A/loop/%s/batch%d" % (kind, j))


# ------------------------------------------------------------------------------------------------------------------
# B. red zones: a workspace of exactly the planned size, outputs of exactly their size, guard bands around all of them
# ------------------------------------------------------------------------------------------------------------------
class _Banded:
    """`nbytes` bytes between two guard bands inside one allocation of the test's own."""

    def __init__(self, nbytes, dtype=torch.uint8, shape=None, prefill=0xFF):
        nbytes = int(nbytes)
        self.nbytes = nbytes
        self.whole = torch.full((2 * GUARD + (nbytes + 255) // 256 * 256,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.view = self.whole[GUARD:GUARD + nbytes]
        self.view.fill_(prefill)
        self.t = self.view.view(dtype)
        if shape is not None:
            self.t = self.t.view(shape)

    def assert_guards(self, what):
        lo, hi = self.whole[:GUARD], self.whole[GUARD + self.nbytes:]
        assert hi.numel() >= GUARD
        assert bool((lo == GUARD_BYTE).all()), "%s: bytes in front of the buffer were written" % what
        assert bool((hi == GUARD_BYTE).all()), "%s: bytes past the end of the buffer were written" % what


def _banded_like(shape, dtype, prefill=0xFF):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return _Banded(n, dtype, tuple(shape), prefill)


def _pack_lens(mask):
    lens = mask.sum(1).numpy().astype(np.int32)
    cu = np.zeros(len(lens) + 1, np.int32)
    np.cumsum((lens + 7) // 8 * 8, out=cu[1:])
    return torch.from_numpy(lens).cuda(), torch.from_numpy(cu).cuda(), int(cu[-1]), int(lens.max())


def _capi_forward(model, ids, mask, ws, out):
    from convdr_amd import _lib
    L = _lib.lib()
    tower, head = model.roberta, (model.embeddingHead, model.norm)
    lens, cu, rows, max_len = _pack_lens(mask)
    c, w, keep = tower.packed(head)
    ids_d, mask_d = ids.cuda().contiguous(), mask.cuda().contiguous()
    if ws is None:
        return L.convdr_encoder_workspace_bytes(C.byref(c), rows, ids.shape[0])
    _lib.check(L.convdr_encoder_forward(C.byref(c), C.byref(w), _lib.ptr(ids_d), 0, _lib.ptr(mask_d), ids.shape[0], ids.shape[1],
                                        _lib.ptr(cu), _lib.ptr(lens), rows, max_len, _lib.ptr(ws), ws.numel(), _lib.ptr(out),
                                        _lib.stream_ptr()), "convdr_encoder_forward")
    torch.cuda.synchronize()


@pytest.mark.parametrize("wide,lens", [(False, EDGE17), (True, EDGE1), (True, SINGLE), (True, BIG)],
                         ids=["128-edge17", "768-edge1", "768-single", "768-big"])
def test_red_zone_inference_forward(wide, lens):
    model = (_rb768() if wide else _tiny()).cuda().eval()
    ids, mask = _ids_mask(np.random.RandomState(3), lens, 128, 1000 if wide else 200)
    need = _capi_forward(model, ids, mask, None, None)
    outs = {}
    for f in FILLS:
        ws = _Banded(need)
        fill_bytes(ws.view, f, seed=5)
        out = _banded_like((len(lens), 768), torch.float32)
        _capi_forward(model, ids, mask, ws.view, out.t)
        ws.assert_guards("B/forward workspace (fill %s)" % f)
        out.assert_guards("B/forward out (fill %s)" % f)
        assert bool(torch.isfinite(out.t).all()), "an output element was not written"
        outs[f] = ({"emb": out.t.clone()}, ws.view.data_ptr(), ws.view.data_ptr())
    assert_fills_agree(outs, "B/forward")
    with torch.no_grad():
        assert torch.equal(outs["Z"][0]["emb"], model.body_emb(ids.cuda(), mask.cuda()))      # the surface runs the same kernels


def _grad_struct(tower, head, flat):
    """convdr_encoder_grads over the flat arena `flat` (parameter order of train.py:_tower_params)."""
    from convdr_amd import _lib, train as TR
    params = TR._tower_params(tower, head)
    sizes = [p.numel() for p in params]
    assert flat.numel() == sum(sizes)
    ptr = [v.data_ptr() for v in flat.split_with_sizes(sizes)]
    nl = len(tower.encoder.layer)
    lg = (_lib.LayerGrads * nl)()
    for i in range(nl):
        b, g = 5 + 16 * i, lg[i]
        g.wqkv, g.bqkv = ptr[b], ptr[b + 3]
        g.wo, g.bo, g.ln1_g, g.ln1_b = ptr[b + 6], ptr[b + 7], ptr[b + 8], ptr[b + 9]
        g.w1, g.b1, g.w2, g.b2 = ptr[b + 10], ptr[b + 11], ptr[b + 12], ptr[b + 13]
        g.ln2_g, g.ln2_b = ptr[b + 14], ptr[b + 15]
    gr = _lib.EncoderGrads()
    gr.word_emb, gr.pos_emb, gr.type_emb, gr.emb_ln_g, gr.emb_ln_b = ptr[:5]
    gr.layers = C.cast(lg, C.POINTER(_lib.LayerGrads))
    b = 5 + 16 * nl
    gr.head_w, gr.head_b, gr.head_ln_g, gr.head_ln_b = ptr[b], ptr[b + 1], ptr[b + 2], ptr[b + 3]
    return gr, lg, params, sizes


def _capi_train(model, ids, mask, G, ws, out, flat, fresh):
    """convdr_encoder_train_forward + convdr_encoder_backward(_fresh) through the C ABI, the way train.py:_EncoderFn drives
    them.  ws None: the planned workspace size."""
    from convdr_amd import _lib, train as TR
    L = _lib.lib()
    tower, head = model.roberta, (model.embeddingHead, model.norm)
    lens, cu, rows, max_len = _pack_lens(mask)
    B = ids.shape[0]
    c, w, keep = tower.packed(head)
    if ws is None:
        return L.convdr_encoder_train_workspace_bytes(C.byref(c), rows, B)
    ids_d, mask_d, G_d = ids.cuda().contiguous(), mask.cuda().contiguous(), G.cuda().contiguous()
    wt, head_t = TR._packed_t(tower, head)
    _lib.check(L.convdr_encoder_train_forward(C.byref(c), C.byref(w), _lib.ptr(ids_d), 0, _lib.ptr(mask_d), B, ids.shape[1],
                                              _lib.ptr(cu), _lib.ptr(lens), rows, max_len, _lib.ptr(ws), ws.numel(), _lib.ptr(out),
                                              None, _lib.stream_ptr()), "convdr_encoder_train_forward")
    gr, lg, params, sizes = _grad_struct(tower, head, flat)
    fn = L.convdr_encoder_backward_fresh if fresh else L.convdr_encoder_backward
    _lib.check(fn(C.byref(c), C.byref(w), wt, _lib.ptr(cu), _lib.ptr(lens), C.c_void_p(head_t) if head_t else None, B, rows,
                  max_len, _lib.ptr(ws), ws.numel(), _lib.ptr(G_d), C.byref(gr), None, _lib.stream_ptr()),
               "convdr_encoder_backward")
    torch.cuda.synchronize()
    return params, sizes


def _named_grads(model, params, sizes, flat):
    names = {id(p): n for n, p in model.named_parameters()}
    return {names[id(p)]: v.clone().view(p.shape) for p, v in zip(params, flat.split_with_sizes(sizes))}


def _oracle_check_grads(sd_cpu, ids, mask, G, emb, grads, layers, heads, cos_tol, norm_tol, tag, **okw):
    """The parity bar of the existing test of this shape, applied to the zero-filled run."""
    sd = {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point) for k, v in sd_cpu.items()}
    ref_emb = OE.rdot_nll_emb(sd, ids, mask, num_layers=layers, num_heads=heads, **okw)
    (ref_emb * G).sum().backward()
    _check(emb, ref_emb.detach().numpy(), tag)
    seen = 0
    for n, g in grads.items():
        r = sd[n].grad if n in sd else None
        if r is None or n.endswith("attention.self.key.bias") or float(r.abs().max()) == 0:
            continue
        _compare(n, g, r, cos_tol=cos_tol, norm_tol=norm_tol)
        seen += 1
    assert seen >= 20, seen


@pytest.mark.parametrize("fresh", [True, False], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("B,L,lens", [(5, 40, [40, 17, 33, 1, 8]), (3, 130, [130, 64, 65])])
def test_red_zone_training_forward_backward(B, L, lens, fresh):
    """Also the accumulating against the storing backward: workspace poisoned, the gradient arena is an input of the former
    (zeroed) and an output of the latter (NaN except the embedding prefix the host zeroes)."""
    from convdr_amd import train as TR
    model = _tiny()
    sd_cpu = _sd(model)
    rs = np.random.RandomState(1)
    ids, mask = _batch(rs, B, L, lens)
    G = torch.from_numpy(rs.randn(B, 768).astype(np.float32))
    model = model.cuda().train()
    need = _capi_train(model, ids, mask, G, None, None, None, fresh)
    all_params = TR._tower_params(model.roberta, (model.embeddingHead, model.norm))
    total, prefix = sum(p.numel() for p in all_params), sum(p.numel() for p in all_params[:5])
    runs = {}
    with _options(embed_bwd_deterministic=1):
        for f in FILLS:
            ws = _Banded(need)
            fill_bytes(ws.view, f, seed=7)
            out = _banded_like((B, 768), torch.float32)
            arena = _banded_like((total,), torch.float32)
            if fresh:
                arena.t[:prefix].zero_()          # what the host zeroes; every other gradient must be STORED
            else:
                arena.t.zero_()
            params, sizes = _capi_train(model, ids, mask, G, ws.view, out.t, arena.t, fresh)
            for b, n in ((ws, "workspace"), (out, "out"), (arena, "gradient arena")):
                b.assert_guards("B/train %s (fill %s)" % (n, f))
            assert bool(torch.isfinite(out.t).all()) and bool(torch.isfinite(arena.t).all()), "an output element was not written"
            o = _named_grads(model, params, sizes, arena.t)
            o["emb"] = out.t.clone()
            runs[f] = (o, ws.view.data_ptr(), ws.view.data_ptr())
    assert_fills_agree(runs, "B/train")
    z = dict(runs["Z"][0])
    emb = z.pop("emb")
    _oracle_check_grads(sd_cpu, ids, mask, G, emb, z, 2, 2, 1 - 2e-4, 6e-3, "B/train")


def _search_raw(idx, q, k, ws, D, I, status, tau_retry, x3):
    cap = idx.cap
    while cap < 2 * k and cap < 8192:
        cap *= 2
    n = idx.ntotal
    plo = idx._plo if x3 else None
    idx._search_call(q, int(q.shape[0]), idx._p32, idx._pbf, plo, n, k, None, cap, idx.rank_target, ws, D, I, status, tau_retry)
    torch.cuda.synchronize()
    return cap


@pytest.mark.parametrize("precision,n,nq,k", [("bf16", 5003, 9, 100), ("fp16", 37, 3, 100), ("bf16x3", 40007, 129, 7),
                                              ("fp16x3", 700, 1, 1)])
def test_red_zone_search(precision, n, nq, k):
    from convdr_amd import _lib
    from convdr_amd.search import FlatIPIndex
    P, Q = synth_corpus(300 + n % 97, n, 768), synth_corpus(13, nq, 768)
    Dr, Ir = OS.flat_ip_search(Q, P, k)
    idx = FlatIPIndex(768, precision=precision)
    idx.add(P)
    x3 = precision.endswith("x3")
    q = torch.from_numpy(Q).cuda()
    cap = idx.cap
    while cap < 2 * k and cap < 8192:
        cap *= 2
    need = _lib.lib().convdr_ip_workspace_bytes(nq, n, 768, k, cap)
    sent64 = int.from_bytes(bytes([SENTINEL_BYTE] * 8), "little")
    runs = {}
    for f in FILLS:
        ws = _Banded(need)
        fill_bytes(ws.view, f, seed=9)
        D = _banded_like((nq, k), torch.float32)
        I = _banded_like((nq, k), torch.int64, prefill=SENTINEL_BYTE)
        st = _banded_like((nq,), torch.int32, prefill=SENTINEL_BYTE)
        tr = _banded_like((nq,), torch.float32)
        _search_raw(idx, q, k, ws.view, D.t, I.t, st.t, tr.t, x3)
        for b, name in ((ws, "workspace"), (D, "D"), (I, "I"), (st, "status"), (tr, "tau_retry")):
            b.assert_guards("B/search %s (fill %s)" % (name, f))
        assert not bool(torch.isnan(D.t).any()) and not bool(torch.isnan(tr.t).any()), "an output element was not written"
        assert not bool((I.t == sent64).any()) and not bool((st.t == (sent64 & 0xffffffff)).any()), "an output element was not written"
        # (tau_retry is -inf where nothing is to retry: compared bitwise, not for finiteness)
        runs[f] = ({"D": D.t.clone(), "I": I.t.clone(), "status": st.t.clone(), "tau_retry": tr.t.clone().view(torch.int32)},
                   ws.view.data_ptr(), ws.view.data_ptr())
    assert_fills_agree(runs, "B/search")
    z = runs["Z"][0]
    _certified_rows_match(z, Dr, Ir, "B/search")                          # a certified query is exact
    if n < k:
        assert bool((z["I"][:, n:] == -1).all()) and bool((z["D"][:, n:] == -3.4028234663852886e38).all())


# ------------------------------------------------------------------------------------------------------------------
# C. training forward + backward through the model surface
# ------------------------------------------------------------------------------------------------------------------
def _train_towers(model):
    return [m for m in model.modules() if m.__dict__.get("_train_ws_pool")]


def _pool_ptrs(towers):
    return tuple(e.ws.data_ptr() for t in towers for e in t._train_ws_pool)


def _fill_pools(towers, kind, seed=0):
    torch.cuda.synchronize()          # (the weight-gradient streams of the previous backward are done with the buffer)
    for t in towers:
        for e in t._train_ws_pool:
            fill_bytes(e.ws, kind, seed)
    torch.cuda.synchronize()
    return _pool_ptrs(towers)


def _step(model, fwd_bwd):
    model.zero_grad(set_to_none=True)
    model.__dict__["_dropout_calls"] = 0             # the same masks every run
    out = fwd_bwd()
    o = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    o.update(out)
    return o


def _train_under_fills(model, fwd_bwd, what, stale=(), n_ws=1, fills=FILLS):
    """fwd_bwd() runs forward(s) + backward and returns {name: embedding tensor}.  The fills go in BEFORE the forward: the
    backward reads what the forward saved.  `stale`: steps of other shapes, most rows first (their leftovers are fill S)."""
    with _options(embed_bwd_deterministic=1):
        for s in stale:
            _step(model, s)
        _step(model, fwd_bwd)
        towers = _train_towers(model)
        assert towers and len(_pool_ptrs(towers)) == n_ws, (what, _pool_ptrs(towers))
        runs = {}
        for i, f in enumerate(fills):
            filled = _fill_pools(towers, f, seed=31 + i)
            runs[f] = (_step(model, fwd_bwd), filled, _pool_ptrs(towers))
        if stale:
            filled = _pool_ptrs(towers)
            for s in stale:
                _step(model, s)
            runs["S"] = (_step(model, fwd_bwd), filled, _pool_ptrs(towers))
    assert_fills_agree(runs, what)
    assert len(runs["Z"][0]) > 20
    z = dict(runs["Z"][0])
    return z.pop("emb"), z


def _fb(model, ids, mask, G):
    ids_d, mask_d, G_d = ids.cuda(), mask.cuda(), G.cuda()

    def run():
        emb = model(ids_d, mask_d)
        (emb * G_d).sum().backward()
        return {"emb": emb.detach().clone()}
    return run


def _randn(rs, *shape):
    return torch.from_numpy(rs.randn(*shape).astype(np.float32))


@pytest.mark.parametrize("p_h,p_a", [(0.0, 0.0), (0.1, 0.1), (0.0, 0.3)])
def test_training_tiny_ragged_with_dropout(p_h, p_a):
    """Ragged and odd lengths, a 1-token sequence last; the dropout keep-bit words are stale for q in [len, plen)."""
    from convdr_amd import train as TR
    rs = np.random.RandomState(41)
    lens = [130, 64, 65, 7, 33, 15, 1]
    B, L = len(lens), 130
    model = _tiny_dropout(p_h, p_a)
    model.dropout_seed = 1234
    sd_cpu = _sd(model)
    ids, mask = _batch(rs, B, L, lens)
    G = _randn(rs, B, 768)
    more = _batch(rs, 9, 130, [130, 128, 127, 129, 65, 100, 99, 3, 77])
    fewer = _batch(rs, 2, 16, [9, 1])
    Gm, Gf = _randn(rs, 9, 768), _randn(rs, 2, 768)
    seed = TR.dropout_seed_of(model, 0)
    model = model.cuda().train()
    emb, grads = _train_under_fills(model, _fb(model, ids, mask, G), "C/tiny/%g_%g" % (p_h, p_a),
                                    stale=[_fb(model, *more, Gm), _fb(model, *fewer, Gf)])
    drop = {"dropout": (p_h, p_a, seed)} if (p_h or p_a) else {}
    cos_tol, norm_tol = (1 - 3e-4, 0.01) if drop else (1 - 2e-4, 6e-3)      # test_dropout_forward_backward... / test_encoder_backward...
    _oracle_check_grads(sd_cpu, ids, mask, G, emb, grads, 2, 2, cos_tol, norm_tol, "C/tiny", **drop)


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("L,lens", [(320, [320, 257, 40, 256, 300]),
                                    (256, [33, 256, 1, 191, 64, 129, 255, 31, 192, 65, 128, 193, 63, 32, 127, 200])],
                         ids=["past256", "upto256"])
def test_training_long_sequences_both_attention_backward_forms(L, lens, fused):
    rs = np.random.RandomState(77)
    B = len(lens)
    model = _tiny_long()
    sd_cpu = _sd(model)
    ids, mask = _batch(rs, B, L, lens)
    G = _randn(rs, B, 768)
    more = _batch(rs, B + 3, 320, [320] * (B + 2) + [1])
    fewer = _batch(rs, 3, 40, [40, 9, 1])
    Gm, Gf = _randn(rs, B + 3, 768), _randn(rs, 3, 768)
    model = model.cuda().train()
    with _options(attn_bwd_fused=fused):
        emb, grads = _train_under_fills(model, _fb(model, ids, mask, G), "C/long/L%d/fused%d" % (L, fused),
                                        stale=[_fb(model, *more, Gm), _fb(model, *fewer, Gf)])
    _oracle_check_grads(sd_cpu, ids, mask, G, emb, grads, 3, 2, 1 - 4e-4, 8e-3, "C/long")      # test_attention_backward_one_workgroup_form...


def test_training_use_mean_pooling():
    """use_mean = True: the whole last layer is live in the forward and the backward (k_masked_mean_bwd)."""
    from convdr_amd.model.models import MSMarcoConfigDict, RobertaConfig
    torch.manual_seed(6)
    cfg = RobertaConfig(vocab_size=200, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                        max_position_embeddings=140, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = MSMarcoConfigDict["rdot_nll"].model_class(cfg, model_argobj=SimpleNamespace(use_mean=True))
    sd_cpu = _sd(model)
    rs = np.random.RandomState(6)
    lens = [40, 17, 33, 8, 9, 1]
    ids, mask = _batch(rs, 6, 40, lens)
    G = _randn(rs, 6, 768)
    more, fewer = _batch(rs, 9, 130, [130] * 8 + [1]), _batch(rs, 1, 8, [1])
    Gm, Gf = _randn(rs, 9, 768), _randn(rs, 1, 768)
    model = model.cuda().train()
    emb, grads = _train_under_fills(model, _fb(model, ids, mask, G), "C/use_mean", stale=[_fb(model, *more, Gm), _fb(model, *fewer, Gf)])
    # the bar of test_use_mean_pooling_matches_reference_fixture: worst gradient cosine > 1 - 1e-3
    sd = {k: v.clone().requires_grad_(v.dtype.is_floating_point) for k, v in sd_cpu.items()}
    ref = OE.rdot_nll_emb(sd, ids, mask, num_layers=2, num_heads=2, use_mean=True)
    (ref * G).sum().backward()
    _check(emb, ref.detach().numpy(), "C/use_mean")
    worst = 1.0
    for n, g in grads.items():
        r = sd[n].grad if n in sd else None
        if r is None or n.endswith("attention.self.key.bias") or r.norm() < 1e-9:
            continue
        g, r = g.cpu().double().reshape(-1), r.double().reshape(-1)
        worst = min(worst, float((g @ r) / (g.norm() * r.norm())))
    assert worst > 1 - 1e-3, worst


def test_training_dpr_tower():
    model = _dpr_tiny(seed=11)
    sd_cpu = _sd(model)
    rs = np.random.RandomState(11)
    lens = [40, 9, 23, 2, 1]
    ids, mask = _batch(rs, 5, 40, lens)
    G = _randn(rs, 5, 128)
    more, fewer = _batch(rs, 11, 64, [64] * 10 + [1]), _batch(rs, 1, 8, [3])
    Gm, Gf = _randn(rs, 11, 128), _randn(rs, 1, 128)
    model = model.cuda().train()
    emb, grads = _train_under_fills(model, _fb(model, ids, mask, G), "C/dpr", stale=[_fb(model, *more, Gm), _fb(model, *fewer, Gf)])
    sd = {k: v.clone().requires_grad_(v.dtype.is_floating_point) for k, v in sd_cpu.items()}
    ref = OE.dpr_emb(sd, ids, mask, tower="question_model", num_layers=2, num_heads=2)
    (ref * G).sum().backward()
    _check(emb, ref.detach().numpy(), "C/dpr")
    seen = 0
    for n, g in grads.items():
        if n in sd and sd[n].grad is not None and not n.endswith("key.bias") and "pooler" not in n:
            _compare(n, g, sd[n].grad, cos_tol=1 - 2e-4, norm_tol=1e-2)         # test_dpr_tower_backward_matches_autograd
            seen += 1
    assert seen > 20


def test_training_at_256_tile_scale():
    """The shape of test_backward_at_256_tile_scale_matches_autograd (cost-model tile policy): the long-K data-gradient and
    weight-gradient engines with the slack rows live."""
    from convdr_amd.model.models import MSMarcoConfigDict, RobertaConfig
    torch.manual_seed(12)
    cfg = RobertaConfig(vocab_size=300, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072,
                        max_position_embeddings=140, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = MSMarcoConfigDict["rdot_nll"].model_class(cfg)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.05)
            elif "LayerNorm.weight" in n or n == "norm.weight":
                p.add_(torch.randn_like(p) * 0.1)
    sd_cpu = _sd(model)
    rs = np.random.RandomState(12)
    B, L = 150, 128
    lens = rs.randint(100, L + 1, size=B).tolist()
    lens[-1] = 1
    assert _packed_rows(lens)[-1] % 256 != 0
    ids, mask = _batch(rs, B, L, lens, vocab=300)
    G = _randn(rs, B, 768)
    more = _batch(rs, B + 7, L, [128] * (B + 6) + [17], vocab=300)
    fewer = _batch(rs, 3, 16, [16, 9, 1], vocab=300)
    Gm, Gf = _randn(rs, B + 7, 768), _randn(rs, 3, 768)
    model = model.cuda().train()
    emb, grads = _train_under_fills(model, _fb(model, ids, mask, G), "C/256tile", stale=[_fb(model, *more, Gm), _fb(model, *fewer, Gf)])
    _oracle_check_grads(sd_cpu, ids, mask, G, emb, grads, 2, 12, 1 - 3e-4, 2e-3, "C/256tile")


def test_training_two_forwards_one_backward_on_stale_workspaces():
    """(model(a) * Ga + model(b) * Gb).sum().backward(): two pool entries alive at once, both holding what forwards of other
    shapes left (S), against the same on zero-filled and poisoned entries."""
    rs = np.random.RandomState(11)
    model = _tiny().cuda().train()
    a = [x.cuda() for x in _batch(rs, 4, 48, [48, 20, 33, 5])]
    b = [x.cuda() for x in _batch(rs, 3, 130, [130, 64, 65])]
    Ga, Gb = _randn(rs, 4, 768).cuda(), _randn(rs, 3, 768).cuda()
    big = [x.cuda() for x in _batch(rs, 9, 130, [130] * 8 + [1])]
    small = [x.cuda() for x in _batch(rs, 2, 16, [9, 1])]
    Gbig, Gsmall = _randn(rs, 9, 768).cuda(), _randn(rs, 2, 768).cuda()

    def two(x, y, gx, gy):
        def run():
            ex, ey = model(*x), model(*y)
            ((ex * gx).sum() + (ey * gy).sum()).backward()
            return {"emb": ex.detach().clone(), "emb_b": ey.detach().clone()}
        return run

    def one(x, g):
        def run():
            e = model(*x)
            (e * g).sum().backward()
            return {"emb": e.detach().clone()}
        return run
    stale = [two(big, big, Gbig, Gbig), two(small, small, Gsmall, Gsmall)]
    emb, grads = _train_under_fills(model, two(a, b, Ga, Gb), "C/two_forwards", stale=stale, n_ws=2)
    # the bar of test_two_forwards_one_backward_keep_their_own_activations: the sum of the two separate backwards
    with _options(embed_bwd_deterministic=1):
        ga, gb = _step(model, one(a, Ga)), _step(model, one(b, Gb))
    for n, g in grads.items():
        if n == "emb_b":
            continue
        ref = ga[n] + gb[n]
        tol = 1e-4 if "embeddings" in n else 1e-6
        assert torch.allclose(g, ref, rtol=1e-4, atol=tol * (1 + ref.abs().max().item())), n
    assert torch.equal(emb, ga["emb"]) and torch.equal(grads["emb_b"], gb["emb"])


def test_whole_kd_train_step_with_poisoned_scratch():
    """Two steps of the KD flow (teacher forward, student forward + backward, MSE, clipped norm, AdamW; dropout on): every
    torch.empty the hosts make on the device -- workspace pools, the teacher's workspace, gradient arena, norm scratch, loss
    and `ds` tensors -- comes back zero-filled in one run and 0xFF-filled in the other, and the pooled workspaces are
    re-filled between the steps.  Loss, norm, clip coefficient and every updated parameter must agree bit for bit."""
    from convdr_amd import train as TR
    rs = np.random.RandomState(5)
    ids, mask = _batch(rs, 6, 48, [48, 20, 33, 5, 40, 1])
    tid, tmask = _batch(rs, 6, 16, [16, 9, 4, 16, 7, 1])
    batch = tuple(x.cuda() for x in (ids, mask, tid, tmask))
    args = SimpleNamespace(learning_rate=1e-3, adam_epsilon=1e-8, max_grad_norm=1.0, ranking_task=False, no_mse=False,
                           num_negatives=0, gradient_accumulation_steps=1)
    real_empty, real_clip = torch.empty, TR.clip_grad_norm_
    results = {}
    for f in ("Z", "N"):
        def poisoned_empty(*a, **k):
            t = real_empty(*a, **k)
            if t.is_cuda and t.numel():
                fill_bytes(t, f)
                torch.cuda.synchronize()          # (the fill is complete before any other stream touches the tensor)
            return t
        norms = []

        def recording_clip(params, max_norm, defer_to=None, **kw):
            total = real_clip(params, max_norm, defer_to=defer_to, **kw)
            norms.append(total.detach().clone())
            if defer_to is not None and getattr(defer_to, "_pending_grad_scale", None) is not None:
                norms.append(defer_to._pending_grad_scale.detach().clone())
            return total
        student, teacher = _tiny_dropout(0.1, 0.1, seed=3).cuda(), _tiny(seed=4).cuda().eval()
        student.dropout_seed = 1234
        assert TR.flatten_parameters(student) is not None
        opt = TR.get_optimizer(args, student, weight_decay=0.0)
        sched = TR.get_linear_schedule_with_warmup(opt, 0, 10)
        out, ptrs = {}, []
        torch.empty, TR.clip_grad_norm_ = poisoned_empty, recording_clip
        try:
            with _options(embed_bwd_deterministic=1):
                for step in range(2):
                    towers = _train_towers(student)
                    if towers:
                        ptrs.append(_fill_pools(towers, f) + (fill_bytes(teacher.roberta._ws, f).data_ptr(),))
                    loss = TR.train_step(args, student, teacher, opt, sched, batch)
                    out["loss%d" % step] = loss[0].detach().clone().reshape(1)
                    torch.cuda.synchronize()
                    if ptrs:
                        assert _pool_ptrs(_train_towers(student)) + (teacher.roberta._ws.data_ptr(),) == ptrs[-1]
        finally:
            torch.empty, TR.clip_grad_norm_ = real_empty, real_clip
        assert len(norms) == 4 and len(ptrs) == 1, (len(norms), len(ptrs))
        for i, t in enumerate(norms):
            out["norm_or_coef%d" % i] = t.reshape(-1)
        for k, v in student.state_dict().items():
            out["param/" + k] = v.detach().clone()
        results[f] = (out, 0, 0)
    assert_fills_agree(results, "C/train_step")
    z = results["Z"][0]
    assert float(z["loss0"]) > 0 and float(z["loss0"]) != float(z["loss1"]) and float(z["norm_or_coef0"]) > 0


# ------------------------------------------------------------------------------------------------------------------
# D. search
# ------------------------------------------------------------------------------------------------------------------
_SEARCH_ORACLE = {}


def _search_case(n, nq, k):
    key = (n, nq, k)
    if key not in _SEARCH_ORACLE:
        P, Q = synth_corpus(200 + n % 89, n, 768), synth_corpus(8 + nq, nq, 768)
        _SEARCH_ORACLE[key] = (P, Q) + tuple(OS.flat_ip_search(Q, P, k))
    return _SEARCH_ORACLE[key]


def _raw_search(idx, q, k):
    D, I, st, tr = idx.search_device(q, k)
    # (tau_retry is -inf where nothing is to retry: compared bitwise, not for finiteness; D holds -FLT_MAX padding)
    return {"D": D.clone(), "I": I.clone(), "status": st.clone(), "tau_retry": tr.clone().view(torch.int32)}


def _certified_rows_match(out, Dr, Ir, what):
    """The raw pass: a query it certifies (status 0) is exact; the others go up the host ladder (checked through search())."""
    ok = (out["status"] == 0).cpu().numpy()
    np.testing.assert_array_equal(out["I"].cpu().numpy()[ok], Ir[ok], err_msg=what)
    np.testing.assert_array_equal(out["D"].cpu().numpy()[ok], Dr[ok], err_msg=what)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3", "fp16", "fp16x3"])
@pytest.mark.parametrize("n,nq,k", [(700, 9, 100), (5003, 1, 1), (40007, 129, 100), (37, 9, 100), (9001, 9, 1000)])
def test_search_workspace_fills(precision, n, nq, k):
    """FlatIPIndex._ws under the four fills (S: a search of few queries directly after one of many, and of another k, on
    the same index); raw pass (D, I, status, tau_retry) and the certified result."""
    from convdr_amd.search import FlatIPIndex
    P, Q, Dr, Ir = _search_case(n, nq, k)
    assert n % 256 != 0 and n % 128 != 0
    idx = FlatIPIndex(768, precision=precision)
    idx.add(P)
    q = torch.from_numpy(Q).cuda()
    many = torch.from_numpy(synth_corpus(77, 140, 768)).cuda()
    idx.search_device(many, max(k, 128))            # the largest workspace first
    idx.search_device(q, k)
    ptr = idx._ws.data_ptr()
    runs = {}
    for i, f in enumerate(FILLS):
        fill_bytes(idx._ws, f, seed=41 + i)
        runs[f] = (_raw_search(idx, q, k), ptr, idx._ws.data_ptr())
    idx.search_device(many, max(k, 128))
    idx.search_device(q[:1], 1)
    runs["S"] = (_raw_search(idx, q, k), ptr, idx._ws.data_ptr())
    assert_fills_agree(runs, "D/%s/%d_%d_%d" % (precision, n, nq, k))
    _certified_rows_match(runs["Z"][0], Dr, Ir, "D/raw")
    for f in FILLS:                                   # the product surface, ladder included, on a filled workspace
        fill_bytes(idx._ws, f, seed=5)
        D, I = idx.search(Q, k)
        np.testing.assert_array_equal(I, Ir)
        np.testing.assert_array_equal(D, Dr)
    if n < k:
        assert (Ir[:, n:] == -1).all()


@pytest.mark.parametrize("precision", ["bf16", "bf16x3", "fp16", "fp16x3"])
def test_search_reserved_tail_is_never_scored(precision):
    """reserve(n_big) then add() of fewer rows: the unfilled rows of the fp32 block and of the scan copies hold whatever the
    allocator returned; the last passage tile reads them."""
    from convdr_amd.search import FlatIPIndex
    n, nq, k = 5003, 9, 100
    P, Q = synth_corpus(200 + n % 89, n, 768), synth_corpus(8 + nq, nq, 768)
    Dr, Ir = OS.flat_ip_search(Q, P, k)
    idx = FlatIPIndex(768, precision=precision)
    idx.reserve(9000)
    idx.add(torch.from_numpy(P).cuda())
    assert idx.ntotal == n and idx._s32.shape[0] == 9000 and n % 128 != 0
    q = torch.from_numpy(Q).cuda()
    idx.search_device(q, k)
    held = lambda: [t for t in (idx._s32, idx._s16, idx._slo) if t is not None]
    assert len(held()) == (3 if precision.endswith("x3") else 2)
    ptrs = tuple(t.data_ptr() for t in held())
    runs = {}
    for i, f in enumerate(FILLS):
        for t in held():
            fill_bytes(t[n:], f, seed=51 + i)
        fill_bytes(idx._ws, f, seed=61 + i)
        runs[f] = (_raw_search(idx, q, k), ptrs, tuple(t.data_ptr() for t in held()))
    assert_fills_agree(runs, "D/reserved_tail/" + precision)
    _certified_rows_match(runs["Z"][0], Dr, Ir, "D/reserved_tail")
    D, I = idx.search(Q, k)                           # (the tails still hold fill R)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)


def test_search_retry_path_on_poisoned_workspace():
    """The shape of test_retry_path_is_exact: the certificate fails, the host ladder re-runs with tau_in and a larger cap."""
    from convdr_amd.search import FlatIPIndex
    P, Q = synth_corpus(8, 20000, 768), synth_corpus(9, 12, 768)
    Dr, Ir = OS.flat_ip_search(Q, P, 100)
    idx = FlatIPIndex(768, rank_target=100, cap=1024)
    idx.add(P)
    idx.search(Q, 100)                                # the ladder grows the workspace to its largest rung
    ptr = idx._ws.data_ptr()
    for i, f in enumerate(FILLS):
        fill_bytes(idx._ws, f, seed=71 + i)
        D, I = idx.search(Q, 100)
        assert idx.stats["retried"] > 0 and idx._ws.data_ptr() == ptr
        np.testing.assert_array_equal(I, Ir)
        np.testing.assert_array_equal(D, Dr)


def test_topk_merge_leaves_the_output_pitch_padding_alone():
    from convdr_amd import _lib
    from convdr_amd.search import merge_topk_device
    rs = np.random.RandomState(3)
    for na, nb, nq in ((100, 100, 37), (7, 100, 5), (1, 1, 3)):
        def lists(n):
            d = np.sort(rs.randint(0, 40, size=(nq, n)).astype(np.float32) * 0.25, axis=1)[:, ::-1].copy()
            i = rs.randint(0, 10 ** 9, size=(nq, n)).astype(np.int64)
            return torch.from_numpy(d).cuda(), torch.from_numpy(i).cuda()
        (Da, Ia), (Db, Ib) = lists(na), lists(nb)
        n_out, ldo = na + nb, na + nb + 5
        ref = merge_topk_device((Da, Ia), (Db, Ib), max(na, nb))
        runs = {}
        for j, f in enumerate(FILLS):
            Do = fill_bytes(torch.empty((nq, ldo), dtype=torch.float32, device="cuda"), f, seed=81 + j)
            Io = fill_bytes(torch.empty((nq, ldo), dtype=torch.int64, device="cuda"), f, seed=91 + j)
            pad = (Do[:, n_out:].clone(), Io[:, n_out:].clone())
            _lib.check(_lib.lib().convdr_topk_merge(_lib.ptr(Da), _lib.ptr(Ia), na, Da.stride(0), _lib.ptr(Db), _lib.ptr(Ib), nb,
                                                    Db.stride(0), nq, n_out, _lib.ptr(Do), _lib.ptr(Io), ldo, _lib.stream_ptr()),
                       "convdr_topk_merge")
            assert torch.equal(Do[:, n_out:].contiguous().view(torch.int32), pad[0].view(torch.int32)), "padding written"
            assert torch.equal(Io[:, n_out:], pad[1]), "padding written"
            runs[f] = ({"D": Do[:, :n_out].clone(), "I": Io[:, :n_out].clone()}, Do.data_ptr(), Do.data_ptr())
        assert_fills_agree(runs, "D/merge")
        assert torch.equal(runs["Z"][0]["D"], ref[0]) and torch.equal(runs["Z"][0]["I"], ref[1])


# ------------------------------------------------------------------------------------------------------------------
# E. small kernels
# ------------------------------------------------------------------------------------------------------------------
def _both_fills(make_outputs, call, what):
    """Outputs (and scratch, names starting with "_") pre-filled with zeros / 0xFF: every output element written, results equal."""
    runs = {}
    for f in ("Z", "N"):
        outs = make_outputs()
        for t in outs.values():
            fill_bytes(t, f)
        call(outs)
        torch.cuda.synchronize()
        for n, t in outs.items():
            if not n.startswith("_"):
                assert not bool(torch.isnan(t).any()), "%s: %s has an element that was not written" % (what, n)
        runs[f] = ({n: t.clone() for n, t in outs.items() if not n.startswith("_")}, 0, 0)
    assert_fills_agree(runs, what)
    return runs["Z"][0]


@pytest.mark.parametrize("n", [100, 70001, 1 << 20])      # 1, 274 and all 1024 partial slots of convdr_grad_norm_clip
def test_grad_norm_with_poisoned_partials(n):
    from convdr_amd import _lib
    L = _lib.lib()
    g = torch.from_numpy(np.random.RandomState(n % 97).randn(n).astype(np.float32)).cuda()
    ref = float(np.sqrt((0.25 * g.cpu().double().numpy() ** 2).sum()))
    coef = 0.5 * min(1.0, 1.0 / (ref + 1e-6))
    z = _both_fills(lambda: {"_scratch": torch.empty(1024, dtype=torch.float32, device="cuda"),
                             "out": torch.empty(2, dtype=torch.float32, device="cuda")},
                    lambda o: _lib.check(L.convdr_grad_norm_clip(_lib.ptr(g), n, 1.0, 0.5, _lib.ptr(o["_scratch"]), _lib.ptr(o["out"]),
                                                                 0, _lib.stream_ptr()), "convdr_grad_norm_clip"), "E/grad_norm_clip")
    # the bars of test_adamw_and_grad_norm_on_slices_that_are_not_16_byte_aligned
    assert abs(z["out"][0].item() - ref) <= 2e-6 * ref + 1e-12
    assert abs(z["out"][1].item() - coef) <= 1e-6 * coef
    for nblocks in (1, 7, 1024):
        def call(o):
            _lib.check(L.convdr_grad_sumsq(_lib.ptr(g), n, _lib.ptr(o["partials"]), nblocks, _lib.stream_ptr()), "convdr_grad_sumsq")
            _lib.check(L.convdr_grad_norm_finish(_lib.ptr(o["partials"]), nblocks, 1.0, 0.5, _lib.ptr(o["out"]), _lib.stream_ptr()),
                       "convdr_grad_norm_finish")
        z = _both_fills(lambda: {"partials": torch.empty(nblocks, dtype=torch.float32, device="cuda"),
                                 "out": torch.empty(2, dtype=torch.float32, device="cuda")}, call, "E/grad_sumsq/%d" % nblocks)
        assert abs(z["out"][0].item() - ref) <= 2e-6 * ref + 1e-12
        assert abs(z["out"][1].item() - coef) <= 1e-6 * coef


def test_mse_with_poisoned_outputs():
    from convdr_amd import _lib
    L = _lib.lib()
    rs = np.random.RandomState(3)
    for shape in ((6, 768), (1, 4), (33, 100)):
        s, t = (torch.from_numpy(rs.randn(*shape).astype(np.float32)).cuda() for _ in range(2))
        z = _both_fills(lambda: {"loss": torch.empty((), dtype=torch.float32, device="cuda"), "ds": torch.empty_like(s)},
                        lambda o: _lib.check(L.convdr_mse_fwd_bwd(_lib.ptr(s), _lib.ptr(t), s.numel(), 1.0, _lib.ptr(o["loss"]),
                                                                  _lib.ptr(o["ds"]), _lib.stream_ptr()), "convdr_mse_fwd_bwd"), "E/mse")
        s2 = s.detach().clone().requires_grad_(True)
        ref = torch.nn.functional.mse_loss(s2, t)
        ref.backward()
        assert abs(z["loss"].item() - ref.item()) < 1e-5 * max(1, abs(ref.item()))          # test_losses_match_torch
        assert torch.allclose(z["ds"], s2.grad, rtol=1e-4, atol=1e-7)


def _rank_ce_reference(e, d, dtype):
    e = e.to(dtype).clone().requires_grad_(True)
    logits = (e.unsqueeze(1) * d.to(dtype)).sum(-1)
    per = torch.nn.functional.cross_entropy(logits, torch.zeros(e.shape[0], dtype=torch.long), reduction="none")
    per.mean().backward()
    return per.detach(), e.grad.detach(), logits.detach()


@pytest.mark.parametrize("K", [1, 2, 10, 64])
def test_rank_ce_matches_fp64_cross_entropy(K):
    """convdr_rank_ce_fwd_bwd against torch.nn.functional.cross_entropy in fp64 on the CPU.  Small logits: the bars of
    test_losses_match_torch.  Logits of the size trained ANCE embeddings produce (several hundred): the distance of plain
    fp32 torch on the CPU from the fp64 result is the yardstick, the kernel is allowed 3x that (another fp32 summation
    order, nothing more)."""
    from convdr_amd import _lib
    L = _lib.lib()
    rs = np.random.RandomState(100 + K)
    B, E = 16, 768
    for regime in ("small", "large"):
        if regime == "small":
            e = torch.from_numpy(rs.randn(B, E).astype(np.float32))
            d = torch.from_numpy(rs.randn(B, K, E).astype(np.float32)) * 0.05
        else:
            e = torch.from_numpy((0.6 * rs.randn(B, E) + 0.6).astype(np.float32))
            d = torch.from_numpy((0.6 * rs.randn(B, K, E) + 0.6).astype(np.float32))
        per64, g64, logits = _rank_ce_reference(e, d, torch.float64)
        if regime == "large":
            assert float(logits.abs().min()) > 150 and float(logits.abs().max()) > 300
        e_d, d_d = e.cuda(), d.cuda()
        z = _both_fills(lambda: {"per": torch.empty(B, dtype=torch.float32, device="cuda"), "de": torch.empty_like(e_d)},
                        lambda o: _lib.check(L.convdr_rank_ce_fwd_bwd(_lib.ptr(e_d), _lib.ptr(d_d), B, K, E, 1.0, _lib.ptr(o["per"]),
                                                                      _lib.ptr(o["de"]), 0, _lib.stream_ptr()),
                                             "convdr_rank_ce_fwd_bwd"), "E/rank_ce/%s/K%d" % (regime, K))
        per, de = z["per"].cpu().double(), z["de"].cpu().double()
        if regime == "small":
            assert abs(per.mean().item() - per64.mean().item()) < 1e-5 * max(1, abs(per64.mean().item()))
            assert torch.allclose(de.float(), g64.float(), rtol=1e-4, atol=1e-7)
        else:
            per32, g32, _ = _rank_ce_reference(e, d, torch.float32)
            y_loss = float((per32.double() - per64).abs().max())
            y_grad = float((g32.double() - g64).abs().max())
            m_loss, m_grad = float((per - per64).abs().max()), float((de - g64).abs().max())
            print("rank_ce large logits K=%d: loss fp32-vs-fp64 %.3g kernel %.3g; grad fp32-vs-fp64 %.3g kernel %.3g"
                  % (K, y_loss, m_loss, y_grad, m_grad))
            margin("stale/rank_ce_large_K%d/loss_abs_err" % K, m_loss, 3 * y_loss)
            margin("stale/rank_ce_large_K%d/grad_abs_err" % K, m_grad, 3 * y_grad)


def test_pair_nll_and_inbatch_ce_with_poisoned_outputs():
    from convdr_amd import _lib
    from oracle import train as OT
    L = _lib.lib()
    rs = np.random.RandomState(21)
    B, E = 7, 768
    q = torch.from_numpy(rs.randn(B, E).astype(np.float32) * 0.2)
    for Cn in (1, 4):
        a = torch.from_numpy(rs.randn(B, Cn, E).astype(np.float32) * 0.2)
        b = torch.from_numpy(rs.randn(B, Cn, E).astype(np.float32) * 0.2)
        qd, ad, bd = q.cuda(), a.cuda().contiguous(), b.cuda().contiguous()
        z = _both_fills(lambda: {"per": torch.empty(B, dtype=torch.float32, device="cuda"), "dq": torch.empty_like(qd),
                                 "da": torch.empty_like(ad), "db": torch.empty_like(bd)},
                        lambda o: _lib.check(L.convdr_pair_nll_fwd_bwd(_lib.ptr(qd), _lib.ptr(ad), _lib.ptr(bd), None, None, B, Cn, E, 1.0,
                                                                       _lib.ptr(o["per"]), _lib.ptr(o["dq"]), _lib.ptr(o["da"]),
                                                                       _lib.ptr(o["db"]), _lib.stream_ptr()), "convdr_pair_nll_fwd_bwd"),
                        "E/pair_nll/C%d" % Cn)
        ref_in = [t.clone().requires_grad_(True) for t in (q, a, b)]
        sa, sb = [(ref_in[0].unsqueeze(1) * x).sum(-1).max(1).values for x in ref_in[1:]]
        ref = -torch.log_softmax(torch.stack([sa, sb], 1), 1)[:, 0]
        ref.mean().backward()
        # the bars of test_pair_nll_kernel_matches_oracle
        assert abs(z["per"].mean().item() - ref.mean().item()) < 1e-5 * max(1.0, abs(ref.mean().item()))
        for n, r in zip(("dq", "da", "db"), ref_in):
            assert torch.allclose(z[n].cpu(), r.grad, rtol=1e-4, atol=1e-6), (Cn, n)
    for B, N, E in ((64, 5120, 768), (3, 7, 64), (1, 1, 128)):
        g = torch.Generator().manual_seed(B)
        embs = torch.randn(B, E, generator=g)
        docs = torch.randn(N, E, generator=g) * 0.3
        pos = torch.randint(0, N, (B,), generator=g)
        e_d, d_d, p_d = embs.cuda(), docs.cuda(), pos.to(torch.int32).cuda()
        z = _both_fills(lambda: {"per": torch.empty(B, dtype=torch.float32, device="cuda"), "de": torch.empty_like(e_d)},
                        lambda o: _lib.check(L.convdr_inbatch_ce_fwd_bwd(_lib.ptr(e_d), _lib.ptr(d_d), B, N, E, _lib.ptr(p_d), 1.0,
                                                                         _lib.ptr(o["per"]), _lib.ptr(o["de"]), 0, _lib.stream_ptr()),
                                             "convdr_inbatch_ce_fwd_bwd"), "E/inbatch_ce/%d" % B)
        e_ref = embs.clone().requires_grad_(True)
        ref = OT.inbatch_rank_loss(e_ref, docs, pos)
        ref.backward()
        # the bars of test_inbatch_negative_loss_matches_oracle
        assert abs(z["per"].mean().item() - ref.item()) < 1e-4 * max(1.0, abs(ref.item()))
        np.testing.assert_allclose(z["de"].cpu().numpy(), e_ref.grad.numpy(), rtol=2e-4, atol=2e-6)
