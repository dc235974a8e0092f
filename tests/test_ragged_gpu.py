"""Ragged encoder entry (k_seq_pack_ragged -> convdr_encoder_forward_ragged -> EncoderTower.embed_ragged) against the padded
entry, and evaluate()'s token-budget coalescing against the reference-run fixture.

The two entries differ in the packing kernel only, so for the same sequences their tok_id / tok_pos words and their
embeddings are compared BITWISE.  Shapes: the tiny fixture models (2 layers, H = 128); lengths 1, 63, 64, 65, 9 and 129 cross
the packing kernel's 64-token step once and twice, B = 5 is no multiple of its 4 waves per workgroup, and the stream offsets
0, 1, 64, 128, 193, 202 leave every sequence but the first off a 16-byte boundary."""
import ctypes as C
import json
import logging
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import cosine

pytestmark = pytest.mark.gpu

COS_TOL = 1e-3           # the project's embedding bar (tests/test_encoder_gpu.py:_check)
MAX_ABS_TOL = 0.08
LENS5 = [1, 63, 64, 65, 9]


def _sd(z):
    return {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}


def _tiny_rdot(z, use_mean=False):
    from convdr_amd.model.models import MSMarcoConfigDict, RobertaConfig
    cfg = json.loads(str(z["config"]))
    model = MSMarcoConfigDict["rdot_nll"].model_class(RobertaConfig(**cfg), model_argobj=SimpleNamespace(use_mean=use_mean))
    missing, unexpected = model.load_state_dict(_sd(z), strict=False)
    assert not unexpected and all("pooler" in k for k in missing), (missing, unexpected)
    return model.cuda().eval()


def _tiny_dpr(golden_dir):
    from convdr_amd.model.models import MSMarcoConfigDict, BertConfig
    z = np.load(os.path.join(golden_dir, "encoder_dpr.npz"))
    args = SimpleNamespace(bert_config=BertConfig(**json.loads(str(z["config"]))))
    model = MSMarcoConfigDict["dpr"].model_class(args)
    missing, unexpected = model.load_state_dict(_sd(z), strict=False)
    assert not unexpected, unexpected
    return model.cuda().eval()


@pytest.fixture(scope="module")
def rdot(golden_dir):
    return _tiny_rdot(np.load(os.path.join(golden_dir, "encoder_rdot_nll.npz")))


@pytest.fixture(scope="module")
def dpr(golden_dir):
    return _tiny_dpr(golden_dir)


def _sequences(lens, vocab, pad_idx, seed):
    """Random in-table ids; the pad id planted INSIDE sequences (0 < l < len), at l = 63 and l = 64 where a sequence has them."""
    rs = np.random.RandomState(seed)
    seqs = []
    for n in lens:
        s = rs.randint(3, vocab, size=n).astype(np.int32)
        s[0] = 0
        for l in (5, 63, 64, n - 1):
            if 0 < l < n:
                s[l] = pad_idx
        seqs.append(s)
    return seqs


def _padded(seqs, width=None):
    L = max(len(s) for s in seqs) if width is None else width
    ids = np.zeros((len(seqs), L), np.int32)
    for b, s in enumerate(seqs):
        ids[b, :len(s)] = s
    return ids


def _pack_words(tower, head, lens):
    """tok_id / tok_pos (all rows, alignment rows included) that the tower's last forward left in its workspace."""
    from convdr_amd import _lib
    c = tower.packed(head)[0]
    rows = int(sum((n + 7) // 8 * 8 for n in lens))
    lay = (C.c_int64 * 14)()
    _lib.check(_lib.lib().convdr_encoder_debug_layout(C.byref(c), rows, len(lens), lay), "convdr_encoder_debug_layout")
    ws = tower._ws
    return tuple(ws[lay[i]:lay[i] + 4 * rows].view(torch.int32).clone() for i in (0, 1))


def _both_entries(tower, head, seqs, stale=False):
    lens = np.asarray([len(s) for s in seqs], np.int32)
    ids = torch.from_numpy(_padded(seqs)).cuda()
    tokens = torch.from_numpy(np.concatenate(seqs)).cuda()
    with torch.no_grad():
        a0 = tower.embed(ids, None, head=head, seq_lens=lens)
        a = tower.embed(ids, None, head=head, seq_lens=lens)
        wa = _pack_words(tower, head, lens)
        assert torch.equal(a0, a), "precondition: the padded entry does not repeat itself bit for bit"
        if stale:
            tower._ws.fill_(0xFF)
        r = tower.embed_ragged(tokens, lens, head=head)
        wr = _pack_words(tower, head, lens)
    torch.cuda.synchronize()
    return a, r, wa, wr


def _assert_same(a, r, wa, wr):
    assert torch.equal(wa[0], wr[0]), "tok_id differs"
    assert torch.equal(wa[1], wr[1]), "tok_pos differs"
    assert bool(torch.isfinite(a).all()) and torch.equal(a, r), "embeddings differ: max |d| = %g" % float((a - r).abs().max())


@pytest.mark.parametrize("lens", [LENS5, [129], [512, 3]], ids=["B5", "B1_L129", "position_table_end"])
@pytest.mark.parametrize("stale", [False, True], ids=["", "stale_ws"])
def test_ragged_pack_matches_padded_pack_roberta(rdot, lens, stale):
    """[512, 3]: the longest sequence RoBERTa's 514-row position table admits -- its last position is max_pos - 1."""
    from convdr_amd.train import check_status
    head = (rdot.embeddingHead, rdot.norm)
    seqs = _sequences(lens, 200, rdot.config.pad_token_id, seed=len(lens))
    if lens == LENS5:
        assert np.cumsum([0] + lens).tolist() == [0, 1, 64, 128, 193, 202]
    a, r, wa, wr = _both_entries(rdot.roberta, head, seqs, stale)
    _assert_same(a, r, wa, wr)
    check_status(rdot)
    # the pad id inside a sequence keeps position pad_idx and does not advance the count
    pos = wr[1].cpu().numpy()
    s, row0 = seqs[-1], int(sum((n + 7) // 8 * 8 for n in lens[:-1]))
    want = np.where(s != 1, 1 + np.cumsum(s != 1), 1)
    assert np.array_equal(pos[row0:row0 + len(s)], want)
    # and through the model surface
    with torch.no_grad():
        q = rdot.query_emb_ragged(torch.from_numpy(np.concatenate(seqs)).cuda(), [len(s) for s in seqs])
    assert torch.equal(q, r)


@pytest.mark.parametrize("lens", [LENS5, [129]], ids=["B5", "B1_L129"])
def test_ragged_pack_matches_padded_pack_bert(dpr, lens):
    from convdr_amd.train import check_status
    tower = dpr.question_model
    seqs = _sequences(lens, 200, 0, seed=7)
    a, r, wa, wr = _both_entries(tower, None, seqs)
    _assert_same(a, r, wa, wr)
    pos = wr[1].cpu().numpy()
    assert np.array_equal(pos[8:8 + 63], np.arange(63)) if lens == LENS5 else np.array_equal(pos[:129], np.arange(129))
    with torch.no_grad():
        q = dpr.query_emb_ragged(torch.from_numpy(np.concatenate(seqs)).cuda(), lens)
    assert torch.equal(q, r)
    check_status(dpr)


def test_ragged_pack_matches_padded_pack_use_mean(golden_dir):
    model = _tiny_rdot(np.load(os.path.join(golden_dir, "encoder_rdot_nll.npz")), use_mean=True)
    seqs = _sequences(LENS5, 200, 1, seed=11)
    lens = np.asarray(LENS5, np.int32)
    ids = torch.from_numpy(_padded(seqs)).cuda()
    with torch.no_grad():
        a = model.query_emb(ids, None, seq_lens=lens)
        r = model.query_emb_ragged(torch.from_numpy(np.concatenate(seqs)).cuda(), lens)
    assert model.roberta.pool_mean and torch.equal(a, r)
    # (mean pooling really ran: it is not the CLS embedding)
    model.use_mean = False
    with torch.no_grad():
        cls = model.query_emb_ragged(torch.from_numpy(np.concatenate(seqs)).cuda(), lens)
    assert not torch.equal(cls[1:], r[1:])


def _c_call(tower, head, seqs, ragged, claimed_lens=None, max_pos=None):
    """Either entry through the C ABI itself (what the Python tower refuses on the host: lengths that do not match the
    offsets, a position table shorter than the sequences).  Offsets always come from the true lengths, so every offset lies
    inside the stream.  -> (out, tok_id, tok_pos); the status word is posted to the tower."""
    from convdr_amd import _lib
    from convdr_amd.train import _status_post
    L_ = _lib.lib()
    true = np.asarray([len(s) for s in seqs], np.int32)
    lens_h = true if claimed_lens is None else np.asarray(claimed_lens, np.int32)
    B = len(seqs)
    cu_h = np.zeros(B + 1, np.int32)
    np.cumsum((lens_h + 7) // 8 * 8, out=cu_h[1:])
    off_h = np.zeros(B + 1, np.int32)
    np.cumsum(true, out=off_h[1:])
    rows = int(cu_h[-1])
    c0, w, _keep = tower.packed(head)
    c = _lib.EncoderConfig.from_buffer_copy(c0)
    if max_pos is not None:
        c.max_pos = max_pos
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cu, lens, off = dev(cu_h), dev(lens_h), dev(off_h)
    ws = torch.empty(L_.convdr_encoder_workspace_bytes(C.byref(c), rows, B), dtype=torch.uint8, device="cuda")
    out = torch.empty((B, c.out_dim or c.hidden), dtype=torch.float32, device="cuda")
    if ragged:
        tokens = dev(np.concatenate(seqs))
        assert int(off_h[-1]) == tokens.numel() and rows >= tokens.numel()
        _lib.check(L_.convdr_encoder_forward_ragged(C.byref(c), C.byref(w), _lib.ptr(tokens), tokens.numel(), _lib.ptr(off), B,
                                                    _lib.ptr(cu), _lib.ptr(lens), rows, int(lens_h.max()), _lib.ptr(ws), ws.numel(),
                                                    _lib.ptr(out), _lib.stream_ptr()), "convdr_encoder_forward_ragged")
    else:
        ids = dev(_padded(seqs, width=int(max(true.max(), lens_h.max()))))
        _lib.check(L_.convdr_encoder_forward(C.byref(c), C.byref(w), _lib.ptr(ids), 1, None, B, ids.shape[1], _lib.ptr(cu),
                                             _lib.ptr(lens), rows, int(lens_h.max()), _lib.ptr(ws), ws.numel(), _lib.ptr(out),
                                             _lib.stream_ptr()), "convdr_encoder_forward")
    _status_post(tower, ws)
    lay = (C.c_int64 * 14)()
    L_.convdr_encoder_debug_layout(C.byref(c), rows, B, lay)
    torch.cuda.synchronize()
    return (out,) + tuple(ws[lay[i]:lay[i] + 4 * rows].view(torch.int32).clone() for i in (0, 1))


@pytest.mark.parametrize("kind", ["roberta", "bert"])
def test_position_clamp_is_the_same_in_both_entries(rdot, dpr, kind):
    """Positions past the table are clamped to max_pos - 1 by both packing kernels.  The Python towers raise IndexError on the
    host before that can happen (check_positions), so this goes through the C ABI with max_pos lowered to 70 in the config
    (the real table has 514 rows: every clamped position is still a valid row)."""
    from convdr_amd.train import check_status
    tower, head = (rdot.roberta, (rdot.embeddingHead, rdot.norm)) if kind == "roberta" else (dpr.question_model, None)
    seqs = _sequences([129, 70, 69, 1], 200, 1 if kind == "roberta" else 0, seed=5)
    a = _c_call(tower, head, seqs, ragged=False, max_pos=70)
    r = _c_call(tower, head, seqs, ragged=True, max_pos=70)
    _assert_same(a[0], r[0], a[1:], r[1:])
    pos = r[2].cpu().numpy()
    assert pos.max() == 69 and (pos[:129] == 69).sum() > 50
    check_status(rdot if kind == "roberta" else dpr)


def test_status_bad_token(rdot):
    """An id equal to the table size: clamped and flagged by the packing kernel, IndexError at check_status."""
    from convdr_amd.train import check_status
    seqs = _sequences(LENS5, 200, 1, seed=3)
    seqs[3][64] = 200
    with torch.no_grad():
        out = rdot.query_emb_ragged(torch.from_numpy(np.concatenate(seqs)).cuda(), LENS5)
    assert bool(torch.isfinite(out).all())
    with pytest.raises(IndexError):
        check_status(rdot)
    check_status(rdot)          # (reported once)


def test_status_bad_lens_then_a_good_call(rdot):
    """seq_lens[1] overstated by one with the offsets unchanged (every offset inside the stream): the sequence is not read,
    the call returns, ValueError at check_status; the next good call is right."""
    from convdr_amd.train import check_status
    head = (rdot.embeddingHead, rdot.norm)
    seqs = _sequences(LENS5, 200, 1, seed=4)
    claimed = list(LENS5)
    claimed[1] += 1
    out, tok_id, tok_pos = _c_call(rdot.roberta, head, seqs, ragged=True, claimed_lens=claimed)
    assert bool(torch.isfinite(out).all())
    tok_id = tok_id.cpu().numpy()
    assert (tok_id[8:72] == -1).all() and (tok_pos.cpu().numpy()[8:72] == 0).all()      # the rejected sequence's rows: empty
    assert np.array_equal(tok_id[72:72 + 64], seqs[2])                                    # its neighbours: packed as usual
    with pytest.raises(ValueError):
        check_status(rdot)
    a, r, wa, wr = _both_entries(rdot.roberta, head, seqs)
    _assert_same(a, r, wa, wr)
    check_status(rdot)


def test_embed_ragged_rejects_bad_arguments_on_the_host(rdot):
    from convdr_amd import _lib
    tokens = torch.zeros(10, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        rdot.roberta.embed_ragged(tokens, [10, 0])                # a length < 1
    with pytest.raises(ValueError):
        rdot.roberta.embed_ragged(tokens, [4, 5])                 # lengths do not add up to the stream
    with pytest.raises(ValueError):
        rdot.roberta.embed_ragged(tokens.long(), [10])
    with pytest.raises(_lib.ConvdrError):
        rdot.roberta.embed_ragged(tokens.cpu(), [10])
    rdot.train()
    try:
        with pytest.raises(_lib.ConvdrError):                     # no ragged training path
            rdot.query_emb_ragged(tokens, [10])
    finally:
        rdot.eval()


# ---- evaluate() with a token budget ---------------------------------------------------------------------------------------
class _DS(torch.utils.data.Dataset):
    """The stub dataset of test_encoder_gpu.py::test_evaluate_loop_matches_reference_fixture."""

    def __init__(self, z, mask=None):
        self.ids, self.mask = z["ids"], z["mask"] if mask is None else mask
        self.qids = [str(q) for q in z["qids"]]
        self.hist = json.loads(str(z["hist"]))

    def __len__(self):
        return len(self.qids)

    def __getitem__(self, i):
        return i

    def get_collate_fn(self, args, mode):
        assert mode == "inference"
        return lambda idx: {"qid": [self.qids[i] for i in idx], "concat_ids": torch.from_numpy(self.ids[idx]),
                            "concat_id_mask": torch.from_numpy(self.mask[idx]), "history_utterances": [self.hist[i] for i in idx]}


def _args(z, **kw):
    return SimpleNamespace(per_gpu_eval_batch_size=int(z["batch"]), n_gpu=1, device=torch.device("cuda"), seed=42, **kw)


@pytest.fixture(scope="module")
def zeval(golden_dir):
    return np.load(os.path.join(golden_dir, "evaluate.npz"))


def _check(emb, ref, what):
    cs = cosine(emb, ref)
    assert cs.min() > 1 - COS_TOL, "%s: cosine %s" % (what, cs)
    assert np.abs(emb - ref).max() < MAX_ABS_TOL, "%s: max abs err %g" % (what, np.abs(emb - ref).max())


GROUPS = {96: [(0, 4), (4, 7), (7, 10), (10, 11)],
          40: [(0, 1), (1, 3), (3, 5), (5, 6), (6, 7), (7, 8), (8, 9), (9, 10), (10, 11)],
          262144: [(0, 11)]}


@pytest.mark.parametrize("budget", [96, 40, 262144])
@pytest.mark.parametrize("how", ["keyword", "args"])
def test_evaluate_with_budget_matches_reference_fixture(rdot, zeval, budget, how):
    from convdr_amd import inference
    z = zeval
    if how == "keyword":
        emb, emb2id, raw = inference.evaluate(_args(z), _DS(z), rdot, logging.getLogger("test"), token_budget=budget)
    else:
        emb, emb2id, raw = inference.evaluate(_args(z, eval_token_budget=budget), _DS(z), rdot, logging.getLogger("test"))
    assert emb.dtype == np.float32 and emb.shape == z["embedding"].shape
    _check(emb, z["embedding"], "evaluate(token_budget=%d)" % budget)
    assert emb2id == [str(q) for q in z["embedding2id"]]
    assert raw == json.loads(str(z["raw_sequences"]))
    st = inference.last_evaluate_stats
    assert st["groups"] == GROUPS[budget]
    assert st["forwards"] == len(GROUPS[budget]) == {96: 4, 40: 9, 262144: 1}[budget]
    assert st["padded_batches"] == 0 and st["token_budget"] == budget


def test_evaluate_without_budget_is_the_per_batch_loop(rdot, zeval):
    from convdr_amd import inference
    z = zeval
    emb, emb2id, raw = inference.evaluate(_args(z), _DS(z), rdot)
    st = dict(inference.last_evaluate_stats)
    assert st["forwards"] == 3 and st["token_budget"] is None and st["padded_batches"] == 0      # the DataLoader's 4 + 4 + 3
    assert st["groups"] == [(0, 4), (4, 8), (8, 11)]
    emb2, emb2id2, raw2 = inference.evaluate(_args(z), _DS(z), rdot)
    assert np.array_equal(emb, emb2) and emb2id == emb2id2 and raw == raw2
    _check(emb, z["embedding"], "evaluate")


def test_evaluate_budget_falls_back_for_a_mask_with_a_hole(rdot, zeval):
    """Query 5 (48 tokens, second DataLoader batch) gets a 0 inside its prefix: that batch goes through the padded call, the
    group in front of it is flushed first and the order stays.  Queries 0-3 keep their group (bit-equal); the others end up in
    other groups (batch-composition bound 1 - 1e-4); query 5 itself is another input."""
    from convdr_amd import inference
    z = zeval
    ref, ref2id, _ = inference.evaluate(_args(z), _DS(z), rdot, token_budget=96)
    mask = z["mask"].copy()
    assert mask[5].sum() == 48
    mask[5, 3] = 0
    emb, emb2id, raw = inference.evaluate(_args(z), _DS(z, mask), rdot, token_budget=96)
    st = inference.last_evaluate_stats
    assert st["padded_batches"] == 1 and st["forwards"] == 3 and st["groups"] == [(0, 4), (8, 11)]
    assert emb2id == ref2id == [str(q) for q in z["embedding2id"]]
    assert raw == json.loads(str(z["raw_sequences"]))
    assert np.array_equal(emb[:4], ref[:4])
    others = [4, 6, 7, 8, 9, 10]
    cs = cosine(emb[others], ref[others])
    assert cs.min() > 1 - 1e-4, cs
    assert not np.array_equal(emb[5], ref[5])


def test_evaluate_budget_model_without_ragged_entry_goes_padded(rdot, zeval):
    """A model that has no query_emb_ragged: every batch through today's call, same result as without a budget."""
    from convdr_amd import inference

    class Plain(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, ids, mask):
            return self.inner(ids, mask)
    z = zeval
    ref, _, _ = inference.evaluate(_args(z), _DS(z), rdot)
    emb, emb2id, _ = inference.evaluate(_args(z), _DS(z), Plain(rdot), token_budget=96)
    st = inference.last_evaluate_stats
    assert st["padded_batches"] == 3 and st["forwards"] == 3 and st["groups"] == []
    assert emb2id == [str(q) for q in z["embedding2id"]]
    cs = cosine(emb, ref)
    assert cs.min() > 1 - 1e-4, cs


def test_evaluate_budget_dpr(dpr, zeval):
    """BiEncoder (BERT kind, no head): the coalesced loop against its own per-batch result."""
    from convdr_amd import inference
    z = zeval
    ref, ref2id, _ = inference.evaluate(_args(z), _DS(z), dpr)
    assert inference.last_evaluate_stats["forwards"] == 3
    emb, emb2id, _ = inference.evaluate(_args(z), _DS(z), dpr, token_budget=96)
    st = inference.last_evaluate_stats
    assert st["groups"] == GROUPS[96] and st["forwards"] == 4 and st["padded_batches"] == 0
    assert emb2id == ref2id and emb.shape == ref.shape == (11, 128)
    cs = cosine(emb, ref)
    assert cs.min() > 1 - 1e-4, cs
