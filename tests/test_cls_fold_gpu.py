"""The last layer's folded CLS path (csrc/cls_fold.hpp: Wk and Wv taken through the single CLS query, K and V never formed)
against the path it replaces (convdr_set_option("cls_fold", 0): K / V projection of every token + CLS-query attention) and
against the fp32 CPU oracle, on the same inputs.

Bars, per case:
  * each path's worst 1 - cos against the oracle is under the suite's COS_TOL = 1e-3;
  * the folded path's worst value is at most twice the unfolded path's: the fold drops the bf16 roundings of K and V and
    adds none of its own (fp32 U and Z enter the matrix unit as bf16 high + low parts), so it should be no worse; the
    factor two is slack for the other summation order;
  * folded vs unfolded 1 - cos is recorded beside the others (tests.helpers.margin), under the same COS_TOL;
  * two folded runs are bitwise equal, and the folded result does not depend on what the workspace held before
    (tests/helpers.py fills: zeros, 0xFF bytes, random bytes).

By default the fold is taken from 16,384 packed rows on (below, the unfolded path is faster: NOTEBOOK.md); the cases here lower
"cls_fold_min_rows" to 0, as other tests lower "fused_ln_min_rows", so that every shape runs the fold kernels, and one test
checks that the default gate routes a small batch to the unfolded path bit for bit.
"""
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from oracle import encoder as OE
from tests.helpers import cosine, margin, trained_like_
from tests.test_encoder_gpu import COS_TOL
from tests.test_stale_memory_gpu import _dpr_tiny, _forward_under_fills, _rb768, _sd
from tests.test_train_gpu import _batch, _tiny

pytestmark = pytest.mark.gpu

RAGGED = [1, 7, 8, 9, 127, 128]


MIN_ROWS_DEFAULT = 16384


@contextmanager
def _fold_from_row_zero():
    from convdr_amd import _lib
    L = _lib.lib()
    _lib.check(L.convdr_set_option(b"cls_fold_min_rows", 0), "convdr_set_option")
    try:
        yield
    finally:
        L.convdr_set_option(b"cls_fold_min_rows", MIN_ROWS_DEFAULT)


@contextmanager
def _unfolded():
    from convdr_amd import _lib
    L = _lib.lib()
    _lib.check(L.convdr_set_option(b"cls_fold", 0), "convdr_set_option")
    try:
        yield
    finally:
        L.convdr_set_option(b"cls_fold", 1)


def _rb12():
    from convdr_amd.model.models import MSMarcoConfigDict, RobertaConfig
    torch.manual_seed(0)
    model = MSMarcoConfigDict["rdot_nll"].model_class(RobertaConfig())
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.02)
            elif "LayerNorm.weight" in n or n == "norm.weight":
                p.add_(torch.randn_like(p) * 0.05)
    return model


def _rb12_trained():
    from convdr_amd.model.models import MSMarcoConfigDict, RobertaConfig
    torch.manual_seed(0)
    return trained_like_(MSMarcoConfigDict["rdot_nll"].model_class(RobertaConfig()), seed=5)


def _rdot(layers, heads):
    return lambda sd, ids, mask: OE.rdot_nll_emb(sd, ids, mask, num_layers=layers, num_heads=heads)


def _dpr(tower):
    return lambda sd, ids, mask: OE.dpr_emb(sd, ids, mask, tower=tower, num_layers=2, num_heads=2)


# name -> (model factory, method name, oracle, vocab, [(lens, L), ...])
CASES = {
    # roberta-base shape, N(0, 0.02) weights: the ragged edge lengths and one sequence of 510 tokens
    "roberta_base_ragged": (_rb12, "body_emb", _rdot(12, 12), 50000, [(RAGGED + [510], 512)]),
    # trained-checkpoint statistics (outlier dimensions, saturated heads): the lengths of the suite's own test of them
    "roberta_base_trained_stats": (_rb12_trained, "body_emb", _rdot(12, 12), 50000, [([512, 129, 8, 1, 300, 64], 512)]),
    # 768 wide, 2 layers: fixed length 128 with B = 70 (one whole 64-sequence tile of the fold kernels and a partial one),
    # and B = 1 with a full and with a one-token sequence; nine one-token sequences are too few packed rows to hold the
    # fold's U and Z in the places of K and V^T: that batch takes the unfolded path either way (folded vs unfolded: 0)
    "w768_fixed128_B70": (lambda: _rb768(2), "body_emb", _rdot(2, 12), 1000, [([128] * 70, 128)]),
    "w768_B1": (lambda: _rb768(2), "query_emb", _rdot(2, 12), 1000, [([128], 128), ([1], 128), ([77], 128), ([1] * 9, 128)]),
    # the 128-wide tiny model (2 heads: 14 of the 16 head columns of the pool kernel are padding)
    "tiny128": (lambda: _tiny(), "body_emb", _rdot(2, 2), 200, [(RAGGED, 128), ([128] * 5, 128), ([3] * 19 + [60], 128)]),
    # the DPR towers (BERT position ids, raw CLS output)
    "dpr_query": (lambda: _dpr_tiny(), "query_emb", _dpr("question_model"), 200, [([64, 1, 7, 8, 9, 63, 33, 40, 17], 64)]),
    "dpr_body": (lambda: _dpr_tiny(), "body_emb", _dpr("ctx_model"), 200, [([64, 1, 7, 8, 9, 63, 33, 40, 17], 64), ([64] * 3, 64)]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_folded_cls_layer_matches_unfolded_and_oracle(case):
    with _fold_from_row_zero():
        _run_case(case)


def test_default_gate_keeps_small_batches_unfolded_and_folds_large_ones():
    model = _rb768(2).cuda().eval()
    rs = np.random.RandomState(1)
    for B, folds in ((70, False), (130, True)):          # 8,960 and 16,640 packed rows
        ids, mask = _batch(rs, B, 128, [128] * B, vocab=1000)
        ids, mask = ids.cuda(), mask.cuda()
        with torch.no_grad():
            default = model.body_emb(ids, mask).clone()
            with _unfolded():
                unfolded = model.body_emb(ids, mask).clone()
            with _fold_from_row_zero():
                folded = model.body_emb(ids, mask).clone()
        assert not torch.equal(folded, unfolded)         # (the two forms differ at rounding level, so equality tells them apart)
        assert torch.equal(default, folded if folds else unfolded), (B, folds)


def _run_case(case):
    make, method, oracle, vocab, batches = CASES[case]
    model = make()
    sd = _sd(model)
    model = model.cuda().eval()
    fn = getattr(model, method)
    rs = np.random.RandomState(len(case))
    worst_f = worst_u = worst_fu = 0.0
    for lens, L in batches:
        ids, mask = _batch(rs, len(lens), L, lens, vocab=vocab)
        with torch.no_grad():
            ref = oracle(sd, ids, mask).numpy()
            ids_d, mask_d = ids.cuda(), mask.cuda()
            folded = fn(ids_d, mask_d).clone()
            again = fn(ids_d, mask_d).clone()
            with _unfolded():
                unfolded = fn(ids_d, mask_d).clone()
        assert bool(torch.isfinite(folded).all()) and bool(torch.isfinite(unfolded).all()), (case, lens)
        assert torch.equal(folded, again), "%s %s: two folded runs differ" % (case, lens)
        f, u = folded.cpu().numpy(), unfolded.cpu().numpy()
        worst_f = max(worst_f, float(1 - cosine(f, ref).min()))
        worst_u = max(worst_u, float(1 - cosine(u, ref).min()))
        worst_fu = max(worst_fu, float(1 - cosine(f, u).min()))
        # same bits whatever the workspace held (the fold's U and Z live where K and V^T were)
        filled = _forward_under_fills(lambda: fn(ids_d, mask_d), model, "cls_fold/%s/%s" % (case, len(lens)))
        assert torch.equal(filled, folded), "%s %s: result under workspace fills differs" % (case, lens)
    print("cls_fold %s: 1-cos folded %.3g unfolded %.3g folded-vs-unfolded %.3g" % (case, worst_f, worst_u, worst_fu))
    margin("cls_fold/%s/folded_worst_1-cos" % case, worst_f, COS_TOL)
    margin("cls_fold/%s/unfolded_worst_1-cos" % case, worst_u, COS_TOL)
    margin("cls_fold/%s/folded_vs_unfolded_1-cos" % case, worst_fu, COS_TOL)
    margin("cls_fold/%s/folded_over_unfolded" % case, worst_f, 2.0 * worst_u)
