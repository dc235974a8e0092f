"""Shared cases of the GPU tests that compare a FlatIPIndex with the oracle row for row (range search, score and rank of given
rows, the row filter): stores and precisions, shapes, the corpus and canonical scores of a shape, the one resident index, and
the row-mask recipes.  Both stores hold the SAME corpus (synth_corpus rounded to half and widened), so one oracle run per shape
serves every store and precision.  Everything is computed once and never written to afterwards."""
import numpy as np
import pytest

from oracle import search as OS
from tests.golden.make_golden import synth_corpus

CONFIGS = [("fp32", "auto"), ("fp32", "bf16"), ("fp16", "auto")]
# n, nq, d, clustered
SHAPES = [
    (300, 3, 64, False),          # ragged last tile, one K step
    (257, 1, 100, False),         # padded width (d_in = 100), one query
    (5000, 37, 768, False),
    (33000, 130, 128, False),     # two query tiles (more than 128 queries or pairs): Tile256 and the r3 emit path
    (5000, 37, 768, True),        # a common component of norm ~30 plus unit noise: q . centre matters
]
MASKS = ["half", "one", "last_tile", "word_edges", "none"]

_CORPUS, _SCORES, _INDEX = {}, {}, {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def corpus(shape):
    """(P = halves widened to fp32, Q); computed once, never written to afterwards"""
    if shape not in _CORPUS:
        n, nq, d, clustered = shape
        P, Q = synth_corpus(100 + n % 97, n, d), synth_corpus(7, nq, d)
        if clustered:
            c = synth_corpus(9, 1, d)
            c *= np.float32(30.0) / np.linalg.norm(c)
            P, Q = P + c, Q + c
        P = P.astype(np.float16).astype(np.float32)
        P.setflags(write=False), Q.setflags(write=False)
        _CORPUS[shape] = (P, Q)
    return _CORPUS[shape]


def scores(shape):
    if shape not in _SCORES:
        P, Q = corpus(shape)
        S = OS.canonical_scores(Q, P)
        S.setflags(write=False)
        _SCORES[shape] = S
    return _SCORES[shape]


def index(shape, storage, precision):
    """one resident index per (shape, store, precision); one at a time"""
    from convdr_amd.search import FlatIPIndex
    key = (shape, storage, precision)
    if key not in _INDEX:
        _INDEX.clear()
        P, _ = corpus(shape)
        idx = FlatIPIndex(shape[2], storage=storage, precision=precision, prepin=False)
        idx.add(P.astype(np.float16) if storage == "fp16" else P)
        _INDEX[key] = idx
    idx = _INDEX[key]
    idx.cap, idx.RANGE_MAX_CAP = 4096, 131072
    return idx


def mask(n, name):
    """bool [n], the allowed rows of the recipe `name`"""
    m = np.zeros(n, bool)
    if name == "half":
        m = np.random.RandomState(11 + n).rand(n) < 0.5
    elif name == "most":
        m = np.random.RandomState(12 + n).rand(n) < 0.9
    elif name == "percent":
        m = np.random.RandomState(13 + n).rand(n) < 0.01
    elif name == "one":
        m[n // 3] = True
    elif name == "last_tile":                # only rows of the last, partial 256-row tile
        assert n % 256
        m[n // 256 * 256:] = True
    elif name == "word_edges":
        m[[31, 32, 63, 64, 255, 256]] = True
    else:
        assert name == "none"
    return m
