"""Ragged encoder entry and token-budget coalescing of evaluate(): everything that needs no GPU -- the export, the argument
validation of convdr_encoder_forward_ragged (which runs before any HIP call) and the host helpers of convdr_amd.inference."""
import ctypes as C

import numpy as np
import pytest

from convdr_amd import _lib

ENTRY = b"convdr_encoder_forward_ragged"
EVAL_LENS = [48, 7, 30, 1, 19, 48, 12, 33, 5, 41, 26]      # the evaluate fixture's lengths (tests/golden/make_golden.py)


def test_library_exports_the_ragged_entry():
    assert "convdr_encoder_forward_ragged" in _lib.exported_symbols()
    assert hasattr(_lib.lib(), "convdr_encoder_forward_ragged")


def _call(B=4, n_tokens=40, rows=64, max_len=16, tokens=16, offsets=32, ws_bytes=1 << 40):
    """Nothing here is ever dereferenced: every case returns from the validation in front of the first HIP call."""
    L = _lib.lib()
    cfg = _lib.EncoderConfig(kind=0, hidden=128, heads=2, layers=2, intermediate=256, vocab=200, max_pos=514, pad_idx=1,
                             out_dim=0, ln_eps=1e-5, head_ln_eps=1e-5, pool_mean=0)
    w = _lib.EncoderWeights()
    p = lambda v: None if v is None else C.c_void_p(v)
    return L.convdr_encoder_forward_ragged(C.byref(cfg), C.byref(w), p(tokens), n_tokens, p(offsets), B, p(48), p(64), rows,
                                           max_len, None, ws_bytes, None, None)


@pytest.mark.parametrize("what,kw", [("B = 0", dict(B=0)), ("rows % 8 != 0", dict(rows=60)), ("rows < n_tokens", dict(rows=32)),
                                     ("max_len = 0", dict(max_len=0)), ("max_len > n_tokens", dict(max_len=41)),
                                     ("n_tokens < B", dict(n_tokens=3, max_len=1)), ("null tokens", dict(tokens=None)),
                                     ("null tok_offsets", dict(offsets=None)), ("workspace too small", dict(ws_bytes=1024))])
def test_argument_validation_needs_no_gpu(what, kw):
    rc = _call(**kw)
    assert rc != 0, what
    assert ENTRY in _lib.lib().convdr_last_error(), (what, _lib.lib().convdr_last_error())


def test_flatten_prefix_batch():
    from convdr_amd.inference import _flatten_prefix_batch
    rs = np.random.RandomState(0)
    ids = rs.randint(3, 200, size=(3, 10)).astype(np.int64)
    lens = [10, 1, 4]
    mask = (np.arange(10)[None, :] < np.asarray(lens)[:, None]).astype(np.int64)
    ids *= mask                                           # right padding with id 0, like the collate function
    tokens, got = _flatten_prefix_batch(ids, mask)
    assert tokens.dtype == np.int32 and got.dtype == np.int32
    assert got.tolist() == lens
    assert tokens.tolist() == ids[0, :10].tolist() + ids[1, :1].tolist() + ids[2, :4].tolist()
    # a 0 followed by a 1: not a prefix mask
    hole = mask.copy()
    hole[0, 2] = 0                                        # 1,1,0,1,...
    assert _flatten_prefix_batch(ids, hole) is None
    hole = mask.copy()
    hole[2, 0] = 0                                        # even the CLS position
    assert _flatten_prefix_batch(ids, hole) is None
    # all ones
    tokens, got = _flatten_prefix_batch(ids, np.ones_like(mask))
    assert got.tolist() == [10, 10, 10] and np.array_equal(tokens, ids.reshape(-1).astype(np.int32))


@pytest.mark.parametrize("budget,expected", [
    (96, [(0, 4), (4, 7), (7, 10), (10, 11)]),
    (40, [(0, 1), (1, 3), (3, 5), (5, 6), (6, 7), (7, 8), (8, 9), (9, 10), (10, 11)]),      # below the longest sequence
    (312, [(0, 11)]),
])
def test_group_cutter_is_plan_batches(budget, expected):
    """Rounded to 8 the lengths are 48, 8, 32, 8, 24, 48, 16, 40, 8, 48, 32 (312 in all); the expected groups were cut by
    hand: greedy in order, a single longer sequence a group of its own."""
    from convdr_amd.encode import plan_batches
    from convdr_amd.inference import _GroupCutter, _cut_groups
    assert _cut_groups(EVAL_LENS, budget) == expected
    assert _cut_groups(iter(EVAL_LENS), budget) == plan_batches(EVAL_LENS, len(EVAL_LENS), budget, align=8)
    # streaming: a group is known as soon as the first sequence that does not fit is announced
    cut, seen = _GroupCutter(budget, align=8), []
    for i, n in enumerate(EVAL_LENS):
        g = cut.add(n)
        if g is not None:
            assert g[1] == i
            seen.append(g)
    assert seen + [cut.close()] == expected and cut.close() is None


def test_group_cutter_matches_plan_batches_on_random_lengths():
    from convdr_amd.encode import plan_batches
    from convdr_amd.inference import _cut_groups
    rs = np.random.RandomState(1)
    for budget in (8, 64, 250, 4096):
        lens = rs.randint(1, 300, size=200)
        assert _cut_groups(lens, budget) == plan_batches(lens, len(lens), budget, align=8)
