"""parallel.search_blocks_sharded on the host path (CPU, gloo): any number of block files over any number of ranks must
give what ONE process walking all blocks gives (oracle.search.search_one_by_one, first topN columns), bit for bit and
with the reference's tie order; plan_block_shards; argument validation of the W-way merge entry points (no GPU)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from convdr_amd import _lib, blocks, parallel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES, DIM, TOPN, NQ = (61, 45, 80, 33, 52), 64, 20, 9


def _worker(rank, world, port, fn, arg, ret):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pickle
        res = fn(rank, world, arg)
        with open(os.path.join(ret, "rank%d.pkl" % rank), "wb") as f:       # (`ret`: the parent's temporary directory)
            pickle.dump(res, f)
    finally:
        dist.destroy_process_group()


def _run(fn, arg, world, port):
    # results come back through files and the children are spawned fresh, as in tests/test_parallel_cpu.py
    import pickle
    import tempfile
    with tempfile.TemporaryDirectory(prefix="convdr_mp_") as td:
        mp.spawn(_worker, args=(world, port, fn, arg, td), nprocs=world, join=True)
        out = []
        for r in range(world):
            with open(os.path.join(td, "rank%d.pkl" % r), "rb") as f:
                out.append(pickle.load(f))
    return out


def _corpus():
    """Five blocks with exact duplicates in blocks (0, 3) and (1, 2, 4), each the best hit of one query; record offsets
    run on across the blocks.  Every block has at least TOPN rows."""
    rs = np.random.RandomState(0)
    Q = rs.randn(NQ, DIM).astype(np.float32)
    embs = [rs.randn(n, DIM).astype(np.float32) for n in SIZES]
    embs[0][5] = 3.0 * Q[0]
    embs[3][2] = embs[0][5]
    embs[1][4] = 3.0 * Q[1]
    embs[2][1] = embs[1][4]
    embs[4][0] = embs[1][4]
    starts = np.concatenate([[0], np.cumsum(SIZES)])
    ids = [np.arange(starts[b], starts[b + 1], dtype=np.int64) for b in range(len(SIZES))]
    return Q, embs, ids


def _write(dirname, embs, ids):
    for b, (e, i) in enumerate(zip(embs, ids)):
        blocks.dump_block(os.path.join(dirname, "passage__emb_p__data_obj_%d.pb" % b), e)
        blocks.dump_block(os.path.join(dirname, "passage__embid_p__data_obj_%d.pb" % b), i)


class OracleIndex:
    """add / search / reset played by the CPU oracle (no search_begin: the host path of the flow)."""

    def __init__(self):
        self.x = None

    def add(self, x):
        assert self.x is None
        self.x = np.asarray(x, np.float32)

    def search(self, q, k):
        from oracle import search as OS
        return OS.flat_ip_search(q, self.x, k)

    def reset(self):
        self.x = None


def _expected(Q, embs, ids):
    from oracle import search as OS
    mD, mI = OS.search_one_by_one(list(zip(embs, ids)), Q, TOPN)
    return mD[:, :TOPN], mI[:, :TOPN]


def _job(rank, world, dirname):
    Q = _corpus()[0]
    tm = {}
    D, I = parallel.search_blocks_sharded(dirname, OracleIndex(), Q, TOPN, timings=tm)
    return D, I, tm


def _merge_sorted(lists, k):
    """Stable descending sort of the concatenation, cut to k: the tie rule "earlier list first"."""
    D = np.concatenate([l[0] for l in lists], axis=1)
    I = np.concatenate([l[1] for l in lists], axis=1)
    order = np.argsort(-D, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(D, order, 1), np.take_along_axis(I, order, 1)


def _simulate(per_block, owners):
    """What W ranks return when rank r walks the blocks owners[r] in order and the ranks' lists are merged with ties to
    the lower rank (numpy alone: no process group)."""
    local = [_merge_sorted([per_block[b] for b in own], TOPN) for own in owners if own]
    return _merge_sorted(local, TOPN)


@pytest.mark.parametrize("B", range(0, 9))
def test_plan_block_shards_is_contiguous_balanced_and_complete(B):
    for W in range(1, 10):
        plan = parallel.plan_block_shards(B, W)
        assert len(plan) == W
        flat = [b for own in plan for b in own]
        assert flat == list(range(B)), (B, W, plan)                    # disjoint, complete, ascending with the rank
        for own in plan:
            assert own == list(range(own[0], own[0] + len(own))) if own else True
        lens = [len(own) for own in plan]
        assert max(lens) - min(lens) <= 1, (B, W, plan)


def test_fixture_tells_contiguous_from_round_robin_ownership():
    """The counter-example behind the ownership rule: on these five blocks a round-robin plan with rank-order ties does
    NOT reproduce the one-process walk, the contiguous plan does."""
    from oracle import search as OS
    Q, embs, ids = _corpus()
    eD, eI = _expected(Q, embs, ids)
    per_block = []
    for e, i in zip(embs, ids):
        D, I = OS.flat_ip_search(Q, e, TOPN)
        per_block.append((D.astype(np.float64), i[I]))
    B = len(SIZES)
    for W in (1, 2, 3, 4, 5, 7):
        D, I = _simulate(per_block, parallel.plan_block_shards(B, W))
        assert np.array_equal(I, eI) and np.array_equal(D, eD), W
    for W in (2, 3, 4):
        D, I = _simulate(per_block, [list(range(r, B, W)) for r in range(W)])
        assert np.array_equal(D, eD), W                                  # the scores agree ...
        assert not np.array_equal(I, eI), W                              # ... the order of the tied ids does not


@pytest.mark.parametrize("world,port", [(2, 29701), (3, 29702)])
def test_five_block_files_over_gloo_ranks_equal_one_process(tmp_path, world, port):
    Q, embs, ids = _corpus()
    _write(str(tmp_path), embs, ids)
    eD, eI = _expected(Q, embs, ids)
    out = _run(_job, str(tmp_path), world, port)
    plan = parallel.plan_block_shards(len(SIZES), world)
    for r, (D, I, tm) in enumerate(out):
        assert D.dtype == np.float64 and I.dtype == np.int64 and D.shape == I.shape == (NQ, TOPN)
        assert np.array_equal(I, eI), r
        assert np.array_equal(D, eD.astype(np.float32).astype(np.float64)), r
        assert tm["block_ids"] == plan[r] and tm["exchange_s"] >= 0.0
    # the planted ties are really in the result: both copies of the duplicate, earlier block first
    assert list(eI[0, :2]) == [int(ids[0][5]), int(ids[3][2])]
    assert list(eI[1, :3]) == [int(ids[1][4]), int(ids[2][1]), int(ids[4][0])]


def test_more_ranks_than_block_files(tmp_path):
    Q, embs, ids = _corpus()
    _write(str(tmp_path), embs[:2], ids[:2])
    eD, eI = _expected(Q, embs[:2], ids[:2])
    out = _run(_job, str(tmp_path), 3, 29703)
    assert [o[2]["block_ids"] for o in out] == [[], [0], [1]]
    for r, (D, I, tm) in enumerate(out):
        assert np.array_equal(I, eI), r
        assert np.array_equal(D, eD.astype(np.float32).astype(np.float64)), r


def test_world_size_one_is_search_one_by_one(tmp_path):
    from convdr_amd import search as S
    Q, embs, ids = _corpus()
    _write(str(tmp_path), embs, ids)
    tm = {}
    D, I = parallel.search_blocks_sharded(str(tmp_path), OracleIndex(), Q, TOPN, timings=tm)
    rD, rI = S.search_one_by_one(str(tmp_path), OracleIndex(), Q, TOPN)
    assert np.array_equal(D, rD[:, :TOPN]) and np.array_equal(I, rI[:, :TOPN])
    assert tm["block_ids"] == [0, 1, 2, 3, 4] and tm["exchange_s"] == 0.0
    assert parallel.count_blocks(str(tmp_path)) == 5 and parallel.count_blocks(str(tmp_path), max_blocks=3) == 3
    os.remove(os.path.join(str(tmp_path), "passage__embid_p__data_obj_2.pb"))      # a missing id file ends the list too
    assert parallel.count_blocks(str(tmp_path)) == 2


def test_topn_beyond_max_k_is_refused(tmp_path):
    with pytest.raises(ValueError, match="4096"):
        parallel.search_blocks_sharded(str(tmp_path), OracleIndex(), np.zeros((1, DIM), np.float32), 4097)


def test_merge_multi_argument_validation_needs_no_gpu():
    L = _lib.lib()
    assert hasattr(L, "convdr_topk_merge_multi") and hasattr(L, "convdr_topk_merge_packed")

    def multi(nlists, n, n_out, nq=3):
        return L.convdr_topk_merge_multi(None, None, nlists, n, nq * n, n, nq, n_out, None, None, n_out, None)

    def packed(nlists, n, n_out, nq=3):
        return L.convdr_topk_merge_packed(None, nlists, n, nq, n_out, None, None, n_out, None)
    for call, name in ((multi, b"convdr_topk_merge_multi"), (packed, b"convdr_topk_merge_packed")):
        for nlists, n, n_out in ((0, 10, 0),             # nlists = 0
                                 (2, 5000, 100),         # n > 4096
                                 (16, 4096, 4096),       # nlists * min(n, n_out) = 65536 > 32768
                                 (2, 10, 21)):           # n_out > nlists * n
            assert call(nlists, n, n_out) != 0, (name, nlists, n, n_out)
            assert name + b":" in L.convdr_last_error(), L.convdr_last_error()
        # nothing to do: accepted without a launch (and so without a GPU)
        assert call(8, 100, 100, nq=0) == 0 and call(8, 100, 0) == 0
    # pitches smaller than the row
    assert L.convdr_topk_merge_multi(None, None, 2, 10, 30, 9, 3, 10, None, None, 10, None) != 0
    assert b"convdr_topk_merge_multi: pitch" in L.convdr_last_error()
    assert L.convdr_topk_merge_packed(None, 2, 10, 3, 10, None, None, 9, None) != 0
    assert b"convdr_topk_merge_packed: pitch" in L.convdr_last_error()
