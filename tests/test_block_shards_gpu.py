"""parallel.search_blocks_sharded with the REAL kernels: two processes share cuda:0 and talk over gloo (RCCL refuses two
ranks on one device), five block files on disk, FlatIPIndex with its pipelined two-blocks-in-flight loop per rank, the
exchange merged by convdr_topk_merge_packed.  Every rank must return what one process walking all five files returns."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES, DIM, TOPN, NQ = (6000, 9000, 20000, 7000, 12000), 768, 100, 37


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _worker(rank, world, port, fn, arg, ret):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pickle
        res = fn(rank, world, arg)
        with open(os.path.join(ret, "rank%d.pkl" % rank), "wb") as f:       # (`ret`: the parent's temporary directory)
            pickle.dump(res, f)
    finally:
        dist.destroy_process_group()


def _run(fn, arg, world, port):
    # results come back through files and the children are spawned fresh, as in tests/test_parallel_gpu.py
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
    """Five blocks of random rows with exact duplicates planted as the best hits of three queries: across the two ranks of a
    world-2 plan ([0, 1] | [2, 3, 4]: blocks 1 and 2, blocks 0 and 4) and inside one rank (blocks 2 and 3).  Record offsets run
    on across the blocks."""
    rs = np.random.RandomState(0)
    Q = rs.randn(NQ, DIM).astype(np.float32)
    embs = [rs.randn(n, DIM).astype(np.float32) for n in SIZES]
    for q, places in ((0, ((1, 77), (2, 4001))), (1, ((0, 5), (4, 11999))), (2, ((2, 0), (3, 6999)))):
        for b, row in places:
            embs[b][row] = 0.25 * Q[q]           # score 0.25 |q|^2 ~ 190: far above the random rows' ~ 4 x 28
    starts = np.concatenate([[0], np.cumsum(SIZES)])
    ids = [np.arange(starts[b], starts[b + 1], dtype=np.int64) for b in range(len(SIZES))]
    return Q, embs, ids


def _job(rank, world, dirname):
    from convdr_amd import parallel
    from convdr_amd import search as S
    Q = _corpus()[0]
    index = S.FlatIPIndex(DIM, device=torch.device("cuda", 0))
    tm = {}
    D, I = parallel.search_blocks_sharded(dirname, index, Q, TOPN, timings=tm)
    D1, I1 = S.search_one_by_one(dirname, index, Q, TOPN)       # one process over all five files, same child
    return D, I, D1[:, :TOPN], I1[:, :TOPN], tm


def test_two_ranks_over_five_block_files_equal_one_process(torch_cuda, tmp_path):
    from convdr_amd import blocks, parallel
    from oracle import search as OS
    Q, embs, ids = _corpus()
    for b, (e, i) in enumerate(zip(embs, ids)):
        blocks.dump_block(str(tmp_path / ("passage__emb_p__data_obj_%d.pb" % b)), e)
        blocks.dump_block(str(tmp_path / ("passage__embid_p__data_obj_%d.pb" % b)), i)
    mD, mI = OS.search_one_by_one(list(zip(embs, ids)), Q, TOPN)
    eD, eI = mD[:, :TOPN], mI[:, :TOPN]
    # the planted ties are in the expected result, earlier block first
    assert list(eI[0, :2]) == [int(ids[1][77]), int(ids[2][4001])]
    assert list(eI[1, :2]) == [int(ids[0][5]), int(ids[4][11999])]
    assert list(eI[2, :2]) == [int(ids[2][0]), int(ids[3][6999])]
    out = _run(_job, str(tmp_path), 2, 29712)
    plan = parallel.plan_block_shards(len(SIZES), 2)
    for r, (D, I, D1, I1, tm) in enumerate(out):
        assert D.dtype == np.float64 and I.dtype == np.int64 and D.shape == I.shape == (NQ, TOPN)
        assert np.array_equal(I, eI), "rank %d: ids differ from the oracle" % r
        assert np.array_equal(D, eD.astype(np.float32).astype(np.float64)), "rank %d: scores differ from the oracle" % r
        assert np.array_equal(I, I1) and np.array_equal(D, D1), "rank %d: differs from single-process search_one_by_one" % r
        assert tm["block_ids"] == plan[r] and tm["blocks"] == len(plan[r]) and tm["exchange_s"] > 0.0, tm
