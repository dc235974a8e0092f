"""Distinct-document top-k on the host path (no GPU): search.distinct_topk against the reference's `seen_pid` walk, the
certificate that makes a document-level result taken from a row-level top-m exact, search_distinct_one_by_one and
parallel.search_blocks_sharded_distinct (gloo) over block files whose keys repeat inside and across blocks, and the
argument validation of convdr_topk_distinct."""
import os
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from convdr_amd import _lib, blocks, parallel
from convdr_amd import search as S
from tests import distinct_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ranked_lists(rs, nq, n, nkeys, pad_tail, pad_inside):
    D = np.sort(rs.randint(0, 12, size=(nq, n)).astype(np.float32) * 0.5 - 2.0, axis=1)[:, ::-1].copy()
    I = rs.randint(0, nkeys, size=(nq, n)).astype(np.int64)
    if pad_tail:
        for q in range(nq):
            t = rs.randint(0, n + 1)
            D[q, n - t:], I[q, n - t:] = DC.PAD_SCORE, -1
    if pad_inside:
        I[rs.rand(nq, n) < 0.15] = -1
    return D, I


@pytest.mark.parametrize("with_map", [False, True])
def test_distinct_topk_is_the_seen_pid_walk(with_map):
    rs = np.random.RandomState(3 + with_map)
    for case in range(60):
        nq, n = int(rs.randint(1, 6)), int(rs.randint(0, 70))
        k = int(rs.randint(1, 80))
        nids = int(rs.randint(1, 40))
        D, I = _ranked_lists(rs, nq, n, nids, case % 2 == 0, case % 3 == 0)
        key_map = (rs.randint(0, 12, size=nids).astype(np.int64) << (33 * (case % 2))) if with_map else None
        got = S.distinct_topk(D, I, k, key_map)
        want = DC.seen_walk(D, I, k, key_map)
        for g, w, name in zip(got, want, "DIKc"):
            assert DC.same_bits(g, w), (case, name, g, w)
    # an id past the map is dropped and reported, never looked up
    D, I = np.array([[3.0, 2.0, 1.0]], np.float32), np.array([[1, 7, 0]], np.int64)
    Do, Io, Ko, c = S.distinct_topk(D, I, 3, np.array([4, 4], np.int64))
    assert Io.tolist() == [[1, -1, -1]] and Ko.tolist() == [[4, -1, -1]] and c.tolist() == [[-1, 2]]
    # float64 scores (the host path of search_one_by_one) keep their dtype and bits
    Do = S.distinct_topk(D.astype(np.float64) / 3.0, I, 2)[0]
    assert Do.dtype == np.float64 and Do[0, 0] == 1.0 and Do[0, 1] == 2.0 / 3.0


def test_certified_prefix_equals_the_exhaustive_walk():
    """Rows in the canonical total order; the first k distinct keys of the whole order are the first k distinct keys of
    any prefix that holds k of them, or that is the whole corpus."""
    rs = np.random.RandomState(8)
    seen_open = seen_cert = 0
    for case in range(400):
        n = int(rs.randint(1, 61))
        k = int(rs.randint(1, 12))
        keys = np.repeat(np.arange(n), rs.randint(1, 5, size=n))[:n]
        keys = keys[rs.permutation(n)].astype(np.int64)
        mult = int(np.unique(keys, return_counts=True)[1].max())
        score = rs.randint(0, 8, size=n).astype(np.float32)                 # 8 values: ties are the rule
        order = np.lexsort((np.arange(n), -score))                          # score descending, lower row first
        D, rows = score[order][None], order[None].astype(np.int64)
        full = DC.seen_walk(D, rows, k, keys)
        for m in sorted(set([1, k, min(n, k * mult), n] + rs.randint(1, n + 1, size=4).tolist())):
            Dm, Im, Km, c = S.distinct_topk(D[:, :m], rows[:, :m], k, keys)
            certified = c[0, 0] >= k or c[0, 1] < m or m == n
            if certified:
                seen_cert += 1
                assert DC.same_bits(Dm, full[0]) and DC.same_bits(Im, full[1]) and DC.same_bits(Km, full[2]), (case, m)
            else:
                seen_open += 1
                assert c[0, 0] < k and c[0, 1] == m and m < n                # a proper prefix, full of rows, short of keys:
                assert (Km[0] >= 0).sum() == c[0, 0]                         # the row is short and its counts say so
            if m >= min(n, k * mult):
                assert certified, (case, m, k, mult)                         # depth k * multiplicity always suffices
    assert seen_open > 50 and seen_cert > 400


def test_search_distinct_one_by_one_equals_the_exhaustive_walk(tmp_path):
    Q, blocks_ = DC.corpus()
    DC.write_blocks(str(tmp_path), blocks_)
    eD, eI = DC.exhaustive(Q, blocks_, DC.TOPN)
    assert blocks.max_rows_per_key(str(tmp_path)) == DC.ROWS_PER_KEY
    assert blocks.max_rows_per_key(str(tmp_path), max_blocks=1) <= DC.ROWS_PER_KEY
    D, I = S.search_distinct_one_by_one(str(tmp_path), DC.OracleIndex(), Q, DC.TOPN)
    assert D.dtype == np.float64 and I.dtype == np.int64 and D.shape == I.shape == (DC.NQ, DC.TOPN)
    assert DC.same_bits(I, eI) and DC.same_bits(D, eD)
    # the plants are in the result: key 5000 once, at its best row's score; the duplicate vector once per key, earlier block first
    assert I[0, 0] == 5000 and (I[0] == 5000).sum() == 1
    assert I[1, :2].tolist() == [5001, 5002] and D[1, 0] == D[1, 1]
    assert I[2, :2].tolist() == [5003, 5004] and D[2, 0] == D[2, 1]
    # the plain row search of the same depth collapses to fewer documents
    rD, rI = S.search_one_by_one(str(tmp_path), DC.OracleIndex(), Q, DC.TOPN)
    assert len(set(rI[0, :DC.TOPN].tolist())) < DC.TOPN
    # keys through a map: unique record offsets, key_map[offset] = the key
    keys = np.concatenate([k for _, k in blocks_])
    starts = np.concatenate([[0], np.cumsum(DC.SIZES)])
    ids = [np.arange(starts[b], starts[b + 1], dtype=np.int64) for b in range(len(DC.SIZES))]
    (tmp_path / "mapped").mkdir()
    DC.write_blocks(str(tmp_path / "mapped"), blocks_, ids)
    assert blocks.max_rows_per_key(str(tmp_path / "mapped")) == 1
    assert blocks.max_rows_per_key(str(tmp_path / "mapped"), key_map=keys) == DC.ROWS_PER_KEY
    D2, I2 = S.search_distinct_one_by_one(str(tmp_path / "mapped"), DC.OracleIndex(), Q, DC.TOPN, key_map=keys)
    assert DC.same_bits(D2, eD) and DC.same_bits(keys[I2], eI)
    # an understated multiplicity is caught by the certificate, not papered over
    with pytest.raises(_lib.ConvdrError, match="understated"):
        S.search_distinct_one_by_one(str(tmp_path), DC.OracleIndex(), Q, DC.TOPN, rows_per_key=1)
    with pytest.raises(ValueError, match=r"1025.*4.*4100|4100"):
        S.search_distinct_one_by_one(str(tmp_path), DC.OracleIndex(), Q, 1025, rows_per_key=4)
    with pytest.raises(FileNotFoundError):
        S.search_distinct_one_by_one(str(tmp_path / "nothing"), DC.OracleIndex(), Q, DC.TOPN)


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
    # results come back through files and the children are spawned fresh, as in tests/test_block_shards_cpu.py
    import pickle
    import tempfile
    with tempfile.TemporaryDirectory(prefix="convdr_mp_") as td:
        mp.spawn(_worker, args=(world, port, fn, arg, td), nprocs=world, join=True)
        out = []
        for r in range(world):
            with open(os.path.join(td, "rank%d.pkl" % r), "rb") as f:
                out.append(pickle.load(f))
    return out


def _job(rank, world, dirname):
    Q = DC.corpus()[0]
    tm = {}
    D, I = parallel.search_blocks_sharded_distinct(dirname, DC.OracleIndex(), Q, DC.TOPN, timings=tm)
    try:
        parallel.search_blocks_sharded_distinct(dirname, DC.OracleIndex(), Q, DC.TOPN, rows_per_key=1)
        raised = False
    except _lib.ConvdrError:
        raised = True
    return D, I, tm, raised


def test_two_gloo_ranks_equal_one_process(tmp_path):
    Q, blocks_ = DC.corpus()
    DC.write_blocks(str(tmp_path), blocks_)
    one_D, one_I = S.search_distinct_one_by_one(str(tmp_path), DC.OracleIndex(), Q, DC.TOPN)
    out = _run(_job, str(tmp_path), 2, 29721)
    for r, (D, I, tm, raised) in enumerate(out):
        assert D.dtype == np.float64 and D.shape == I.shape == (DC.NQ, DC.TOPN)
        assert DC.same_bits(I, one_I) and DC.same_bits(D, one_D), r
        assert tm["block_ids"] == parallel.plan_block_shards(3, 2)[r]
        assert raised, "an understated rows_per_key must raise on every rank"
    # key 5000 has rows in blocks 0 and 1, i.e. on both ranks: one entry, the best row's score
    assert (one_I[0] == 5000).sum() == 1 and one_I[0, 0] == 5000
    # world size 1 (no process group): the same answer
    D, I = parallel.search_blocks_sharded_distinct(str(tmp_path), DC.OracleIndex(), Q, DC.TOPN)
    assert DC.same_bits(I, one_I) and DC.same_bits(D, one_D)
    with pytest.raises(ValueError, match="4100"):
        parallel.search_blocks_sharded_distinct(str(tmp_path), DC.OracleIndex(), Q, 1025, rows_per_key=4)


def test_argument_validation_needs_no_gpu():
    L = _lib.lib()

    def call(n, n_out, nq=3, ld=None, ldo=None, key_map_len=0):
        return L.convdr_topk_distinct(None, None, n, n if ld is None else ld, nq, None, key_map_len, n_out, None, None, None,
                                      n_out if ldo is None else ldo, None, None)
    for bad in (dict(n=4097, n_out=10), dict(n=10, n_out=4097), dict(n=-1, n_out=1), dict(n=10, n_out=-1),
                dict(n=10, n_out=5, nq=-1), dict(n=10, n_out=5, key_map_len=4)):
        assert call(**bad) != 0, bad
        assert b"convdr_topk_distinct: bad sizes" in L.convdr_last_error(), L.convdr_last_error()
    for bad in (dict(n=10, n_out=5, ld=9), dict(n=10, n_out=5, ldo=4)):
        assert call(**bad) != 0, bad
        assert b"convdr_topk_distinct: pitch" in L.convdr_last_error(), L.convdr_last_error()
    # nothing to do: accepted without a launch (and so without a GPU)
    assert call(10, 5, nq=0) == 0 and call(64, 0) == 0 and call(4096, 0) == 0
