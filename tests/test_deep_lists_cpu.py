"""Deep lists without a GPU: argument validation of convdr_topk_distinct_deep / convdr_topk_merge_deep[_packed] and the
workspace formula; the `max_depth` keyword of the distinct and sharded searches on the host path (OracleIndex) at row depth
4,400, in one process and over two gloo ranks, against the exhaustive walk."""
import os
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from convdr_amd import _lib, parallel
from convdr_amd import search as S
from convdr_amd.search import FlatIPIndex
from tests import deep_cases as XC
from tests import distinct_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEEP = FlatIPIndex.DEEP_MAX_K


# ---- the C entries ---------------------------------------------------------------------------------------------------
def test_distinct_deep_validates_before_any_device_call():
    L = _lib.lib()

    def call(n, n_out, nq=3, ld=None, ldo=None, key_map_len=0, ws=None):
        ws = L.convdr_topk_distinct_deep_workspace_bytes(max(nq, 0), max(n, 0)) if ws is None else ws
        return L.convdr_topk_distinct_deep(None, None, n, n if ld is None else ld, nq, None, key_map_len, n_out, None, None, None,
                                           n_out if ldo is None else ldo, None, None, ws, None)
    for bad in (dict(n=65537, n_out=10, ws=1 << 40), dict(n=10, n_out=65537), dict(n=-1, n_out=1), dict(n=10, n_out=-1),
                dict(n=10, n_out=5, nq=-1), dict(n=10, n_out=5, key_map_len=4)):
        assert call(**bad) != 0, bad
        assert b"convdr_topk_distinct_deep: bad sizes" in L.convdr_last_error(), L.convdr_last_error()
    for bad in (dict(n=5000, n_out=5, ld=4999), dict(n=5000, n_out=5, ldo=4)):
        assert call(**bad) != 0, bad
        assert b"convdr_topk_distinct_deep: pitch" in L.convdr_last_error(), L.convdr_last_error()
    assert call(5000, 5, ws=XC.distinct_ws_bytes(3, 5000) - 1) != 0
    assert b"convdr_topk_distinct_deep: workspace too small" in L.convdr_last_error(), L.convdr_last_error()
    # nothing to do: accepted without a launch (and so without a GPU)
    assert call(5000, 5, nq=0) == 0 and call(65536, 0) == 0 and call(0, 0) == 0


def test_distinct_deep_workspace_bytes():
    f = _lib.lib().convdr_topk_distinct_deep_workspace_bytes
    assert f(-1, 10) == 0 and f(3, -1) == 0 and f(3, 65537) == 0
    assert f(3, 5000) == XC.distinct_ws_bytes(3, 5000) == 120064 + 3 * 16384 * 4
    assert f(1, 65536) == 65536 * 8 + 131072 * 4           # 512 KB of keys + a 512 KB table
    assert f(0, 5000) == 0 and f(2, 0) == 2 * 256
    for n in (0, 1, 31, 32, 33, 4096, 4097, 5000, 65536):
        for nq in (1, 2, 7):
            assert f(nq, n) == XC.distinct_ws_bytes(nq, n), (nq, n)
    ns = (0, 1, 32, 33, 100, 4096, 4097, 8192, 8193, 40000, 65536)
    for nq in (1, 3, 100):
        vals = [f(nq, n) for n in ns]
        assert vals == sorted(vals) and f(nq + 1, 5000) > f(nq, 5000)


@pytest.mark.parametrize("name", ["convdr_topk_merge_deep", "convdr_topk_merge_deep_packed"])
def test_merge_deep_validates_before_any_device_call(name):
    L = _lib.lib()

    def call(nlists, n, n_out, nq=3, ldo=None):
        ldo = n_out if ldo is None else ldo
        if name.endswith("packed"):
            return L.convdr_topk_merge_deep_packed(None, nlists, n, nq, n_out, None, None, ldo, None)
        return L.convdr_topk_merge_deep(None, None, nlists, n, nq * n, n, nq, n_out, None, None, ldo, None)
    for bad in ((0, 10, 5), (65, 10, 5), (2, 65537, 5), (2, -1, 0), (2, 10, 21), (2, 10, -1)):
        assert call(*bad) != 0, bad
        assert (name + ": bad sizes").encode() in L.convdr_last_error(), L.convdr_last_error()
    assert call(2, 5000, 10, nq=-1) != 0 and (name + ": bad sizes").encode() in L.convdr_last_error()
    assert call(2, 5000, 10, ldo=9) != 0 and (name + ": pitch").encode() in L.convdr_last_error()
    # nothing to do: accepted without a launch -- a shape the shallow entry refuses among them (9 x 4096 staged scores)
    assert call(9, 4096, 4096, nq=0) == 0 and call(64, 65536, 65536, nq=0) == 0 and call(3, 5000, 0) == 0


# ---- the host path at depth ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deep_corpus(tmp_path_factory):
    Q, blocks_ = XC.corpus()
    d = tmp_path_factory.mktemp("deep_blocks")
    DC.write_blocks(str(d), blocks_)
    return str(d), Q, blocks_, DC.exhaustive(Q, blocks_, XC.TOPN)


def test_search_distinct_one_by_one_at_depth_4400(deep_corpus):
    d, Q, blocks_, (eD, eI) = deep_corpus
    D, I = S.search_distinct_one_by_one(d, DC.OracleIndex(), Q, XC.TOPN, rows_per_key=XC.ROWS_PER_KEY, max_depth=DEEP)
    assert D.dtype == np.float64 and I.dtype == np.int64 and D.shape == I.shape == (XC.NQ, XC.TOPN)
    assert DC.same_bits(I, eI) and DC.same_bits(D, eD)
    assert I[0, 0] == 50000 and (I[0] == 50000).sum() == 1 and I[1, :2].tolist() == [50001, 50002]
    assert (I >= 0).all()                                          # every query has TOPN documents
    # rows_per_key counted from the id files
    D2, I2 = S.search_distinct_one_by_one(d, DC.OracleIndex(), Q, XC.TOPN, max_depth=XC.M)
    assert DC.same_bits(I2, eI) and DC.same_bits(D2, eD)
    # the default refuses as before, names its limit; so does a max_depth below m
    with pytest.raises(ValueError, match=r"4400 is outside 1\.\.4096 \(FlatIPIndex\.MAX_K\)"):
        S.search_distinct_one_by_one(d, DC.OracleIndex(), Q, XC.TOPN, rows_per_key=XC.ROWS_PER_KEY)
    with pytest.raises(ValueError, match=r"4400 is outside 1\.\.4399 \(max_depth\)"):
        S.search_distinct_one_by_one(d, DC.OracleIndex(), Q, XC.TOPN, rows_per_key=XC.ROWS_PER_KEY, max_depth=XC.M - 1)
    # the plain row depth does not replace it: 1,100 rows hold fewer than 1,100 documents
    with pytest.raises(_lib.ConvdrError, match="understated"):
        S.search_distinct_one_by_one(d, DC.OracleIndex(), Q, XC.TOPN, rows_per_key=1, max_depth=DEEP)


@pytest.mark.parametrize("bad", [0, -1, 65537])
def test_max_depth_outside_its_range_raises(deep_corpus, bad):
    d, Q = deep_corpus[:2]
    with pytest.raises(ValueError, match="max_depth"):
        S.search_distinct_one_by_one(d, DC.OracleIndex(), Q, 10, rows_per_key=4, max_depth=bad)
    with pytest.raises(ValueError, match="max_depth"):
        parallel.search_blocks_sharded(d, DC.OracleIndex(), Q, 10, max_depth=bad)
    with pytest.raises(ValueError, match="max_depth"):
        parallel.search_blocks_sharded_distinct(d, DC.OracleIndex(), Q, 10, rows_per_key=4, max_depth=bad)


def test_sharded_defaults_refuse_what_they_refused(deep_corpus):
    d, Q = deep_corpus[:2]
    with pytest.raises(ValueError, match=r"topN = 4400 is outside 1\.\.4096 \(FlatIPIndex\.MAX_K\)"):
        parallel.search_blocks_sharded(d, DC.OracleIndex(), Q, XC.M)
    with pytest.raises(ValueError, match=r"4400 is outside 1\.\.4096 \(FlatIPIndex\.MAX_K\)"):
        parallel.search_blocks_sharded_distinct(d, DC.OracleIndex(), Q, XC.TOPN, rows_per_key=XC.ROWS_PER_KEY)
    with pytest.raises(ValueError, match=r"topN = 4400 is outside 1\.\.4399 \(max_depth\)"):
        parallel.search_blocks_sharded(d, DC.OracleIndex(), Q, XC.M, max_depth=XC.M - 1)


# ---- two gloo ranks --------------------------------------------------------------------------------------------------
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
    Q = XC.corpus()[0]
    tm = {}
    rows = parallel.search_blocks_sharded(dirname, DC.OracleIndex(), Q, XC.M, max_depth=DEEP, timings=tm)
    docs = parallel.search_blocks_sharded_distinct(dirname, DC.OracleIndex(), Q, XC.TOPN, rows_per_key=XC.ROWS_PER_KEY,
                                                   max_depth=DEEP)
    raised = []
    for bad in (0, 65537):
        try:
            parallel.search_blocks_sharded(dirname, DC.OracleIndex(), Q, 10, max_depth=bad)
            raised.append(False)
        except ValueError:
            raised.append(True)
    return rows, docs, tm, raised


def test_two_gloo_ranks_equal_one_process_at_depth_4400(deep_corpus):
    d, Q, blocks_, (eD, eI) = deep_corpus
    one_D, one_I = S.search_one_by_one(d, DC.OracleIndex(), Q, XC.M)
    one_D, one_I = one_D[:, :XC.M], one_I[:, :XC.M]
    out = _run(_job, d, 2, 29731)
    for r, (rows, docs, tm, raised) in enumerate(out):
        assert rows[0].shape == rows[1].shape == (XC.NQ, XC.M)
        # (the exchange carries fp32 scores: the host path's float64 scores are widened fp32 values)
        assert DC.same_bits(rows[1], one_I) and DC.same_bits(rows[0], one_D.astype(np.float32).astype(np.float64)), r
        assert DC.same_bits(docs[1], eI) and DC.same_bits(docs[0], eD), r
        assert tm["block_ids"] == parallel.plan_block_shards(3, 2)[r]
        assert raised == [True, True]
