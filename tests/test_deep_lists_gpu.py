"""Deep lists on the device: convdr_topk_distinct_deep against the reference's `seen_pid` walk and
convdr_topk_merge_deep[_packed] against numpy's stable descending sort of the concatenation, bit for bit; stale workspace and
output memory; the routing of merge_rank_topk / exchange_topk / distinct_topk_device beyond 4,096 entries; the `max_depth`
keyword of FlatIPIndex.search_distinct, search_distinct_one_by_one and the two sharded searches with the real kernels."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import deep_cases as XC
from tests import distinct_cases as DC
from tests.helpers import FILLS, fill_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _deep_max():
    from convdr_amd.search import FlatIPIndex
    return FlatIPIndex.DEEP_MAX_K


# ---- convdr_topk_distinct_deep ---------------------------------------------------------------------------------------------
#                  nq,     n, n_out
DISTINCT_SHAPES = [(3, 4097, 1000), (2, 16385, 4097), (1, 65536, 65536), (2, 20000, 0), (0, 5000, 10), (5, 7, 9), (3, 4096, 1000)]


def _workspace(nq, n, fill="N", seed=0):
    from convdr_amd import _lib
    need = _lib.lib().convdr_topk_distinct_deep_workspace_bytes(nq, n)
    assert need == XC.distinct_ws_bytes(nq, n)
    return fill_bytes(torch.empty(max(need, 1), dtype=torch.uint8, device="cuda"), fill, seed=seed), need


def _distinct_deep(Dt, It, n, ld, nq, km, n_out, Do, Io, Ko, ldo, counts, ws, ws_bytes):
    from convdr_amd import _lib
    _lib.check(_lib.lib().convdr_topk_distinct_deep(_lib.ptr(Dt), _lib.ptr(It), n, ld, nq, _lib.ptr(km),
                                                    0 if km is None else km.numel(), n_out, _lib.ptr(Do), _lib.ptr(Io),
                                                    _lib.ptr(Ko), ldo, _lib.ptr(counts), _lib.ptr(ws), ws_bytes,
                                                    _lib.stream_ptr()), "convdr_topk_distinct_deep")


def _distinct_shallow(Dt, It, n, ld, nq, km, n_out, Do, Io, Ko, ldo, counts):
    from convdr_amd import _lib
    _lib.check(_lib.lib().convdr_topk_distinct(_lib.ptr(Dt), _lib.ptr(It), n, ld, nq, _lib.ptr(km), 0 if km is None else km.numel(),
                                               n_out, _lib.ptr(Do), _lib.ptr(Io), _lib.ptr(Ko), ldo, _lib.ptr(counts),
                                               _lib.stream_ptr()), "convdr_topk_distinct")


def _same(Do, Io, Ko, counts, want, what):
    rD, rI, rK, rc = want
    assert np.array_equal(Do.cpu().numpy().view(np.int32), rD.view(np.int32)), "%s: scores" % (what,)
    assert np.array_equal(Io.cpu().numpy(), rI), "%s: ids" % (what,)
    if Ko is not None:
        assert np.array_equal(Ko.cpu().numpy(), rK), "%s: keys" % (what,)
    if counts is not None:
        assert np.array_equal(counts.cpu().numpy(), rc), "%s: counts %s vs %s" % (what, counts.cpu().numpy().tolist(), rc.tolist())


def _outputs(nq, n_out):
    Do = fill_bytes(torch.empty((nq, n_out), dtype=torch.float32, device="cuda"), "N")
    Io = fill_bytes(torch.empty((nq, n_out), dtype=torch.int64, device="cuda"), "R", seed=3)
    Ko = fill_bytes(torch.empty((nq, n_out), dtype=torch.int64, device="cuda"), "R", seed=4)
    counts = torch.full((nq, 2), -77, dtype=torch.int32, device="cuda")
    return Do, Io, Ko, counts


@pytest.mark.parametrize("nq,n,n_out", DISTINCT_SHAPES)
def test_distinct_deep_equals_the_seen_pid_walk(torch_cuda, nq, n, n_out, monkeypatch):
    from convdr_amd import search as S
    from convdr_amd import toplists              # (owns distinct_topk_device and the global it reads)
    for ki, kind in enumerate(XC.KINDS):
        D, I, key_map = XC.distinct_case(kind, nq, n, 100 * n + 10 * nq + ki)
        want = DC.seen_walk(D, I, n_out, key_map)
        if kind == "oob" and nq and n:
            assert want[3][0, 0] == -1 and (nq == 1 or want[3][nq - 1, 0] == -1)
        if kind == "equal" and nq and n:
            assert (want[3] == [1, n]).all()
        Dt, It = torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda()
        km = None if key_map is None else torch.from_numpy(key_map).cuda()
        ws, need = _workspace(nq, n, "R", seed=ki)
        Do, Io, Ko, counts = _outputs(nq, n_out)
        _distinct_deep(Dt, It, n, n, nq, km, n_out, Do, Io, Ko, n_out, counts, ws, need)
        if n_out == 0 or nq == 0:
            assert (counts == -77).all()              # returned without a launch: nothing written
            continue
        _same(Do, Io, Ko, counts, want, (kind, nq, n, n_out))
        # Kout and counts NULL
        Do2, Io2 = torch.empty_like(Do), torch.empty_like(Io)
        _distinct_deep(Dt, It, n, n, nq, km, n_out, Do2, Io2, None, n_out, None, ws, need)
        assert torch.equal(Do2.view(torch.int32), Do.view(torch.int32)) and torch.equal(Io2, Io)
        if n <= 4096 and n_out <= 4096:               # the shallow kernel's own bytes
            Do3, Io3, Ko3, counts3 = _outputs(nq, n_out)
            _distinct_shallow(Dt, It, n, n, nq, km, n_out, Do3, Io3, Ko3, n_out, counts3)
            assert torch.equal(Do3.view(torch.int32), Do.view(torch.int32)) and torch.equal(Io3, Io)
            assert torch.equal(Ko3, Ko) and torch.equal(counts3, counts)
        # the python wrapper: one call, and a call its workspace budget splits into one query at a time
        _same(*S.distinct_topk_device(Dt, It, n_out, km), want, ("wrapper", kind, nq, n, n_out))
        if n > 4096 and nq > 1 and kind in ("mult", "oob"):
            monkeypatch.setattr(toplists, "DISTINCT_DEEP_WS_BYTES", XC.distinct_ws_bytes(1, n))
            names = _Counting.NAMES
            with _Counting() as c:
                got = S.distinct_topk_device(Dt, It, n_out, km)
            monkeypatch.setattr(toplists, "DISTINCT_DEEP_WS_BYTES", None)
            assert c.calls == dict({x: 0 for x in names}, convdr_topk_distinct_deep=nq), c.calls
            _same(*got, want, ("wrapper/split", kind, nq, n, n_out))


@pytest.mark.parametrize("nq,n,n_out", [(3, 4097, 1000), (2, 16385, 4097), (5, 7, 9)])
def test_distinct_deep_reads_no_stale_workspace_or_output_memory(torch_cuda, nq, n, n_out):
    for kind in ("padded", "map"):
        D, I, key_map = XC.distinct_case(kind, nq, n, 7 * n + nq)
        want = DC.seen_walk(D, I, n_out, key_map)
        km = None if key_map is None else torch.from_numpy(key_map).cuda()
        ld, ldo = n + 3, n_out + 5
        Dw = fill_bytes(torch.empty((nq, ld), dtype=torch.float32, device="cuda"), "N")
        Iw = fill_bytes(torch.empty((nq, ld), dtype=torch.int64, device="cuda"), "R", seed=5)       # garbage ids beside every row
        Dw[:, :n], Iw[:, :n] = torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda()
        runs = []
        for j, f in enumerate(("Z",) + FILLS):                  # the first two runs start from the same bytes: repeatability
            ws, need = _workspace(nq, n, f, seed=51 + j)
            Do = fill_bytes(torch.empty((nq, ldo), dtype=torch.float32, device="cuda"), f, seed=81 + j)
            Io = fill_bytes(torch.empty((nq, ldo), dtype=torch.int64, device="cuda"), f, seed=91 + j)
            Ko = fill_bytes(torch.empty((nq, ldo), dtype=torch.int64, device="cuda"), f, seed=71 + j)
            counts = fill_bytes(torch.empty((nq, 2), dtype=torch.int32, device="cuda"), f, seed=61 + j)
            pad = tuple(t[:, n_out:].clone() for t in (Do, Io, Ko))
            _distinct_deep(Dw, Iw, n, ld, nq, km, n_out, Do, Io, Ko, ldo, counts, ws, need)
            assert torch.equal(Do[:, n_out:].contiguous().view(torch.int32), pad[0].view(torch.int32)), (kind, f, "pad columns written")
            assert torch.equal(Io[:, n_out:], pad[1]) and torch.equal(Ko[:, n_out:], pad[2]), (kind, f, "pad columns written")
            _same(Do[:, :n_out].contiguous(), Io[:, :n_out].contiguous(), Ko[:, :n_out].contiguous(), counts, want, (kind, f))
            runs.append((tuple(t.cpu().numpy().tobytes() for t in (Do, Io, Ko, counts)),
                         tuple(t[:, :n_out].cpu().numpy().tobytes() for t in (Do, Io, Ko)) + (counts.cpu().numpy().tobytes(),)))
        assert runs[0][0] == runs[1][0], "two runs on the same bytes differ"
        assert all(r[1] == runs[0][1] for r in runs), "the result depends on what the workspace held"


# ---- convdr_topk_merge_deep / _packed ---------------------------------------------------------------------------------------
#               W,     n, nq, n_out
MERGE_SHAPES = [(2, 4097, 3, 4097), (8, 5000, 2, 5000), (3, 65536, 1, 65536), (16, 8192, 2, 100), (1, 5000, 2, 300),
                (9, 4096, 3, 4096), (8, 100, 37, 100)]


def _merge_deep(Dt, It, W, n, list_stride, ld, nq, n_out, Do, Io, ldo):
    from convdr_amd import _lib
    _lib.check(_lib.lib().convdr_topk_merge_deep(_lib.ptr(Dt), _lib.ptr(It), W, n, list_stride, ld, nq, n_out, _lib.ptr(Do),
                                                 _lib.ptr(Io), ldo, _lib.stream_ptr()), "convdr_topk_merge_deep")


def _merge_deep_packed(Pt, W, n, nq, n_out, Do, Io, ldo):
    from convdr_amd import _lib
    _lib.check(_lib.lib().convdr_topk_merge_deep_packed(_lib.ptr(Pt), W, n, nq, n_out, _lib.ptr(Do), _lib.ptr(Io), ldo,
                                                        _lib.stream_ptr()), "convdr_topk_merge_deep_packed")


def _same_merge(Do, Io, rD, rI, what):
    assert np.array_equal(Do.cpu().numpy().view(np.int32), rD.view(np.int32)), "%s: scores" % (what,)
    assert np.array_equal(Io.cpu().numpy(), rI), "%s: ids" % (what,)


@pytest.mark.parametrize("W,n,nq,n_out", MERGE_SHAPES)
def test_merge_deep_equals_a_stable_sort_of_the_concatenation(torch_cuda, W, n, nq, n_out):
    rs = np.random.RandomState(1000 * W + n)
    D, I = XC.merge_lists(rs, W, n, nq)
    rD, rI = XC.merge_reference(D, I, n_out)
    if W > 1:
        assert (rD[:, 1:] == rD[:, :-1]).mean() > 0.3                 # ties really are the rule
    Dt, It = torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda()
    Do = torch.empty((nq, n_out), dtype=torch.float32, device="cuda")
    Io = torch.empty((nq, n_out), dtype=torch.int64, device="cuda")
    _merge_deep(Dt, It, W, n, nq * n, n, nq, n_out, Do, Io, n_out)
    _same_merge(Do, Io, rD, rI, ("plain", W, n, nq, n_out))
    # list_stride and ld larger than the tight ones
    ld, ls = n + 3, nq * (n + 3) + 17
    Dw = fill_bytes(torch.empty(W * ls, dtype=torch.float32, device="cuda"), "N")
    Iw = fill_bytes(torch.empty(W * ls, dtype=torch.int64, device="cuda"), "N")
    for w in range(W):
        Dw[w * ls:w * ls + nq * ld].view(nq, ld)[:, :n] = Dt[w]
        Iw[w * ls:w * ls + nq * ld].view(nq, ld)[:, :n] = It[w]
    Do2, Io2 = torch.empty_like(Do), torch.empty_like(Io)
    _merge_deep(Dw, Iw, W, n, ls, ld, nq, n_out, Do2, Io2, n_out)
    _same_merge(Do2, Io2, rD, rI, ("pitched", W, n, nq, n_out))
    # the wire format
    Pt = torch.from_numpy(XC.merge_pack(D, I)).cuda()
    Do3, Io3 = torch.empty_like(Do), torch.empty_like(Io)
    _merge_deep_packed(Pt, W, n, nq, n_out, Do3, Io3, n_out)
    _same_merge(Do3, Io3, rD, rI, ("packed", W, n, nq, n_out))
    if n <= 4096 and W * min(n, n_out) <= 32768:                      # the shallow kernel's own bytes
        from convdr_amd import _lib
        Do4, Io4 = torch.empty_like(Do), torch.empty_like(Io)
        _lib.check(_lib.lib().convdr_topk_merge_multi(_lib.ptr(Dt), _lib.ptr(It), W, n, nq * n, n, nq, n_out, _lib.ptr(Do4),
                                                      _lib.ptr(Io4), n_out, _lib.stream_ptr()), "convdr_topk_merge_multi")
        assert torch.equal(Do4.view(torch.int32), Do.view(torch.int32)) and torch.equal(Io4, Io)


def test_merge_deep_a_list_of_padding_only_and_all_scores_equal(torch_cuda):
    W, n, nq, n_out = 4, 5000, 6, 5000
    D, I = XC.merge_lists(np.random.RandomState(3), W, n, nq)
    D[1], I[1] = XC.PAD_SCORE, -1
    D[:, 3:] = np.float32(1.5)                      # queries 3..5: all W * n scores equal (list 1 included)
    rD, rI = XC.merge_reference(D, I, n_out)
    assert np.array_equal(rI[3:], I[0, 3:, :n_out])     # ... so the first list is the whole answer there
    Dt, It = torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda()
    Do = torch.empty((nq, n_out), dtype=torch.float32, device="cuda")
    Io = torch.empty((nq, n_out), dtype=torch.int64, device="cuda")
    _merge_deep(Dt, It, W, n, nq * n, n, nq, n_out, Do, Io, n_out)
    _same_merge(Do, Io, rD, rI, "plain")
    Do2, Io2 = torch.empty_like(Do), torch.empty_like(Io)
    _merge_deep_packed(torch.from_numpy(XC.merge_pack(D, I)).cuda(), W, n, nq, n_out, Do2, Io2, n_out)
    _same_merge(Do2, Io2, rD, rI, "packed")


@pytest.mark.parametrize("W,n,nq,n_out", [(2, 4097, 3, 4097), (8, 5000, 2, 777), (3, 7, 5, 9)])
def test_merge_deep_leaves_output_padding_alone_and_reads_no_stale_output(torch_cuda, W, n, nq, n_out):
    rs = np.random.RandomState(7 + W)
    D, I = XC.merge_lists(rs, W, n, nq)
    rD, rI = XC.merge_reference(D, I, n_out)
    Dt, It = torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda()
    Pt = torch.from_numpy(XC.merge_pack(D, I)).cuda()
    ldo = n_out + 5
    for name in ("plain", "packed"):
        for j, f in enumerate(FILLS):
            Do = fill_bytes(torch.empty((nq, ldo), dtype=torch.float32, device="cuda"), f, seed=81 + j)
            Io = fill_bytes(torch.empty((nq, ldo), dtype=torch.int64, device="cuda"), f, seed=91 + j)
            pad = (Do[:, n_out:].clone(), Io[:, n_out:].clone())
            if name == "plain":
                _merge_deep(Dt, It, W, n, nq * n, n, nq, n_out, Do, Io, ldo)
            else:
                _merge_deep_packed(Pt, W, n, nq, n_out, Do, Io, ldo)
            assert torch.equal(Do[:, n_out:].contiguous().view(torch.int32), pad[0].view(torch.int32)), (name, f, "padding written")
            assert torch.equal(Io[:, n_out:], pad[1]), (name, f, "padding written")
            _same_merge(Do[:, :n_out].contiguous(), Io[:, :n_out].contiguous(), rD, rI, (name, f))


# ---- routing ---------------------------------------------------------------------------------------------------------
class _Counting:
    """Counts the calls that cross the _lib boundary for the list entry points."""
    NAMES = ("convdr_topk_merge", "convdr_topk_merge_multi", "convdr_topk_merge_packed", "convdr_topk_merge_deep",
             "convdr_topk_merge_deep_packed", "convdr_topk_distinct", "convdr_topk_distinct_deep")

    def __init__(self):
        from convdr_amd import _lib
        self.L = _lib.lib()
        self.calls = {n: 0 for n in self.NAMES}
        self.real = {n: getattr(self.L, n) for n in self.NAMES}

    def __enter__(self):
        for n in self.NAMES:
            def wrapped(*a, _n=n):
                self.calls[_n] += 1
                return self.real[_n](*a)
            setattr(self.L, n, wrapped)
        return self

    def __exit__(self, *exc):
        for n in self.NAMES:
            setattr(self.L, n, self.real[n])


def _only(name, times=1):
    return dict({n: 0 for n in _Counting.NAMES}, **{name: times})


def test_merge_rank_topk_beyond_4096_is_one_deep_launch(torch_cuda):
    from convdr_amd import parallel
    W, nq, k = 3, 3, 5000
    D, I = XC.merge_lists(np.random.RandomState(23), W, k, nq)
    Dc, Ic = parallel.merge_rank_topk(torch.from_numpy(D), torch.from_numpy(I), k)
    with _Counting() as c:
        Dg, Ig = parallel.merge_rank_topk(torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda(), k)
    assert c.calls == _only("convdr_topk_merge_deep"), c.calls
    assert Dg.shape == (nq, k) and torch.equal(Dg.cpu().view(torch.int32), Dc.view(torch.int32)) and torch.equal(Ig.cpu(), Ic)


def test_exchange_topk_beyond_4096_hands_the_gathered_buffer_to_the_deep_packed_merge(torch_cuda):
    """World size 1 with force=True: the whole exchange path (pack, all-gather, merge) in a 1-rank RCCL group."""
    from convdr_amd import parallel
    nq, k = 3, 5000
    D, I = XC.merge_lists(np.random.RandomState(9), 1, k, nq)
    Dt, It = torch.from_numpy(D[0]).cuda(), torch.from_numpy(I[0]).cuda()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29732", rank=0, world_size=1, device_id=Dt.device)
    try:
        with _Counting() as c:
            Dm, Im = parallel.exchange_topk(Dt, It, k, force=True)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert c.calls == _only("convdr_topk_merge_deep_packed"), c.calls
    assert torch.equal(Dm.view(torch.int32), Dt.view(torch.int32)) and torch.equal(Im, It)


# ---- FlatIPIndex.search_distinct(max_depth=) -----------------------------------------------------------------------------
N_ROWS, DIM, NQ, K, LEAD = 9000, 64, 4, 10, 4500


def test_search_distinct_certifies_beyond_4096_rows(torch_cuda):
    """4,500 near-best rows of ONE key lead query 0: its first ten documents end inside row depth 5,120, past MAX_K."""
    from convdr_amd._lib import ConvdrError
    from convdr_amd.search import FlatIPIndex
    rs = np.random.RandomState(31)
    Q = rs.randn(NQ, DIM).astype(np.float32)
    P = rs.randn(N_ROWS, DIM).astype(np.float32)
    keys = np.repeat(np.arange(N_ROWS), rs.randint(1, 5, size=N_ROWS))[:N_ROWS][rs.permutation(N_ROWS)].astype(np.int64) + 2 ** 34
    lead = rs.permutation(N_ROWS)[:LEAD]
    for j, r in enumerate(lead):
        P[r], keys[r] = (2.5 - 1e-4 * j) * Q[0], 6
    D, rows = DC.total_order(Q, [(P, keys)])
    want = DC.seen_walk(D, rows, K, keys)
    depths = [20 * 2 ** j for j in range(9)]                         # 20 .. 5120
    prefix = {m: DC.seen_walk(D[:, :m], rows[:, :m], K, keys)[3] for m in depths}
    searched, final, todo = [], np.zeros((NQ, 2), np.int32), np.arange(NQ)
    for m in depths:
        searched.append(len(todo))
        final[todo] = prefix[m][todo]
        todo = todo[prefix[m][todo, 0] < K]
    assert len(todo) == 0 and searched[-1] == 1 and prefix[2560][0, 0] == 1      # query 0 alone reaches depth 5,120
    idx = FlatIPIndex(DIM)
    idx.add(P)
    kt = torch.from_numpy(keys).cuda()
    with _Counting() as c:
        Dd, Id, Kd, counts = idx.search_distinct(torch.from_numpy(Q).cuda(), K, kt, max_depth=_deep_max())
    _same(Dd, Id, Kd, counts, (want[0], want[1], want[2], final), "max_depth")
    assert idx.distinct_stats == {"depths": depths, "searched": searched}, idx.distinct_stats
    assert c.calls["convdr_topk_distinct_deep"] == 1 and c.calls["convdr_topk_distinct"] == len(depths) - 1, c.calls
    assert Kd[0, 0].item() == 6 and Id[0, 0].item() == lead[0]
    with pytest.raises(ConvdrError, match="4096"):
        idx.search_distinct(torch.from_numpy(Q).cuda(), K, kt)
    with pytest.raises(ValueError, match="max_depth"):
        idx.search_distinct(torch.from_numpy(Q).cuda(), K, kt, max_depth=_deep_max() + 1)
    # a block of one key: no depth holds two keys, the whole block certifies
    big = FlatIPIndex(DIM)
    big.add(rs.randn(6000, DIM).astype(np.float32))
    one_key = torch.zeros(6000, dtype=torch.int64, device="cuda")
    Dd, Id, Kd, counts = big.search_distinct(Q[:2], 2, one_key, depth=4096, max_depth=_deep_max())
    assert counts.cpu().numpy().tolist() == [[1, 6000], [1, 6000]] and (Kd[:, 0] == 0).all() and (Kd[:, 1] == -1).all()
    assert big.distinct_stats == {"depths": [4096, 6000], "searched": [2, 2]}, big.distinct_stats


# ---- search_distinct_one_by_one and the sharded flows at row depth 4,400 ------------------------------------------------------
@pytest.fixture(scope="module")
def deep_corpus(tmp_path_factory):
    Q, blocks_ = XC.corpus()
    d = tmp_path_factory.mktemp("deep_blocks")
    DC.write_blocks(str(d), blocks_)
    keys = np.concatenate([k for _, k in blocks_])
    starts = np.concatenate([[0], np.cumsum(XC.SIZES)])
    mapped = tmp_path_factory.mktemp("deep_blocks_mapped")
    DC.write_blocks(str(mapped), blocks_, [np.arange(starts[b], starts[b + 1], dtype=np.int64) for b in range(3)])
    return str(d), str(mapped), Q, keys, DC.exhaustive(Q, blocks_, XC.TOPN)


def test_search_distinct_one_by_one_at_depth_4400_on_the_device(torch_cuda, deep_corpus):
    from convdr_amd import search as S
    from convdr_amd.search import FlatIPIndex
    d, mapped, Q, keys, (eD, eI) = deep_corpus
    with _Counting() as c:
        D, I = S.search_distinct_one_by_one(d, FlatIPIndex(XC.DIM), Q, XC.TOPN, rows_per_key=XC.ROWS_PER_KEY, max_depth=_deep_max())
    assert c.calls["convdr_topk_distinct_deep"] == 1 and c.calls["convdr_topk_distinct"] == 0, c.calls
    assert D.dtype == np.float64 and I.dtype == np.int64
    assert DC.same_bits(I, eI) and DC.same_bits(D, eD)
    assert I[0, 0] == 50000 and (I[0] == 50000).sum() == 1 and I[1, :2].tolist() == [50001, 50002]
    D2, I2 = S.search_distinct_one_by_one(mapped, FlatIPIndex(XC.DIM), Q, XC.TOPN, key_map=keys, max_depth=_deep_max())
    assert DC.same_bits(D2, eD) and DC.same_bits(keys[I2], eI)
    with pytest.raises(ValueError, match="4400"):
        S.search_distinct_one_by_one(d, FlatIPIndex(XC.DIM), Q, XC.TOPN, rows_per_key=XC.ROWS_PER_KEY)


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
    # results come back through files and the children are spawned fresh, as in tests/test_block_shards_gpu.py
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
    from convdr_amd import parallel
    from convdr_amd import search as S
    Q = XC.corpus()[0]
    index = S.FlatIPIndex(XC.DIM, device=torch.device("cuda", 0))
    deep = S.FlatIPIndex.DEEP_MAX_K
    tm = {}
    rows = parallel.search_blocks_sharded(dirname, index, Q, XC.M, max_depth=deep, timings=tm)
    docs = parallel.search_blocks_sharded_distinct(dirname, index, Q, XC.TOPN, rows_per_key=XC.ROWS_PER_KEY, max_depth=deep)
    one = S.search_one_by_one(dirname, index, Q, XC.M)           # one process over all three files, same child
    return rows, docs, (one[0][:, :XC.M], one[1][:, :XC.M]), tm


def test_two_ranks_on_one_gpu_equal_one_process_at_depth_4400(torch_cuda, deep_corpus):
    from convdr_amd import parallel
    d, _, Q, keys, (eD, eI) = deep_corpus
    out = _run(_job, d, 2, 29733)
    for r, (rows, docs, one, tm) in enumerate(out):
        assert rows[0].shape == rows[1].shape == (XC.NQ, XC.M)
        assert DC.same_bits(rows[1], one[1]) and DC.same_bits(rows[0], one[0]), "rank %d: rows differ from one process" % r
        assert DC.same_bits(docs[1], eI) and DC.same_bits(docs[0], eD), "rank %d: documents differ from the exhaustive walk" % r
        assert tm["block_ids"] == parallel.plan_block_shards(3, 2)[r]
