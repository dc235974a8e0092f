"""convdr_topk_merge_multi / convdr_topk_merge_packed (the W-way merge in one launch) against a numpy stable descending
sort of the concatenation, bit for bit; output pitch padding and stale output memory; parallel.merge_rank_topk /
exchange_topk reach the library through the new entry points."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILLS = ("Z", "N", "R")        # zeros, bytes 0xFF, seeded random bytes (the three fills of tests/helpers.py)
PAD_SCORE = np.float32(-3.4028234663852886e38)

#          W,   n,   nq, n_out
SHAPES = [(8, 100, 1000, 100),        # the product shape
          (2, 100, 37, 200),
          (3, 7, 5, 9),
          (1, 50, 4, 20),
          (16, 256, 11, 300),
          (8, 4096, 3, 4096),         # the LDS cap: 32768 staged scores
          (5, 1, 3, 5)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _fill_bytes(torch, t, kind, seed=0):
    assert t.is_contiguous()
    b = t.reshape(-1).view(torch.uint8)
    if kind == "Z":
        b.zero_()
    elif kind == "N":
        b.fill_(0xFF)
    else:
        g = torch.Generator(device=b.device).manual_seed(seed)
        b.copy_(torch.randint(0, 256, (b.numel(),), generator=g, dtype=torch.uint8, device=b.device))
    return t


def _lists(rs, W, n, nq):
    """[W, nq, n] scores drawn from 40 distinct values (ties inside and across lists are the rule), rows descending, the
    last list ending in a run of FAISS padding; ids random."""
    D = np.sort(rs.randint(0, 40, size=(W, nq, n)).astype(np.float32) * 0.25 - 3.0, axis=2)[:, :, ::-1].copy()
    I = rs.randint(0, 2 ** 62, size=(W, nq, n), dtype=np.int64)
    npad = max(1, n // 3) if n > 1 else 0
    if npad:
        D[W - 1, :, n - npad:] = PAD_SCORE
        I[W - 1, :, n - npad:] = -1
    return D, I


def _reference(D, I, n_out):
    W, nq, n = D.shape
    d = D.transpose(1, 0, 2).reshape(nq, W * n)
    i = I.transpose(1, 0, 2).reshape(nq, W * n)
    order = np.argsort(-d.astype(np.float64), axis=1, kind="stable")[:, :n_out]
    return np.take_along_axis(d, order, 1), np.take_along_axis(i, order, 1)


def _pack(D, I):
    """[W, nq, n] -> the wire format [W, nq, n, 3] int32: score bits, offset low word, offset high word."""
    W, nq, n = D.shape
    buf = np.empty((W, nq, n, 3), np.int32)
    buf[..., 0] = D.view(np.int32)
    buf[..., 1:] = np.ascontiguousarray(I).view(np.int32).reshape(W, nq, n, 2)
    return buf


def _call_multi(torch, Dt, It, W, n, list_stride, ld, nq, n_out, Do, Io, ldo):
    from convdr_amd import _lib
    _lib.check(_lib.lib().convdr_topk_merge_multi(_lib.ptr(Dt), _lib.ptr(It), W, n, list_stride, ld, nq, n_out, _lib.ptr(Do),
                                                  _lib.ptr(Io), ldo, _lib.stream_ptr()), "convdr_topk_merge_multi")


def _call_packed(torch, Pt, W, n, nq, n_out, Do, Io, ldo):
    from convdr_amd import _lib
    _lib.check(_lib.lib().convdr_topk_merge_packed(_lib.ptr(Pt), W, n, nq, n_out, _lib.ptr(Do), _lib.ptr(Io), ldo,
                                                   _lib.stream_ptr()), "convdr_topk_merge_packed")


def _same_bits(torch, Do, Io, rD, rI, what):
    assert np.array_equal(Do.cpu().numpy().view(np.int32), rD.view(np.int32)), "%s: scores" % (what,)
    assert np.array_equal(Io.cpu().numpy(), rI), "%s: ids" % (what,)


@pytest.mark.parametrize("W,n,nq,n_out", SHAPES)
def test_both_entry_points_equal_a_stable_sort_of_the_concatenation(torch_cuda, W, n, nq, n_out):
    torch = torch_cuda
    rs = np.random.RandomState(1000 * W + n)
    D, I = _lists(rs, W, n, nq)
    rD, rI = _reference(D, I, n_out)
    if W * n >= 200:
        assert (rD[:, 1:] == rD[:, :-1]).mean() > 0.3                 # ties really are the rule
    # tight layout
    Dt, It = torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda()
    Do = torch.empty((nq, n_out), dtype=torch.float32, device="cuda")
    Io = torch.empty((nq, n_out), dtype=torch.int64, device="cuda")
    _call_multi(torch, Dt, It, W, n, nq * n, n, nq, n_out, Do, Io, n_out)
    _same_bits(torch, Do, Io, rD, rI, ("multi", W, n, nq, n_out))
    # list_stride and ld larger than the tight ones
    ld, ls = n + 3, nq * (n + 3) + 17
    Dw = _fill_bytes(torch, torch.empty(W * ls, dtype=torch.float32, device="cuda"), "N")
    Iw = _fill_bytes(torch, torch.empty(W * ls, dtype=torch.int64, device="cuda"), "N")
    for w in range(W):
        Dw[w * ls:w * ls + nq * ld].view(nq, ld)[:, :n] = Dt[w]
        Iw[w * ls:w * ls + nq * ld].view(nq, ld)[:, :n] = It[w]
    Do2, Io2 = torch.empty_like(Do), torch.empty_like(Io)
    _call_multi(torch, Dw, Iw, W, n, ls, ld, nq, n_out, Do2, Io2, n_out)
    _same_bits(torch, Do2, Io2, rD, rI, ("multi/pitched", W, n, nq, n_out))
    # the wire format
    Pt = torch.from_numpy(_pack(D, I)).cuda()
    Do3, Io3 = torch.empty_like(Do), torch.empty_like(Io)
    _call_packed(torch, Pt, W, n, nq, n_out, Do3, Io3, n_out)
    _same_bits(torch, Do3, Io3, rD, rI, ("packed", W, n, nq, n_out))
    assert torch.equal(Do3.view(torch.int32), Do.view(torch.int32)) and torch.equal(Io3, Io)     # packed == unpacked


def test_a_list_of_padding_only_and_lists_of_one_repeated_score(torch_cuda):
    """A rank that owns no block contributes FAISS padding only; rows of one repeated score: every compare is a tie."""
    torch = torch_cuda
    W, n, nq, n_out = 4, 100, 9, 100
    D, I = _lists(np.random.RandomState(3), W, n, nq)
    D[1], I[1] = PAD_SCORE, -1
    D[:, 4:] = np.float32(1.5)                      # queries 4..8: all W * n scores equal (list 1 included)
    rD, rI = _reference(D, I, n_out)
    assert np.array_equal(rI[4:], I[0, 4:, :n_out])     # ... so the first list is the whole answer there
    Dt, It = torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda()
    Do = torch.empty((nq, n_out), dtype=torch.float32, device="cuda")
    Io = torch.empty((nq, n_out), dtype=torch.int64, device="cuda")
    _call_multi(torch, Dt, It, W, n, nq * n, n, nq, n_out, Do, Io, n_out)
    _same_bits(torch, Do, Io, rD, rI, "multi")
    Do2, Io2 = torch.empty_like(Do), torch.empty_like(Io)
    _call_packed(torch, torch.from_numpy(_pack(D, I)).cuda(), W, n, nq, n_out, Do2, Io2, n_out)
    _same_bits(torch, Do2, Io2, rD, rI, "packed")


@pytest.mark.parametrize("W,n,nq,n_out", [(8, 100, 37, 100), (3, 7, 5, 9), (8, 4096, 2, 4096), (5, 1, 3, 5)])
def test_output_padding_is_left_alone_and_stale_output_memory_is_not_read(torch_cuda, W, n, nq, n_out):
    torch = torch_cuda
    rs = np.random.RandomState(7 + W)
    D, I = _lists(rs, W, n, nq)
    rD, rI = _reference(D, I, n_out)
    Dt, It = torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda()
    Pt = torch.from_numpy(_pack(D, I)).cuda()
    ldo = n_out + 5
    for name in ("multi", "packed"):
        for j, f in enumerate(FILLS):
            Do = _fill_bytes(torch, torch.empty((nq, ldo), dtype=torch.float32, device="cuda"), f, seed=81 + j)
            Io = _fill_bytes(torch, torch.empty((nq, ldo), dtype=torch.int64, device="cuda"), f, seed=91 + j)
            pad = (Do[:, n_out:].clone(), Io[:, n_out:].clone())
            if name == "multi":
                _call_multi(torch, Dt, It, W, n, nq * n, n, nq, n_out, Do, Io, ldo)
            else:
                _call_packed(torch, Pt, W, n, nq, n_out, Do, Io, ldo)
            assert torch.equal(Do[:, n_out:].contiguous().view(torch.int32), pad[0].view(torch.int32)), (name, f, "padding written")
            assert torch.equal(Io[:, n_out:], pad[1]), (name, f, "padding written")
            _same_bits(torch, Do[:, :n_out].contiguous(), Io[:, :n_out].contiguous(), rD, rI, (name, f))


class _Counting:
    """Counts the calls that cross the _lib boundary for the merge entry points."""
    NAMES = ("convdr_topk_merge", "convdr_topk_merge_multi", "convdr_topk_merge_packed")

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


@pytest.mark.parametrize("W", [2, 3, 8])
def test_merge_rank_topk_is_one_launch_of_the_new_entry_point(torch_cuda, W):
    torch = torch_cuda
    from convdr_amd import parallel
    nq, k = 37, 100
    D, I = _lists(np.random.RandomState(20 + W), W, k, nq)
    Dc, Ic = parallel.merge_rank_topk(torch.from_numpy(D), torch.from_numpy(I), k)
    with _Counting() as c:
        Dg, Ig = parallel.merge_rank_topk(torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda(), k)
    assert c.calls == {"convdr_topk_merge": 0, "convdr_topk_merge_multi": 1, "convdr_topk_merge_packed": 0}, c.calls
    assert Dg.shape == (nq, k) and torch.equal(Dg.cpu().view(torch.int32), Dc.view(torch.int32)) and torch.equal(Ig.cpu(), Ic)
    # the private chain (the route of out-of-contract shapes) gives the same bits
    Dh, Ih = parallel._merge_rank_topk_chain(torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda(), k)
    assert torch.equal(Dh.view(torch.int32), Dg.view(torch.int32)) and torch.equal(Ih, Ig)


def test_merge_rank_topk_outside_the_contract_takes_the_chain(torch_cuda):
    torch = torch_cuda
    from convdr_amd import parallel
    W, nq, k = 9, 3, 4096                                  # W * k = 36864 > 32768
    D, I = _lists(np.random.RandomState(5), W, k, nq)
    Dc, Ic = parallel.merge_rank_topk(torch.from_numpy(D), torch.from_numpy(I), k)
    with _Counting() as c:
        Dg, Ig = parallel.merge_rank_topk(torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda(), k)
    assert c.calls == {"convdr_topk_merge": W - 1, "convdr_topk_merge_multi": 0, "convdr_topk_merge_packed": 0}, c.calls
    assert torch.equal(Dg.cpu().view(torch.int32), Dc.view(torch.int32)) and torch.equal(Ig.cpu(), Ic)


def test_exchange_topk_hands_the_gathered_buffer_to_the_packed_merge(torch_cuda):
    """World size 1 with force=True: the whole exchange path (pack, all-gather, merge) in a 1-rank RCCL group."""
    torch = torch_cuda
    import torch.distributed as dist
    from convdr_amd import parallel
    nq, k = 37, 100
    D, I = _lists(np.random.RandomState(9), 1, k, nq)
    Dt, It = torch.from_numpy(D[0]).cuda(), torch.from_numpy(I[0]).cuda()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29711", rank=0, world_size=1, device_id=Dt.device)
    try:
        with _Counting() as c:
            Dm, Im = parallel.exchange_topk(Dt, It, k, force=True)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert c.calls == {"convdr_topk_merge": 0, "convdr_topk_merge_multi": 0, "convdr_topk_merge_packed": 1}, c.calls
    assert torch.equal(Dm.view(torch.int32), Dt.view(torch.int32)) and torch.equal(Im, It)
