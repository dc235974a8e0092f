"""convdr_topk_distinct (the first entry per key of a ranked list, one launch) against the reference's `seen_pid` walk in
numpy, bit for bit: score bits, ids, keys and the (n_distinct, n_valid) certificate; pitches, stale output memory and
repeatability; FlatIPIndex.search_distinct and search_distinct_one_by_one against the exhaustive walk over the oracle's
canonical order."""
import numpy as np
import pytest

from tests import distinct_cases as DC
from tests.helpers import FILLS, fill_bytes

pytestmark = pytest.mark.gpu

#         nq,   n, n_out
SHAPES = [(3, 1, 1), (5, 7, 9), (37, 100, 100), (11, 400, 100), (3, 4096, 1000), (2, 4096, 4096), (4, 64, 0), (0, 10, 5)]
KINDS = ("equal", "distinct", "mult", "high", "padded", "map", "oob")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _case(kind, nq, n, seed):
    """-> (D [nq, n] descending with ties, I [nq, n], key_map or None)."""
    if nq == 0:
        D, I, key_map = _case(kind, 1, n, seed)
        return D[:0], I[:0], key_map
    rs = np.random.RandomState(seed)
    D = np.sort(rs.randint(0, 40, size=(nq, n)).astype(np.float32) * 0.25 - 3.0, axis=1)[:, ::-1].copy()
    key_map = None
    if kind == "equal":
        I = np.full((nq, n), 2 ** 40 + 17, np.int64)
    elif kind == "distinct":
        I = np.stack([rs.permutation(n) for _ in range(nq)]).astype(np.int64).reshape(nq, n) * 3 + 2 ** 33
    elif kind == "high":                              # ids that differ only above bit 32 (and repeat)
        I = (rs.randint(0, max(1, n // 2), size=(nq, n)).astype(np.int64) << 32) + 12345
    elif kind in ("map", "oob"):
        nids = max(2, n)
        I = rs.randint(0, nids, size=(nq, n)).astype(np.int64)
        key_map = (rs.randint(0, max(1, n // 2), size=nids).astype(np.int64) << (32 * (seed % 2))) + 7
        if kind == "oob" and nq and n:
            I[0, n // 2] = nids                       # one id past the map in query 0: never looked up
            if nq > 1 and n > 2:
                I[nq - 1, n - 1] = 2 ** 62
    else:                                             # "mult", "padded": every key on 1..4 rows
        I = np.stack([np.repeat(rs.permutation(n), rs.randint(1, 5, size=n))[:n][rs.permutation(n)] for _ in range(nq)])
        I = I.astype(np.int64).reshape(nq, n) + 2 ** 35
    if kind == "padded" and n:
        for q in range(nq):                           # a FAISS padding tail, and padding ids inside the row
            t = rs.randint(0, n // 2 + 1)
            D[q, n - t:], I[q, n - t:] = DC.PAD_SCORE, -1
        I[rs.rand(nq, n) < 0.1] = -1
    return D, I, key_map


def _call(torch, Dt, It, n, ld, nq, km, n_out, Do, Io, Ko, ldo, counts):
    from convdr_amd import _lib
    _lib.check(_lib.lib().convdr_topk_distinct(_lib.ptr(Dt), _lib.ptr(It), n, ld, nq, _lib.ptr(km), 0 if km is None else km.numel(),
                                               n_out, _lib.ptr(Do), _lib.ptr(Io), _lib.ptr(Ko), ldo, _lib.ptr(counts),
                                               _lib.stream_ptr()), "convdr_topk_distinct")


def _same(torch, Do, Io, Ko, counts, want, what):
    rD, rI, rK, rc = want
    assert np.array_equal(Do.cpu().numpy().view(np.int32), rD.view(np.int32)), "%s: scores" % (what,)
    assert np.array_equal(Io.cpu().numpy(), rI), "%s: ids" % (what,)
    assert np.array_equal(Ko.cpu().numpy(), rK), "%s: keys" % (what,)
    if counts is not None:
        assert np.array_equal(counts.cpu().numpy(), rc), "%s: counts %s vs %s" % (what, counts.cpu().numpy().tolist(), rc.tolist())


@pytest.mark.parametrize("nq,n,n_out", SHAPES)
def test_kernel_equals_the_seen_pid_walk(torch_cuda, nq, n, n_out):
    torch = torch_cuda
    for ki, kind in enumerate(KINDS):
        D, I, key_map = _case(kind, nq, n, 100 * n + 10 * nq + ki)
        want = DC.seen_walk(D, I, n_out, key_map)
        if kind == "oob" and nq and n:
            assert want[3][0, 0] == -1 and (nq == 1 or n <= 2 or want[3][nq - 1, 0] == -1)
        if kind == "equal" and nq and n:
            assert (want[3][:, 0] == 1).all()
        Dt, It = torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda()
        km = None if key_map is None else torch.from_numpy(key_map).cuda()
        Do = fill_bytes(torch.empty((nq, n_out), dtype=torch.float32, device="cuda"), "N")
        Io = fill_bytes(torch.empty((nq, n_out), dtype=torch.int64, device="cuda"), "R", seed=3)
        Ko = fill_bytes(torch.empty((nq, n_out), dtype=torch.int64, device="cuda"), "R", seed=4)
        counts = torch.full((nq, 2), -77, dtype=torch.int32, device="cuda")
        _call(torch, Dt, It, n, n, nq, km, n_out, Do, Io, Ko, n_out, counts)
        if n_out == 0:
            assert (counts == -77).all()              # returned without a launch: nothing written
            continue
        _same(torch, Do, Io, Ko, counts, want, (kind, nq, n, n_out))
        # the python wrapper, without the key output pointer
        from convdr_amd.search import distinct_topk_device
        got = distinct_topk_device(Dt, It, n_out, km)
        _same(torch, *got, want, ("wrapper", kind, nq, n, n_out))
        Do2 = torch.empty_like(Do)
        Io2 = torch.empty_like(Io)
        _call(torch, Dt, It, n, n, nq, km, n_out, Do2, Io2, None, n_out, None)
        assert torch.equal(Do2.view(torch.int32), Do.view(torch.int32)) and torch.equal(Io2, Io)


@pytest.mark.parametrize("nq,n,n_out", [(5, 7, 9), (37, 100, 100), (11, 400, 100), (3, 4096, 1000), (2, 4096, 4096)])
def test_pitches_stale_output_memory_and_repeatability(torch_cuda, nq, n, n_out):
    torch = torch_cuda
    for kind in ("padded", "map"):
        D, I, key_map = _case(kind, nq, n, 7 * n + nq)
        want = DC.seen_walk(D, I, n_out, key_map)
        km = None if key_map is None else torch.from_numpy(key_map).cuda()
        ld, ldo = n + 3, n_out + 5
        Dw = fill_bytes(torch.empty((nq, ld), dtype=torch.float32, device="cuda"), "N")
        Iw = fill_bytes(torch.empty((nq, ld), dtype=torch.int64, device="cuda"), "R", seed=5)       # garbage ids beside every row
        Dw[:, :n], Iw[:, :n] = torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda()
        runs = []
        for j, f in enumerate(FILLS + ("Z",)):                  # the last two runs start from the same bytes: repeatability
            Do = fill_bytes(torch.empty((nq, ldo), dtype=torch.float32, device="cuda"), f, seed=81 + j)
            Io = fill_bytes(torch.empty((nq, ldo), dtype=torch.int64, device="cuda"), f, seed=91 + j)
            Ko = fill_bytes(torch.empty((nq, ldo), dtype=torch.int64, device="cuda"), f, seed=71 + j)
            counts = fill_bytes(torch.empty((nq, 2), dtype=torch.int32, device="cuda"), f, seed=61 + j)
            pad = tuple(t[:, n_out:].clone() for t in (Do, Io, Ko))
            _call(torch, Dw, Iw, n, ld, nq, km, n_out, Do, Io, Ko, ldo, counts)
            assert torch.equal(Do[:, n_out:].contiguous().view(torch.int32), pad[0].view(torch.int32)), (kind, f, "pad columns written")
            assert torch.equal(Io[:, n_out:], pad[1]) and torch.equal(Ko[:, n_out:], pad[2]), (kind, f, "pad columns written")
            _same(torch, Do[:, :n_out].contiguous(), Io[:, :n_out].contiguous(), Ko[:, :n_out].contiguous(), counts, want, (kind, f))
            runs.append(tuple(t.cpu().numpy().tobytes() for t in (Do, Io, Ko, counts)))
        assert runs[0] == runs[-1], "two runs on the same bytes differ"


# ---- FlatIPIndex.search_distinct ---------------------------------------------------------------------------------------
N_ROWS, DIM, NQ, K = 5000, 64, 9, 10


@pytest.fixture(scope="module")
def keyed_block():
    """5,000 rows whose keys own 1..4 rows, exact duplicate rows planted as the best hits of three queries (under one key
    and under two), and the exhaustive document-level answer over the oracle's canonical order."""
    rs = np.random.RandomState(21)
    Q = rs.randn(NQ, DIM).astype(np.float32)
    P = rs.randn(N_ROWS, DIM).astype(np.float32)
    keys = np.repeat(np.arange(N_ROWS), rs.randint(1, 5, size=N_ROWS))[:N_ROWS][rs.permutation(N_ROWS)].astype(np.int64) + 2 ** 34
    for q, rows, ks in ((0, (40, 41, 4000), (1, 1, 2)), (1, (7, 3000, 3001, 4500), (3, 3, 3, 3)), (2, (100, 200), (4, 5))):
        for r, k in zip(rows, ks):
            P[r], keys[r] = 3.0 * Q[q], k
    for j, r in enumerate(range(1000, 1012)):          # twelve near-best rows of ONE key for query 3: 2k rows hold < k keys
        P[r], keys[r] = (2.5 - 0.01 * j) * Q[3], 6
    D, rows = DC.total_order(Q, [(P, keys)])
    want = DC.seen_walk(D, rows, K, keys)
    # the reference's own counts over every prefix depth a search may visit: which queries a pass leaves uncertified
    prefix_counts = {m: DC.seen_walk(D[:, :m], rows[:, :m], K, keys)[3] for m in (10, 20, 40, 80, 160)}
    return Q, P, keys, want, prefix_counts


def _expected_passes(prefix_counts, start):
    """(depths, queries searched per pass, counts of the pass that certified each query) of a search that starts at
    depth `start` and doubles: a query stays open while its prefix holds fewer than K keys."""
    depths, searched, final = [], [], np.zeros((NQ, 2), np.int32)
    todo, m = np.arange(NQ), start
    while len(todo):
        depths.append(m)
        searched.append(len(todo))
        final[todo] = prefix_counts[m][todo]
        todo = todo[prefix_counts[m][todo, 0] < K]
        m *= 2
    return depths, searched, final


def _index(torch, P):
    from convdr_amd.search import FlatIPIndex
    idx = FlatIPIndex(DIM)
    idx.add(P)
    return idx


def test_search_distinct_equals_the_exhaustive_walk(torch_cuda, keyed_block):
    torch = torch_cuda
    Q, P, keys, want, prefix_counts = keyed_block
    idx = _index(torch, P)
    kt = torch.from_numpy(keys).cuda()
    D, I, Kk, counts = idx.search_distinct(torch.from_numpy(Q).cuda(), K, kt)
    assert D.shape == I.shape == Kk.shape == (NQ, K) and counts.shape == (NQ, 2)
    # query 3 holds 12 rows of one key among its best: the first pass (2k rows) cannot certify it, a deeper one does.  Which
    # passes run, over how many queries, and the counts they certify with, all follow from the reference walk
    depths, searched, final = _expected_passes(prefix_counts, 2 * K)
    assert len(depths) >= 2 and prefix_counts[2 * K][3, 0] < K
    _same(torch, D, I, Kk, counts, (want[0], want[1], want[2], final), "default depth")
    assert idx.distinct_stats["depths"] == depths and idx.distinct_stats["searched"] == searched, idx.distinct_stats
    assert I[0, 0].item() == 40 and Kk[0, :2].tolist() == [1, 2] and I[1, 0].item() == 7 and I[2, :2].tolist() == [100, 200]
    # a start depth of 10 forces the deepening path for most queries: the same answer
    D2, I2, K2, c2 = idx.search_distinct(torch.from_numpy(Q).cuda(), K, kt, depth=10)
    depths, searched, final = _expected_passes(prefix_counts, 10)
    assert searched[1] >= 3                                 # queries 0, 1 and 3 hold a repeated key in their ten best rows
    assert idx.distinct_stats["depths"] == depths and idx.distinct_stats["searched"] == searched, idx.distinct_stats
    assert np.array_equal(c2.cpu().numpy(), final)
    assert torch.equal(D2.view(torch.int32), D.view(torch.int32)) and torch.equal(I2, I) and torch.equal(K2, Kk)
    # numpy queries, a key vector that is too short
    D3, I3, _, _ = idx.search_distinct(Q, K, kt)
    assert torch.equal(D3.view(torch.int32), D.view(torch.int32)) and torch.equal(I3, I)
    from convdr_amd._lib import ConvdrError
    with pytest.raises(ConvdrError, match="keys"):
        idx.search_distinct(Q, K, kt[:100].contiguous())


def test_search_distinct_on_a_corpus_with_fewer_keys_than_k(torch_cuda, keyed_block):
    torch = torch_cuda
    Q, P, keys, _, _ = keyed_block
    n = 15
    small_keys = np.array([3, 3, 4, 5, 5, 5, 6, 7, 7, 8, 8, 8, 8, 9, 9], np.int64)        # 7 keys < K
    idx = _index(torch, P[:n])
    D, rows = DC.total_order(Q, [(P[:n], small_keys)])
    want = DC.seen_walk(D, rows, K, small_keys)
    kt = torch.from_numpy(small_keys).cuda()
    for depth in (None, 2 * K):                       # m == ntotal, and m > ntotal: the list runs out of rows (n_valid < m)
        Dd, Id, Kd, counts = idx.search_distinct(torch.from_numpy(Q).cuda(), K, kt, depth=depth)
        _same(torch, Dd, Id, Kd, counts, (want[0], want[1], want[2], np.tile(np.array([[7, n]], np.int32), (NQ, 1))), depth)
        assert (Id[:, 7:] == -1).all() and (Kd[:, 7:] == -1).all()
        assert len(idx.distinct_stats["depths"]) == 1
    # strict: an uncertifiable query at the limit raises and names it; otherwise the short row comes back with its counts
    rs = np.random.RandomState(2)
    big = _index(torch, rs.randn(6000, DIM).astype(np.float32))
    one_key = torch.zeros(6000, dtype=torch.int64, device="cuda")
    from convdr_amd._lib import ConvdrError
    with pytest.raises(ConvdrError, match="4096"):
        big.search_distinct(Q[:2], 2, one_key, depth=4096)
    Dd, Id, Kd, counts = big.search_distinct(Q[:2], 2, one_key, depth=4096, strict=False)
    assert counts.cpu().numpy().tolist() == [[1, 4096], [1, 4096]] and (Kd[:, 0] == 0).all() and (Kd[:, 1] == -1).all()


def test_search_distinct_one_by_one_equals_the_cpu_oracle(torch_cuda, tmp_path):
    torch = torch_cuda
    from convdr_amd import search as S
    from convdr_amd.search import FlatIPIndex
    Q, blocks_ = DC.corpus()
    DC.write_blocks(str(tmp_path), blocks_)
    eD, eI = DC.exhaustive(Q, blocks_, DC.TOPN)
    tm = {}
    D, I = S.search_distinct_one_by_one(str(tmp_path), FlatIPIndex(DC.DIM), Q, DC.TOPN, timings=tm)
    assert D.dtype == np.float64 and I.dtype == np.int64 and tm["blocks"] == 3
    assert DC.same_bits(I, eI) and DC.same_bits(D, eD)
    assert I[0, 0] == 5000 and (I[0] == 5000).sum() == 1 and I[1, :2].tolist() == [5001, 5002]
    # through a key map on unique record offsets
    keys = np.concatenate([k for _, k in blocks_])
    starts = np.concatenate([[0], np.cumsum(DC.SIZES)])
    (tmp_path / "mapped").mkdir()
    DC.write_blocks(str(tmp_path / "mapped"), blocks_, [np.arange(starts[b], starts[b + 1], dtype=np.int64) for b in range(3)])
    D2, I2 = S.search_distinct_one_by_one(str(tmp_path / "mapped"), FlatIPIndex(DC.DIM), Q, DC.TOPN, key_map=keys)
    assert DC.same_bits(D2, eD) and DC.same_bits(keys[I2], eI)
    from convdr_amd._lib import ConvdrError
    with pytest.raises(ConvdrError, match="understated"):
        S.search_distinct_one_by_one(str(tmp_path), FlatIPIndex(DC.DIM), Q, DC.TOPN, rows_per_key=1)
