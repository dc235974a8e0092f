"""Judging a run on the device against the oracle of tests/judge_cases.py.

Bit for bit: labels, negatives, counts, num_rel, num_rel_ret, recip_rank, recall_c, P_c (the fp64 ones are one correctly rounded
division of two exact integers).  map and ndcg_cut_c: rtol 1e-9, atol 1e-12 -- at most 65,536 fp64 additions of non-negative
terms give a relative error below 65,536 * 2^-53 ~ 7e-12, plus a few ulp from log2; 1e-9 leaves two orders of magnitude and
is still far below any single term's share of the value, at least 1 / (65,536 * 17)."""
import numpy as np
import pytest
import torch

from convdr_amd import _lib, judge
from tests import judge_cases as JC
from tests.helpers import FILLS, fill_bytes

pytestmark = pytest.mark.gpu

WORKGROUP = 1024         # RUN_THREADS of csrc/run_judge.hpp: the workgroup of the measure and negative kernels ...
PIECE = 1024             # ... and the ranks they walk per step (one per thread)
LABEL_WORKGROUP = 256    # k_run_label
N_LIST = (1, 7, 64, 65, 100, LABEL_WORKGROUP - 1, LABEL_WORKGROUP, LABEL_WORKGROUP + 1, 1000, PIECE - 1, PIECE, PIECE + 1,
          2 * PIECE - 1, 2 * PIECE, 2 * PIECE + 1, 4096, 4097)
SHAPES = [(5, n) for n in N_LIST] + [(nq, n) for nq in (0, 1, 37) for n in (7, 100, PIECE + 1)] + [(2, 65536)]
RUNS = ("Z",) + FILLS    # the first two runs start from the same bytes: repeatability
EXACT = ("num_rel", "num_rel_ret", "recip_rank", "recall_", "P_")
RTOL, ATOL = 1e-9, 1e-12


def _device_case(nq, n):
    c = JC.case(nq, n)
    Kw, Iw = torch.from_numpy(c["K"]).cuda(), torch.from_numpy(c["I"]).cuda()
    q = judge.Qrels.from_dict(dict(enumerate(c["judged"])), range(nq), device="cuda")
    return c, Kw[:, :n], Iw[:, :n], n + JC.PITCH_EXTRA, q


def _buf(shape, dtype, fill, seed):
    return fill_bytes(torch.empty(shape, dtype=dtype, device="cuda"), fill, seed=seed)


def _check_measures(got, want, cols, what):
    assert got.shape == want.shape, what
    for j, name in enumerate(cols):
        if name.startswith(EXACT):
            assert JC.same_bits(got[:, j], want[:, j]), "%s: %s differs: %s vs %s" % (what, name, got[:, j], want[:, j])
        else:
            np.testing.assert_allclose(got[:, j], want[:, j], rtol=RTOL, atol=ATOL, err_msg="%s: %s" % (what, name))


@pytest.mark.parametrize("nq,n", SHAPES)
def test_kernels_match_the_oracle(nq, n):
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr
    c, K, I, ld, q = _device_case(nq, n)
    assert K.stride(0) == ld or nq <= 1
    cuts = c["cutoffs"]
    ccuts = (judge.C.c_int32 * len(cuts))(*cuts)
    cols = JC.columns(cuts)
    labels = None
    for j, f in enumerate(RUNS):
        out = _buf((nq, n), torch.int32, f, 11 + j)
        _lib.check(L.convdr_run_label(p(K), n, ld, nq, p(q.off), p(q.key), p(q.grade), q.nnz, p(out), st()), "convdr_run_label")
        assert JC.same_bits(out.cpu().numpy(), c["labels"]), "labels under fill %s" % f
        labels = out
    for lvl in (1, 2):
        first = None
        for j, f in enumerate(RUNS):
            out = _buf((nq, len(cols)), torch.float64, f, 21 + j)
            _lib.check(L.convdr_run_measures(p(labels), n, nq, p(q.off), p(q.grade), p(q.ideal), q.nnz, lvl, ccuts, len(cuts),
                                             p(out), st()), "convdr_run_measures")
            got = out.cpu().numpy()
            _check_measures(got, c["measures"][lvl], cols, "nq=%d n=%d rel_level=%d fill %s" % (nq, n, lvl, f))
            first = got if first is None else first
            assert JC.same_bits(got, first), "measures differ between two calls (fill %s)" % f
    for fill_to in JC.FILL_TO:
        w = max(n, fill_to)
        wk, wr, wc = c["negatives"][fill_to]
        for j, f in enumerate(RUNS):
            ok, orow = _buf((nq, w), torch.int64, f, 31 + j), _buf((nq, w), torch.int64, f, 41 + j)
            cnt = _buf((nq,), torch.int32, f, 51 + j)
            _lib.check(L.convdr_run_negatives(p(K), p(I), n, ld, nq, p(labels), p(q.off), p(q.grade), q.nnz, fill_to, p(ok),
                                              p(orow), p(cnt), st()), "convdr_run_negatives")
            what = "nq=%d n=%d fill_to=%d fill %s" % (nq, n, fill_to, f)
            assert JC.same_bits(cnt.cpu().numpy(), wc), "%s: counts %s vs %s" % (what, cnt.cpu().numpy(), wc)
            assert JC.same_bits(ok.cpu().numpy(), wk), "%s: keys" % what
            assert JC.same_bits(orow.cpu().numpy(), wr), "%s: rows" % what
        ok = _buf((nq, w), torch.int64, "R", 61)                 # without row ids
        cnt = _buf((nq,), torch.int32, "R", 62)
        _lib.check(L.convdr_run_negatives(p(K), None, n, ld, nq, p(labels), p(q.off), p(q.grade), q.nnz, fill_to, p(ok), None,
                                          p(cnt), st()), "convdr_run_negatives")
        assert JC.same_bits(ok.cpu().numpy(), wk) and JC.same_bits(cnt.cpu().numpy(), wc)


def test_hand_worked_case_on_the_device():
    K = torch.tensor([[5, 9, 2, 7, 3]], dtype=torch.int64, device="cuda")
    q = judge.Qrels.from_dict({0: {9: 2, 3: 1, 4: 3, 7: 0}}, [0], device="cuda")
    labels = judge.label_run(K, q)
    assert labels.cpu().tolist() == [[JC.UNJUDGED, 2, JC.UNJUDGED, 0, 1]]
    for lvl in (1, 2):
        m = judge.run_measures(labels, q, cutoffs=(1, 3, 9), rel_level=lvl)
        assert m.columns == JC.columns((1, 3, 9))
        want = np.asarray([JC.measures_of(labels.cpu().tolist()[0], {9: 2, 3: 1, 4: 3, 7: 0}, (1, 3, 9), lvl)])
        _check_measures(m.per_query.cpu().numpy(), want, m.columns, "hand case, rel_level %d" % lvl)
    for fill_to, want in ((3, [7, 5, 2, -1, -1]), (20, [7, 5, 2, 7] + [-1] * 16), (0, [7, -1, -1, -1, -1])):
        keys, rows, counts = judge.run_negatives(K, labels, q, fill_to=fill_to)
        assert rows is None and keys.cpu().tolist() == [want] and counts.cpu().tolist() == [sum(k >= 0 for k in want)]


@pytest.mark.parametrize("nq,n", [(5, 100), (37, PIECE + 1), (0, 7)])
def test_python_surface(nq, n):
    c, K, I, _, q = _device_case(nq, n)
    labels = judge.label_run(K, q)
    assert JC.same_bits(labels.cpu().numpy(), c["labels"])
    cols = JC.columns(c["cutoffs"])
    for lvl in (1, 2):
        m = judge.run_measures(labels, q, cutoffs=c["cutoffs"], rel_level=lvl)
        assert m.columns == cols and m.per_query.is_cuda
        want = c["measures"][lvl]
        _check_measures(m.per_query.cpu().numpy(), want, cols, "rel_level %d" % lvl)
        mean, judged = m.mean(), want[want[:, 0] > 0] if nq else want
        assert mean["num_q"] == len(judged)
        for j, name in enumerate(cols):
            np.testing.assert_allclose(mean[name], judged[:, j].mean() if len(judged) else 0.0, rtol=RTOL, atol=ATOL)
    for fill_to in JC.FILL_TO:
        wk, wr, wc = c["negatives"][fill_to]
        keys, rows, counts = judge.run_negatives(K, labels, q, fill_to=fill_to, rows=I)
        assert JC.same_bits(keys.cpu().numpy(), wk) and JC.same_bits(rows.cpu().numpy(), wr)
        assert JC.same_bits(counts.cpu().numpy(), wc)
        keys, rows, counts = judge.run_negatives(K.contiguous(), labels, q, fill_to=fill_to, rows=I)     # two pitches
        assert JC.same_bits(keys.cpu().numpy(), wk) and JC.same_bits(rows.cpu().numpy(), wr)


# ---- end to end: a resident index, rows that share keys -----------------------------------------------------------------
@pytest.fixture(scope="module")
def resident():
    from convdr_amd.search import FlatIPIndex
    rs = np.random.RandomState(5)
    P = rs.randn(2000, 64).astype(np.float32)
    Q = rs.randn(40, 64).astype(np.float32)
    key_map = []
    while len(key_map) < len(P):
        key_map += [len(key_map) + 7 * JC.HIGH] * int(rs.randint(1, 4))        # every key on 1 to 3 rows, all beyond bit 32
    key_map = np.asarray(key_map[:len(P)], np.int64)[rs.permutation(len(P))]
    idx = FlatIPIndex(64)
    idx.add(P)
    D, I = idx.search(Q, 200)
    judged = []
    for j in range(len(Q)):
        seen = key_map[I[j]]
        keys = np.unique(np.concatenate([seen[rs.permutation(200)[:30]], key_map[rs.randint(0, len(P), 10)]]))
        grades = rs.choice((-1, 0, 0, 0, 1, 2, 3), size=len(keys)) if j % 7 else np.zeros(len(keys), np.int64)
        judged.append({int(k): int(g) for k, g in zip(keys, grades)})
    q = judge.Qrels.from_dict(dict(enumerate(judged)), range(len(Q)), device="cuda")
    return idx, Q, key_map, D, I, judged, q


def test_judge_run_end_to_end(resident):
    from convdr_amd.search import distinct_topk
    idx, Q, key_map, D, I, judged, q = resident
    Dt, It = idx.search_tensors(Q, 200)
    cuts = (3, 10, 100)
    K, labels, m = judge.judge_run(Dt, It, q, key_map=torch.from_numpy(key_map).cuda(), cutoffs=cuts)
    _, _, Kw, counts = distinct_topk(D, I, 200, key_map)
    assert JC.same_bits(K.cpu().numpy(), Kw)
    assert 0 < counts[:, 0].min() and counts[:, 0].max() < 200          # rows did share keys: padding tails in every list
    lab = [JC.labels_of(Kw[j].tolist(), judged[j]) for j in range(len(Q))]
    assert JC.same_bits(labels.cpu().numpy(), np.asarray(lab, np.int32))
    want = np.asarray([JC.measures_of(lab[j], judged[j], cuts, 1) for j in range(len(Q))])
    _check_measures(m.per_query.cpu().numpy(), want, m.columns, "judge_run")
    assert 0 < m.mean()["num_q"] < len(Q) and m.mean()["recip_rank"] > 0
    K50, labels50, _ = judge.judge_run(Dt, It, q, key_map=torch.from_numpy(key_map).cuda(), topN=50)
    assert JC.same_bits(K50.cpu().numpy(), Kw[:, :50]) and JC.same_bits(labels50.cpu().numpy(), np.asarray(lab, np.int32)[:, :50])


def test_negatives_name_rows_of_the_index(resident):
    from convdr_amd.search import distinct_topk_device
    idx, Q, key_map, D, I, judged, q = resident
    Dt, It = idx.search_tensors(Q, 200)
    _, Io, Ko, _ = distinct_topk_device(Dt, It, 200, torch.from_numpy(key_map).cuda())
    labels = judge.label_run(Ko, q)
    keys, rows, counts = judge.run_negatives(Ko, labels, q, fill_to=20, rows=Io)
    Kh, Ih, cnt = Ko.cpu().numpy(), Io.cpu().numpy(), counts.cpu().numpy()
    assert (cnt > 0).any() and (cnt == 0).any()
    for j in range(len(Q)):
        wk, wr = JC.negatives_of(Kh[j].tolist(), judged[j], 20, Ih[j].tolist())
        assert cnt[j] == len(wk) and keys[j, :cnt[j]].cpu().tolist() == wk and rows[j, :cnt[j]].cpu().tolist() == wr
        assert bool((keys[j, cnt[j]:] == -1).all()) and bool((rows[j, cnt[j]:] == -1).all())
        if cnt[j]:
            assert key_map[wr].tolist() == wk
            embs = idx.rows_tensors(rows[j, :cnt[j]])
            assert JC.same_bits(embs.cpu().numpy(), idx.reconstruct_batch(np.asarray(wr, np.int64)))
