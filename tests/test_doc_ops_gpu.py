"""Documents by id on the device: convdr_keys_rows_count / convdr_keys_rows_fill against the numpy oracle of tests/doc_cases.py,
and FlatIPIndex.rows_all / score_ids / search_docs / reconstruct_docs / upsert_docs against entries that other tests pin
(score_rows, search, distinct_topk).  Every comparison is exact: integers, or bits."""
import functools

import numpy as np
import pytest
import torch

from convdr_amd import _lib
from convdr_amd import search as S
from tests import doc_cases as DC
from tests import key_cases as K
from tests.helpers import fill_bytes

pytestmark = pytest.mark.gpu

NS = (0, 1, 255, 256, 257, 1000, 20000)
MS = (0, 1, 2, 1000)
GUARD = 8                                                # entries behind every output that must stay as they were
STORAGES = ("fp32", "fp16")
ST_ROWS_CAP = 16                                         # bit 4 of the head's status word: total > rows_cap


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()         # (a copy: the cases are read-only arrays)


def filled(shape, dtype, fill, seed):
    return fill_bytes(torch.empty(shape, dtype=dtype, device="cuda"), fill, seed)


def run_csr(col_d, lst_d, n, m, cap, fill, seed):
    """build, count, fill with a list of `cap` entries; the workspace and every output pre-filled; name -> numpy"""
    L, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr
    need = int(L.convdr_keys_rows_workspace_bytes(m, cap))
    assert need > 0
    ws = filled(need, torch.uint8, fill, seed)
    status = filled(1, torch.int32, fill, seed + 1)
    start = filled(m + GUARD, torch.int64, fill, seed + 2)
    count = filled(m + GUARD, torch.int32, fill, seed + 3)
    dup = filled(m + GUARD, torch.int32, fill, seed + 4)
    total = filled(1 + GUARD, torch.int64, fill, seed + 5)
    rows = filled(cap + GUARD, torch.int64, fill, seed + 6)
    before = rows.clone()
    guard = [t[k:].clone() for t, k in ((start, m), (count, m), (dup, m), (total, 1))]
    _lib.check(L.convdr_keyset_build(ptr(lst_d), m, ptr(ws), need, ptr(status), st()), "convdr_keyset_build")
    _lib.check(L.convdr_keys_rows_count(ptr(col_d), n, ptr(ws), need, ptr(lst_d), m, ptr(start), ptr(count), ptr(dup), ptr(total),
                                        st()), "convdr_keys_rows_count")
    _lib.check(L.convdr_keys_rows_fill(ptr(col_d), n, ptr(ws), need, m, ptr(rows), cap, st()), "convdr_keys_rows_fill")
    for (t, k), g in zip(((start, m), (count, m), (dup, m), (total, 1)), guard):
        assert torch.equal(t[k:], g)
    tot = int(total[0].item())
    written = tot if tot <= cap else 0                     # (a list that is too short is not written at all)
    assert torch.equal(rows[written:], before[written:])
    return {"status": status.cpu().numpy(), "head": ws[:8].view(torch.int32).cpu().numpy(), "start": start[:m].cpu().numpy(),
            "count": count[:m].cpu().numpy(), "dup": dup[:m].cpu().numpy(), "total": total[:1].cpu().numpy(),
            "rows": rows[:cap].cpu().numpy()}


# ---- the kernels against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", DC.FAMILIES)
def test_the_csr_equals_the_oracle_at_every_size_whatever_the_memory_held(family):
    for n in NS:
        for m in MS:
            what = "%s n=%d m=%d" % (family, n, m)
            col, lst = DC.case(family, n, m)
            col_d, lst_d = dev(col), dev(lst)
            start, count, rows, dup = DC.rows_all(col, lst)
            cap = len(rows) if (n + m) % 2 else n                  # an exact list and the longest a column can need
            runs = [run_csr(col_d, lst_d, n, m, cap, fill, seed) for fill, seed in (("N", 0), ("R", 11 + n + m))]
            got = runs[0]
            for name in got:
                other = runs[1][name]
                if name == "rows":                                 # (behind total the list keeps what the fill put there)
                    got[name], other = got[name][:len(rows)], other[:len(rows)]
                assert got[name].tobytes() == other.tobytes(), "%s: %s differs between the two runs" % (what, name)
            slots = 64
            while slots < 2 * m:
                slots *= 2
            assert got["status"].tolist() == [0] and got["head"][0] == 0 and (1 << int(got["head"][1])) == slots, what
            assert got["total"].tolist() == [len(rows)], what
            assert got["count"].dtype == np.int32 and np.array_equal(got["count"], count), what
            assert got["dup"].dtype == np.int32 and np.array_equal(got["dup"], dup), what
            assert got["start"].dtype == np.int64 and np.array_equal(got["start"][count > 0], start[count > 0]), what
            assert np.array_equal(got["start"][dup], got["start"]), "%s: a repeat does not share its first occurrence's segment" % what
            assert got["rows"].dtype == np.int64 and np.array_equal(got["rows"], rows), what
            for j in range(0, m, max(1, m // 50)):                 # (the oracle's own words, for a sample of the list)
                seg = got["rows"][got["start"][j]:got["start"][j] + got["count"][j]]
                assert np.array_equal(seg, np.nonzero(col == lst[j])[0]), "%s: position %d" % (what, j)


def test_a_list_too_short_for_the_rows_is_left_alone_and_flagged_and_a_second_fill_needs_no_second_count():
    n, m = 20000, 1000
    col, lst = DC.case("interleaved", n, m)
    col_d, lst_d = dev(col), dev(lst)
    _, _, rows, _ = DC.rows_all(col, lst)
    tot = len(rows)
    assert tot > 5000
    for cap in (tot - 1, 0, 5000):
        got = run_csr(col_d, lst_d, n, m, cap, "N", 3)             # (run_csr holds the whole list against its old bytes)
        assert got["total"].tolist() == [tot] and got["head"][0] == ST_ROWS_CAP, cap
    L, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr
    need = int(L.convdr_keys_rows_workspace_bytes(m, tot))
    ws, status = filled(need, torch.uint8, "R", 5), filled(1, torch.int32, "N", 0)
    start, count, total = filled(m, torch.int64, "N", 0), filled(m, torch.int32, "N", 0), filled(1, torch.int64, "N", 0)
    _lib.check(L.convdr_keyset_build(ptr(lst_d), m, ptr(ws), need, ptr(status), st()), "build")
    _lib.check(L.convdr_keys_rows_count(ptr(col_d), n, ptr(ws), need, ptr(lst_d), m, ptr(start), ptr(count), None, ptr(total), st()),
               "count")                                             # (dup_of is optional)
    for fill in ("N", "R"):
        out = filled(tot, torch.int64, fill, 9)
        _lib.check(L.convdr_keys_rows_fill(ptr(col_d), n, ptr(ws), need, m, ptr(out), tot, st()), "fill")
        assert np.array_equal(out.cpu().numpy(), rows) and int(ws[:4].view(torch.int32).item()) == 0


def test_the_reserved_key_sets_a_status_bit_and_is_on_no_row():
    n, m = 300, 40
    col, lst = (a.copy() for a in K.case("chunks", n, m))
    col[[0, 299]] = K.I64_MIN
    lst[[3, 17]] = K.I64_MIN
    start, count, rows, dup = DC.rows_all(col, lst)
    got = run_csr(dev(col), dev(lst), n, m, n, "N", 7)
    assert got["status"].tolist() == [S.KEY_ST_LIST] and got["head"][0] == S.KEY_ST_COLUMN
    assert np.array_equal(got["count"], count) and np.array_equal(got["dup"], dup) and got["total"].tolist() == [len(rows)]
    assert got["start"][[3, 17]].tolist() == [0, 0] and got["count"][[3, 17]].tolist() == [0, 0] and got["dup"][[3, 17]].tolist() == [3, 17]
    assert np.array_equal(got["rows"][:len(rows)], rows)


def test_a_workspace_whose_set_is_not_the_lists_is_refused_on_the_device():
    n, m = 600, 1000
    col, lst = DC.case("chunks", n, m)
    col_d, lst_d = dev(col), dev(lst)
    L, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr
    need = int(L.convdr_keys_rows_workspace_bytes(m, n))
    ws, status = filled(need, torch.uint8, "N", 0), filled(1, torch.int32, "N", 0)
    _lib.check(L.convdr_keyset_build(ptr(lst_d[:10]), 10, ptr(ws), need, ptr(status), st()), "build")     # a set of 64 slots
    start, count, total = filled(m, torch.int64, "N", 0), filled(m, torch.int32, "N", 0), filled(1, torch.int64, "N", 0)
    rows = filled(n, torch.int64, "N", 0)
    _lib.check(L.convdr_keys_rows_count(ptr(col_d), n, ptr(ws), need, ptr(lst_d), m, ptr(start), ptr(count), None, ptr(total), st()), "count")
    _lib.check(L.convdr_keys_rows_fill(ptr(col_d), n, ptr(ws), need, m, ptr(rows), n, st()), "fill")
    assert int(ws[:4].view(torch.int32).item()) & S.KEY_ST_NOSET
    assert total.tolist() == [0] and not start.any() and not count.any() and bool((rows == -1).all())


# ---- the index ----------------------------------------------------------------------------------------------------------------
def index(storage, X, ids, precision="auto"):
    idx = S.FlatIPIndex(X.shape[1], storage=storage, precision=precision, prepin=False)
    idx.compact_window_rows = 512
    cut = X.shape[0] // 3
    X = X.half() if storage == "fp16" else X
    idx.add(X[:cut].clone(), ids=ids[:cut])
    idx.add(X[cut:].clone(), ids=dev(ids[cut:]))
    return idx


def test_rows_all_of_the_index_equals_the_oracle_and_refuses_the_reserved_id():
    n = 20000
    col, lst = DC.case("interleaved", n, 1000)
    X = torch.randn((n, 64), generator=torch.Generator(device="cuda").manual_seed(1), device="cuda")
    idx = index("fp16", X, col)
    want = DC.rows_all(col, lst)
    for arg in (lst, dev(lst)):
        a, b = idx.rows_all(arg), idx.rows_all(arg)
        assert [t.dtype for t in a] == [torch.int64, torch.int32, torch.int64] and all(t.is_cuda for t in a)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        start, count, rows = (t.cpu().numpy() for t in a)
        assert np.array_equal(count, want[1]) and np.array_equal(rows, want[2]) and rows.shape == (len(want[2]),)
        assert np.array_equal(start[count > 0], want[0][count > 0])
    start, count, rows = idx.rows_all(np.zeros(0, np.int64))
    assert start.shape == count.shape == rows.shape == (0,)
    bad = lst.copy()
    bad[5] = K.I64_MIN
    with pytest.raises(ValueError, match="reserved"):
        idx.rows_all(dev(bad))
    with pytest.raises(ValueError, match="reserved"):
        idx.rows_all(bad)
    # after a removal a document's rows are no run of the column: rows_of's (first row, count) cannot name them, the CSR does
    idx.remove_ids(lst[::3])
    col2 = idx.ids.cpu().numpy()
    start, count, rows = (t.cpu().numpy() for t in idx.rows_all(lst))
    want = DC.rows_all(col2, lst)
    assert np.array_equal(count, want[1]) and np.array_equal(rows, want[2]) and count[::3].max() == 0


SCORE_N = 20000


@functools.lru_cache(maxsize=None)
def score_corpus(d_in):
    """(X device fp32 [SCORE_N, d_in] of exact halves with every entry positive, ids = the interleaved column, Q device fp32
    [5, d_in] whose query 1 is all negative -- every score of it is --, the id of a document of three IDENTICAL rows)"""
    g = torch.Generator(device="cuda").manual_seed(100 + d_in)
    X = (torch.rand((SCORE_N, d_in), generator=g, device="cuda") + 0.25).half().float()
    Q = torch.randn((5, d_in), generator=g, device="cuda")
    Q[1] = -Q[1].abs() - 0.1
    col = DC.interleaved(SCORE_N)
    ids, reps = np.unique(col, return_counts=True)
    twin = int(ids[reps == 3][40])
    r = np.nonzero(col == twin)[0]
    X[r[1]] = X[r[0]]
    X[r[2]] = X[r[0]]
    return X, col, Q, twin


def score_lists(col, twin, nq, m, seed):
    """int64 [nq, m] (or [nq] for m = 1): documents of 1, 3 and 5,000 rows, the twin document, ids on no row, INT64_MIN"""
    rs = np.random.RandomState(seed)
    ids, reps = np.unique(col, return_counts=True)
    special = np.array([DC.BIG_ID, twin, K.I64_MIN, 424242424242, -1], np.int64)
    if m == 1:
        return special[:nq].copy()
    out = np.empty((nq, m), np.int64)
    for q in range(nq):
        row = np.concatenate([special, rs.choice(ids[reps == 3], 15), rs.choice(ids[reps == 1], 10),
                              31337 + 7 * np.arange(5, dtype=np.int64), [K.I64_MIN] * 5])[:m]
        out[q] = row[rs.permutation(m)]
    return out


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("d_in", (64, 70, 768))
def test_score_ids_equals_the_max_of_score_rows_over_the_documents_rows(storage, d_in):
    """D against the max of score_rows' fp32 scores; R against the first maximum of its fp64 scores (two rows whose fp64
    scores differ may share an fp32 one: the rule speaks of the fp64 scores), and D[pair] == score_rows(R[pair]) on top."""
    X, col, Q, twin = score_corpus(d_in)
    idx = index(storage, X, col)
    every = torch.arange(SCORE_N, device="cuda")[None, :].expand(5, SCORE_N).contiguous()
    Dr, Xr = (t.cpu().numpy() for t in idx.score_rows_tensors(Q, every))          # every (query, row) score, once
    assert (Dr[1] < 0).all() and Dr.dtype == np.float32 and Xr.dtype == np.float64
    for nq in (1, 5):
        for m in (1, 40):
            what = "%s d=%d nq=%d m=%d" % (storage, d_in, nq, m)
            ids = score_lists(col, twin, nq, m, d_in + nq + m)
            q0 = 1 if nq == 1 else 0                               # (a single query: the all-negative one)
            Qs = Q[q0:q0 + nq].contiguous()
            D, R = idx.score_ids_tensors(Qs, dev(ids))
            assert D.dtype == torch.float32 and R.dtype == torch.int64 and D.shape == R.shape == ids.shape and D.is_cuda, what
            Dn, Rn = idx.score_ids(Qs.cpu().numpy(), ids)
            assert Dn.tobytes() == D.cpu().numpy().tobytes() and np.array_equal(Rn, R.cpu().numpy()), what
            seen = set()
            for q in range(nq):
                for j in range(m):
                    key = int(ids.reshape(nq, m)[q, j])
                    rows = DC.rows_of(col, key)
                    d, r = Dn.reshape(nq, m)[q, j], int(Rn.reshape(nq, m)[q, j])
                    if not len(rows):
                        assert d == DC.PAD_SCORE and r == -1, "%s: (%d, %d) id %d" % (what, q, j, key)
                        continue
                    best, row = DC.maxp(Xr[q0 + q, rows], rows)
                    assert r == row and d == Dr[q0 + q, rows].max() == Dr[q0 + q, r], "%s: (%d, %d) id %d" % (what, q, j, key)
                    seen.add(len(rows))
                    if key == twin:
                        assert r == rows[0] and len(set(Xr[q0 + q, rows].tolist())) == 1, what
            assert seen >= ({1, 3, 5000} if m > 1 else {3, 5000} if nq > 1 else {5000}), what
    # an index without rows of the ids, and no rows at all
    D, R = idx.score_ids(Q.cpu().numpy()[:2], np.array([[5, K.I64_MIN], [6, 7]]))
    assert (D == DC.PAD_SCORE).all() and (R == -1).all()
    D, R = idx.score_ids_tensors(Q[:0], np.zeros((0, 3), np.int64))
    assert D.shape == R.shape == (0, 3)


SEARCH_N, SEARCH_D = 3001, 64


@functools.lru_cache(maxsize=None)
def search_corpus():
    g = torch.Generator(device="cuda").manual_seed(77)
    X = torch.randn((SEARCH_N, SEARCH_D), generator=g, device="cuda").half().float()
    Q = torch.randn((6, SEARCH_D), generator=g, device="cuda")
    return X, DC.chunked_ids(SEARCH_N), Q


def docs_oracle(idx, Q, k, ids, mask=None):
    """distinct_topk of the FULL search order (of the allowed rows) with keys = the id column: (D, rows, ids, counts)"""
    D, I = idx.search(Q.cpu().numpy(), idx.ntotal, allowed=mask)
    return S.distinct_topk(D, I, k, key_map=ids)


def assert_docs(got, want, what):
    D, ids, rows, _ = (t.cpu().numpy() for t in got)
    assert D.tobytes() == want[0].tobytes() and np.array_equal(rows, want[1]) and np.array_equal(ids, want[2]), what


@pytest.mark.parametrize("storage", STORAGES)
def test_search_docs_equals_distinct_topk_of_the_full_order_with_and_without_a_filter(storage):
    X, ids, Q = search_corpus()
    idx = index(storage, X, ids)
    rs = np.random.RandomState(5)
    docs = np.unique(ids)
    gone = np.isin(ids, rs.choice(docs, len(docs) // 4, replace=False))          # every row of a quarter of the documents ...
    mask = ~gone & ~((rs.rand(SEARCH_N) < 0.3) & np.isin(ids, docs[::3]))        # ... and some chunk rows of every third
    few = np.isin(ids, docs[:37])                                                # fewer documents than k = 200
    assert 0 < mask.sum() < SEARCH_N and len(np.unique(ids[few])) == 37
    for k in (1, 10, 200):
        want = docs_oracle(idx, Q, k, ids)
        got = idx.search_docs(Q, k)
        assert [t.dtype for t in got] == [torch.float32, torch.int64, torch.int64, torch.int32]
        assert_docs(got, want, "%s k=%d" % (storage, k))
        assert (want[1] >= 0).all() and (want[3][:, 0] == len(docs)).all()       # (the oracle walked every row: no padding)
        # the scores and best rows of the documents it returns, by id
        D2, R2 = idx.score_ids_tensors(Q, got[1])
        assert torch.equal(D2, got[0]) and torch.equal(R2, got[2]), "%s k=%d" % (storage, k)
        # the side-table form returns what it returned: the column is just a key vector
        side = idx.search_distinct(Q, k, dev(ids))
        assert all(torch.equal(a, b) for a, b in zip((got[0], got[2], got[1]), side[:3]))
        for name, mk in (("mask", mask), ("few", few)):
            f = idx.row_filter(mk)
            got = idx.search_docs(Q, k, allowed=f)
            assert_docs(got, docs_oracle(idx, Q, k, ids, mk), "%s k=%d %s" % (storage, k, name))
            rows = got[2].cpu().numpy()
            assert mk[rows[rows >= 0]].all()
            if name == "few" and k == 200:                       # certified and padded: it does not raise
                c = got[3].cpu().numpy()
                assert (c[:, 0] == 37).all() and (rows[:, 37:] == -1).all() and (got[1].cpu().numpy()[:, 37:] == -1).all()
                assert (got[0].cpu().numpy()[:, 37:] == DC.PAD_SCORE).all()
    none = idx.search_docs(Q, 5, allowed=np.zeros(SEARCH_N, bool))
    assert (none[1] == -1).all() and (none[2] == -1).all() and not none[3].any()


def model_upsert(X, col, lst, counts, E):
    """the expected corpus after upsert_docs, in row order: (rows fp32 [n', d], ids [n'], (in place, replaced, added))"""
    X, keep, off = X.copy(), np.ones(len(col), bool), np.cumsum(counts) - counts
    tail_x, tail_id, kinds = [], [], [0, 0, 0]
    for j, (key, c) in enumerate(zip(lst.tolist(), counts.tolist())):
        rows, new = DC.rows_of(col, key), E[off[j]:off[j] + c]
        if len(rows) == c:
            X[rows] = new
            kinds[0] += 1
            continue
        keep[rows] = False
        kinds[1 if len(rows) else 2] += 1
        tail_x.append(new)
        tail_id += [key] * c
    return np.concatenate([X[keep]] + tail_x), np.concatenate([col[keep], np.array(tail_id, np.int64)]), tuple(kinds)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("d_in", (64, 70))
def test_upsert_docs_and_reconstruct_docs_rebuild_the_corpus_document_by_document(storage, d_in):
    n = 1317
    g = torch.Generator(device="cuda").manual_seed(9 + d_in)
    X = torch.randn((n, d_in), generator=g, device="cuda").half().float()
    E = torch.randn((400, d_in), generator=g, device="cuda").half().float()
    Q = torch.randn((6, d_in), generator=g, device="cuda")
    col = DC.chunked_ids(n)
    idx = index(storage, X, col)
    docs, reps = np.unique(col, return_counts=True)
    rs = np.random.RandomState(d_in)
    same = rs.choice(docs, 30, replace=False)
    rest = np.setdiff1d(docs, same)
    more, fewer = rest[reps[np.isin(docs, rest)] <= 3][:12], rest[reps[np.isin(docs, rest)] >= 4][:12]
    fresh = 900_000_000 + 13 * np.arange(10, dtype=np.int64)
    lst = np.concatenate([same, more, fewer, fresh])
    was = {int(k): int(c) for k, c in zip(docs, reps)}
    counts = np.concatenate([[was[int(k)] for k in same], [was[int(k)] + 2 for k in more], [was[int(k)] - 1 for k in fewer],
                             rs.randint(1, 5, size=10)]).astype(np.int64)
    order = rs.permutation(len(lst))
    lst, counts = lst[order], counts[order]
    emb = E[:int(counts.sum())].contiguous()
    untouched = np.setdiff1d(docs, lst)
    before = idx.reconstruct_docs(untouched)
    want_x, want_ids, kinds = model_upsert(X.cpu().numpy(), col, lst, counts, emb.cpu().numpy())
    assert kinds == (30, 24, 10)
    assert idx.upsert_docs(dev(lst), counts, emb) == kinds
    assert idx.ntotal == len(want_ids) and np.array_equal(idx.ids.cpu().numpy(), want_ids)
    assert idx.reconstruct_n(0, idx.ntotal).tobytes() == want_x.tobytes()
    # document by document: id -> the multiset of its rows
    every = np.unique(want_ids)
    start, count, got = idx.reconstruct_docs(every)
    assert got.shape == (len(want_ids), d_in) and got.dtype == np.float32
    for j, key in enumerate(every.tolist()):
        mine, theirs = got[start[j]:start[j] + count[j]], want_x[want_ids == key]
        assert sorted(r.tobytes() for r in mine) == sorted(r.tobytes() for r in theirs), key
    off = np.cumsum(counts) - counts
    for j, key in enumerate(lst.tolist()):                        # the listed documents hold exactly their new rows
        assert sorted(r.tobytes() for r in got[start[np.searchsorted(every, key)]:][:counts[j]]) == \
            sorted(r.tobytes() for r in emb.cpu().numpy()[off[j]:off[j] + counts[j]]), key
    after = idx.reconstruct_docs(untouched)
    assert np.array_equal(before[1], after[1]) and before[2].tobytes() == after[2].tobytes()
    s2, c2, _ = idx.reconstruct_docs(np.array([lst[0], 5, lst[0]]))
    assert c2.tolist() == [counts[0], 0, counts[0]] and s2[0] == s2[2]
    # the rebuilt corpus searches like an index built from it
    fresh_idx = index(storage, torch.from_numpy(want_x).cuda(), want_ids)
    for k in (1, 10):
        want = docs_oracle(fresh_idx, Q, k, want_ids)
        assert_docs(idx.search_docs(Q, k), want, "%s d=%d k=%d" % (storage, d_in, k))
    if storage == "fp16":
        assert idx.update_flags() == 0

    # refused before anything is written: a repeated list id; counts / emb that do not fit
    def state():
        return idx.ntotal, idx.ids.clone(), idx.reconstruct_n(0, idx.ntotal).tobytes(), idx._max_norm.clone()

    def unchanged(s):
        t = state()
        return t[0] == s[0] and torch.equal(t[1], s[1]) and t[2] == s[2] and torch.equal(t[3], s[3])
    s = state()
    with pytest.raises(ValueError, match="repeats an id"):
        idx.upsert_docs(np.array([lst[0], 123456, lst[0]]), np.array([1, 2, 1]), E[:4].contiguous())
    assert unchanged(s)
    for ids_, counts_, emb_ in ((lst[:2], np.array([1, 2]), E[:4].contiguous()), (lst[:2], np.array([0, 3]), E[:3].contiguous()),
                                (lst[:2], np.array([1, 2]), E[:3].cpu()), (lst[:2], np.array([1, 2]), E[:3].double())):
        with pytest.raises(ValueError, match="upsert_docs"):
            idx.upsert_docs(ids_, counts_, emb_)
        assert unchanged(s)
    with pytest.raises(ValueError, match="reserved"):
        idx.upsert_docs(dev(np.array([lst[0], K.I64_MIN])), np.array([1, 1]), E[:2].contiguous())
    assert unchanged(s)
