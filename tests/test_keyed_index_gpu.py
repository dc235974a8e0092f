"""Row ids on the device: the convdr_keyset_* / convdr_keys_* / convdr_ip_compact_ids entries against the numpy oracle of
tests/key_cases.py, and FlatIPIndex.add(ids=) / search_ids / remove_ids / id_filter / rows_of / reconstruct_ids / upsert against
the same index driven in row numbers.  Every comparison is exact: integers, or bits."""
import functools

import numpy as np
import pytest
import torch

from convdr_amd import _lib
from convdr_amd import search as S
from tests import key_cases as K
from tests.helpers import fill_bytes

pytestmark = pytest.mark.gpu

NS = (0, 1, 31, 32, 33, 255, 256, 257, 1000, 70001)
MS = (0, 1, 2, 32, 33, 64, 65, 1000, 5000)               # slot counts 64 .. 16,384: both sides of 64, 128 and 2,048
GUARD = 8                                                # entries behind every output that must stay as they were
CONFIGS = (("fp32", "auto"), ("fp32", "bf16"), ("fp32", "fp16x3"), ("fp16", "auto"))
SHAPES = ((1317, 64), (257, 768), (5000, 100))           # (n, d_in); 100 is padded to 128 columns


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()         # (a copy: the cases are read-only arrays)


def words_of(n):
    return (n + 255) // 256 * 8


def packed(mask):
    """pack_row_mask of a numpy mask, as numpy int32 words"""
    return S.pack_row_mask(torch.as_tensor(np.ascontiguousarray(mask))).numpy()


def filled(shape, dtype, fill, seed):
    return fill_bytes(torch.empty(shape, dtype=dtype, device="cuda"), fill, seed)


def build_set(lst_d, m, fill, seed):
    L = _lib.lib()
    need = int(L.convdr_keyset_workspace_bytes(m))
    assert need > 0
    ws = filled(need, torch.uint8, fill, seed)
    status = filled(1, torch.int32, fill, seed + 1)
    _lib.check(L.convdr_keyset_build(_lib.ptr(lst_d), m, _lib.ptr(ws), need, _lib.ptr(status), _lib.stream_ptr()), "convdr_keyset_build")
    return ws, status


def member(ws, col_d, n, invert, fill, seed):
    words = words_of(n)
    bits = filled(words + GUARD, torch.int32, fill, seed + 2)
    counts = filled(2 + GUARD, torch.int64, fill, seed + 3)
    guard = (bits[words:].clone(), counts[2:].clone())
    _lib.check(_lib.lib().convdr_keys_member(_lib.ptr(col_d), n, _lib.ptr(ws), ws.numel(), invert, _lib.ptr(bits), words,
                                             _lib.ptr(counts), _lib.stream_ptr()), "convdr_keys_member")
    assert torch.equal(bits[words:], guard[0]) and torch.equal(counts[2:], guard[1])
    return bits[:words].cpu().numpy(), counts[:2].cpu().numpy(), ws[:8].view(torch.int32).cpu().numpy()


def locate(ws, col_d, n, lst_d, m, fill, seed):
    first = filled(m + GUARD, torch.int64, fill, seed + 4)
    count = filled(m + GUARD, torch.int32, fill, seed + 5)
    dup = filled(m + GUARD, torch.int32, fill, seed + 6)
    guard = [t[m:].clone() for t in (first, count, dup)]
    _lib.check(_lib.lib().convdr_keys_locate(_lib.ptr(col_d), n, _lib.ptr(ws), ws.numel(), _lib.ptr(lst_d), m, _lib.ptr(first),
                                             _lib.ptr(count), _lib.ptr(dup), _lib.stream_ptr()), "convdr_keys_locate")
    for t, g in zip((first, count, dup), guard):
        assert torch.equal(t[m:], g)
    return first[:m].cpu().numpy(), count[:m].cpu().numpy(), dup[:m].cpu().numpy(), ws[:8].view(torch.int32).cpu().numpy()


def run_entries(col_d, lst_d, n, m, fill, seed):
    """build, member (both values of invert), locate, with the workspace and every output pre-filled; name -> numpy"""
    ws, status = build_set(lst_d, m, fill, seed)
    out = {"status": status.cpu().numpy()}
    for invert in (0, 1):
        out["bits%d" % invert], out["counts%d" % invert], out["head%d" % invert] = member(ws, col_d, n, invert, fill, seed)
    out["first"], out["count"], out["dup"], out["head2"] = locate(ws, col_d, n, lst_d, m, fill, seed)
    return out


# ---- the kernels against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", K.FAMILIES)
def test_member_and_locate_equal_the_oracle_at_every_size_whatever_the_memory_held(family):
    for n in NS:
        for m in MS:
            what = "%s n=%d m=%d" % (family, n, m)
            col, lst = K.case(family, n, m)
            col_d, lst_d = dev(col), dev(lst)
            runs = [run_entries(col_d, lst_d, n, m, fill, seed) for fill, seed in (("N", 0), ("R", 11 + n + m))]
            for name in runs[0]:
                assert runs[0][name].tobytes() == runs[1][name].tobytes(), "%s: %s differs between the two runs" % (what, name)
            got = runs[0]
            isin, miss = K.member(col, lst), K.missing(col, lst)
            slots = 64
            while slots < 2 * m:
                slots *= 2
            assert got["status"].tolist() == [0], what
            for name in ("head0", "head1", "head2"):
                assert got[name][0] == 0 and (1 << int(got[name][1])) == slots, "%s: %s %s" % (what, name, got[name][:2])
            assert np.array_equal(got["bits0"], packed(isin)), what
            assert np.array_equal(got["bits1"], packed(~isin)), what
            assert got["counts0"].tolist() == [int(isin.sum()), miss], what
            assert got["counts1"].tolist() == [n - int(isin.sum()), miss], what
            first, count, dup = K.locate(col, lst)
            assert got["first"].dtype == np.int64 and np.array_equal(got["first"], first), what
            assert got["count"].dtype == np.int32 and np.array_equal(got["count"], count), what
            assert got["dup"].dtype == np.int32 and np.array_equal(got["dup"], dup), what


def test_one_build_serves_many_row_passes_and_dup_of_is_optional():
    n, m = 1000, 65
    col, lst = K.case("chunks", n, m)
    col_d, lst_d = dev(col), dev(lst)
    ws, _ = build_set(lst_d, m, "R", 1)
    a = member(ws, col_d, n, 0, "N", 2)
    loc = locate(ws, col_d, n, lst_d, m, "N", 3)
    b = member(ws, col_d, n, 0, "R", 4)
    loc2 = locate(ws, col_d, n, lst_d, m, "R", 5)
    for x, y in zip(a + loc, b + loc2):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal(a[0], packed(K.member(col, lst))) and np.array_equal(loc[1], K.locate(col, lst)[1])
    first = filled(m, torch.int64, "N", 0)
    count = filled(m, torch.int32, "N", 0)
    _lib.check(_lib.lib().convdr_keys_locate(_lib.ptr(col_d), n, _lib.ptr(ws), ws.numel(), _lib.ptr(lst_d), m, _lib.ptr(first),
                                             _lib.ptr(count), None, _lib.stream_ptr()), "convdr_keys_locate")
    assert np.array_equal(first.cpu().numpy(), loc[0]) and np.array_equal(count.cpu().numpy(), loc[1])


def test_the_reserved_key_sets_a_status_bit_and_never_hits():
    n, m = 300, 40
    col, lst = (a.copy() for a in K.case("random", n, m))
    col[[0, 299]] = K.I64_MIN
    lst[[3, 17]] = K.I64_MIN
    col_d, lst_d = dev(col), dev(lst)
    ws, status = build_set(lst_d, m, "R", 7)
    assert status.cpu().tolist() == [S.KEY_ST_LIST]
    legal = np.isin(col, lst[lst != K.I64_MIN]) & (col != K.I64_MIN)
    bits, counts, head = member(ws, col_d, n, 0, "N", 8)
    assert head[0] == S.KEY_ST_COLUMN and np.array_equal(bits, packed(legal)) and counts[0] == legal.sum()
    bits, counts, head = member(ws, col_d, n, 1, "N", 9)
    assert head[0] == S.KEY_ST_COLUMN and np.array_equal(bits, packed(~legal)) and counts[0] == n - legal.sum()
    first, count, dup, head = locate(ws, col_d, n, lst_d, m, "N", 10)
    assert head[0] == S.KEY_ST_COLUMN and first[3] == -1 and count[3] == 0 and dup[3] == 3 and dup[17] == 17
    # a clean column after a flagged one: the row pass resets its status word
    clean = dev(K.case("random", n, m)[0])
    assert member(ws, clean, n, 0, "N", 11)[2][0] == 0


def test_a_workspace_without_a_set_is_refused_on_the_device_and_nothing_else_is_touched():
    """the row passes take the slot count from the head: a head that names none -- garbage, or a set larger than the bytes
    they were given -- must not send them past the workspace"""
    n, m = 600, 5000
    col, lst = K.case("consecutive", n, m)
    col_d, lst_d = dev(col), dev(lst)
    for case in ("garbage", "larger than the bytes given"):
        if case == "garbage":
            ws = filled(int(_lib.lib().convdr_keyset_workspace_bytes(m)), torch.uint8, "N", 0)
            given = ws.numel()
        else:
            ws, _ = build_set(lst_d, m, "R", 3)
            given = int(_lib.lib().convdr_keyset_workspace_bytes(100))
        before = ws[256:].clone()
        bits = filled(words_of(n), torch.int32, "N", 1)
        counts = filled(2, torch.int64, "N", 2)
        _lib.check(_lib.lib().convdr_keys_member(_lib.ptr(col_d), n, _lib.ptr(ws), given, 0, _lib.ptr(bits), bits.numel(),
                                                 _lib.ptr(counts), _lib.stream_ptr()), "convdr_keys_member")
        assert int(ws[:4].view(torch.int32).item()) == S.KEY_ST_NOSET, case
        assert not bits.any() and counts.tolist() == [0, 0] and torch.equal(ws[256:], before), case


# ---- the id column's compaction ---------------------------------------------------------------------------------------------
def keep_patterns(n, seed=0):
    rs = np.random.RandomState(seed + n)
    p = {"all": np.ones(n, bool), "none": np.zeros(n, bool)}
    for name, r in (("first row", 0), ("last row", n - 1)):
        k = np.zeros(n, bool); k[r] = True
        p["only the %s kept" % name], p["only the %s removed" % name] = k, ~k
    k = np.zeros(n, bool)
    for t in range((n + 255) // 256):
        k[min(n - 1, t * 256 + (t * 37 + 5) % 256)] = True
    p["one row per tile"] = k
    k = np.zeros(n, bool); k[::2] = True
    p["alternating"] = k
    k = np.ones(n, bool); k[[r for r in (31, 32, 255, 256) if r < n]] = False
    p["word and tile edges removed"], p["word and tile edges kept"] = k, ~k
    p["random half"], p["random 1 %"] = rs.rand(n) < 0.5, rs.rand(n) >= 0.01
    return p


@pytest.mark.parametrize("n", (257, 1317, 5000))
def test_compact_ids_equals_the_masked_column(n):
    L, ptr = _lib.lib(), _lib.ptr
    col = K.case("random", n, 0)[0]
    src = dev(col)
    need = int(L.convdr_ip_compact_workspace_bytes(n, 16, 256))
    for name, keep in keep_patterns(n).items():
        outs = []
        for fill, seed in (("N", 0), ("R", 5)):
            bits = S.pack_row_mask(dev(keep))
            ws = filled(need, torch.uint8, fill, seed)
            n_kept = filled(1, torch.int64, fill, seed)
            dst = filled(n + GUARD, torch.int64, fill, seed + 1)
            guard = dst[n:].clone()
            _lib.check(L.convdr_ip_compact_plan(ptr(bits), bits.numel(), n, ptr(ws), need, ptr(n_kept), _lib.stream_ptr()), "plan")
            _lib.check(L.convdr_ip_compact_ids(ptr(src), ptr(dst), n, ptr(bits), bits.numel(), ptr(ws), need, _lib.stream_ptr()), "ids")
            kept = int(n_kept.item())
            assert kept == int(keep.sum()) and torch.equal(dst[n:], guard), name
            outs.append(dst[:kept].cpu().numpy())
        assert np.array_equal(outs[0], col[keep]) and np.array_equal(outs[1], col[keep]), "n=%d: %s" % (n, name)
        assert np.array_equal(src.cpu().numpy(), col), name
    # no bitmap: every row kept, a copy
    ws = filled(need, torch.uint8, "R", 1)
    n_kept = filled(1, torch.int64, "N", 0)
    dst = filled(n, torch.int64, "N", 0)
    _lib.check(L.convdr_ip_compact_plan(None, 0, n, ptr(ws), need, ptr(n_kept), _lib.stream_ptr()), "plan")
    _lib.check(L.convdr_ip_compact_ids(ptr(src), ptr(dst), n, None, 0, ptr(ws), need, _lib.stream_ptr()), "ids")
    assert int(n_kept.item()) == n and np.array_equal(dst.cpu().numpy(), col)


# ---- the index ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus(n, d_in, seed=5):
    """(X device fp32 [n, d_in] whose values are exact halves, Q device fp32 [6, d_in], E device fp32 [64, d_in] exact halves:
    re-encoded rows); never modified"""
    g = torch.Generator(device="cuda").manual_seed(seed * 1000 + n + d_in)
    X = torch.randn((n, d_in), generator=g, device="cuda").half().float()
    Q = torch.randn((6, d_in), generator=g, device="cuda")
    E = torch.randn((64, d_in), generator=g, device="cuda").half().float()
    return X, Q, E


def chunk_ids(n):
    """an id sits on up to three rows, anywhere in the block; negative and positive ids"""
    rs = np.random.RandomState(n)
    return (rs.permutation(n) // 3).astype(np.int64) * 1000003 - 40_000_000_000


def distinct_ids(n):
    return np.random.RandomState(n + 1).permutation(n).astype(np.int64) * 7 - 1000


def index(storage, precision, X, ids, window=512):
    """the rows added in two pieces, the first with host ids, the second with device ids"""
    idx = S.FlatIPIndex(X.shape[1], storage=storage, precision=precision, prepin=False)
    idx.compact_window_rows = window
    X = X.half() if storage == "fp16" else X
    cut = X.shape[0] // 3
    idx.add(X[:cut].clone(), ids=ids[:cut])
    idx.add(X[cut:].clone(), ids=dev(ids[cut:]))
    return idx


def id_list(ids, seed=0):
    """present ids (all their rows go), absent ids, repeated entries; shuffled"""
    rs = np.random.RandomState(seed + len(ids))
    present = rs.choice(np.unique(ids), size=max(1, len(ids) // 7), replace=False)
    absent = np.arange(25, dtype=np.int64) * 1000003 + 17
    lst = np.concatenate([present, absent, present[:9], absent[:3]])
    rs.shuffle(lst)
    return lst


def bits_of(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def held(idx):
    return {name: getattr(idx, name) for name in ("_p32", "_pbf", "_plo") if getattr(idx, name) is not None}


def assert_same_index(a, b, Q, what):
    assert a.ntotal == b.ntotal, what
    assert sorted(held(a)) == sorted(held(b)), what
    for k, v in held(a).items():
        assert torch.equal(bits_of(v), bits_of(held(b)[k])), "%s: %s" % (what, k)
    assert torch.equal(a.ids, b.ids), what
    ra, rb = a.reconstruct_n(0, a.ntotal), b.reconstruct_n(0, b.ntotal)
    assert ra.tobytes() == rb.tobytes(), what
    (Da, Ia), (Db, Ib) = a.search(Q, 10), b.search(Q, 10)
    assert Da.tobytes() == Db.tobytes() and np.array_equal(Ia, Ib), what


def same_result(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("storage,precision", CONFIGS)
@pytest.mark.parametrize("n,d_in", SHAPES)
def test_search_ids_id_filter_and_rows_of_equal_the_row_number_route(storage, precision, n, d_in):
    X, Q, _ = corpus(n, d_in)
    ids = chunk_ids(n)
    idx = index(storage, precision, X, ids)
    assert idx.ntotal == n and np.array_equal(idx.ids.cpu().numpy(), ids)
    D, I = idx.search(Q, 10)
    Dk, Ik = idx.search_ids(Q, 10)
    assert Dk.tobytes() == D.tobytes() and Ik.dtype == np.int64 and np.array_equal(Ik, ids[I])
    lst = id_list(ids)
    isin = K.member(ids, lst)
    for invert in (False, True):
        mask = isin != invert
        f = idx.id_filter(lst, invert=invert)
        assert f.n == n and f.n_allowed == int(mask.sum()) and np.array_equal(f.bits.cpu().numpy(), packed(mask))
        assert same_result(idx.search(Q, 10, allowed=f), idx.search(Q, 10, allowed=mask)), invert
    # fewer allowed rows than k: the padding stays -1
    few = idx.id_filter(lst[:1])
    Dk, Ik = idx.search_ids(Q, 10, allowed=few)
    D, I = idx.search(Q, 10, allowed=few)
    assert few.n_allowed < 10 and (I[:, few.n_allowed:] == -1).all() and np.array_equal(Ik, np.where(I >= 0, ids[np.maximum(I, 0)], -1))
    first, count = idx.rows_of(dev(lst))
    want = K.locate(ids, lst)
    assert first.dtype == torch.int64 and count.dtype == torch.int32
    assert np.array_equal(first.cpu().numpy(), want[0]) and np.array_equal(count.cpu().numpy(), want[1])
    on = lst[want[0] >= 0]
    assert idx.reconstruct_ids(on).tobytes() == idx.reconstruct_batch(want[0][want[0] >= 0]).tobytes()
    with pytest.raises(IndexError):
        idx.reconstruct_ids(lst)


@pytest.mark.parametrize("storage,precision", (("fp32", "auto"), ("fp16", "auto")))
def test_the_column_follows_reserve_reset_twin_update_rows_and_a_refused_add(storage, precision):
    n, d_in = 1317, 64
    X, _, E = corpus(n, d_in)
    ids = chunk_ids(n)
    idx = S.FlatIPIndex(d_in, storage=storage, precision=precision, prepin=False)
    idx.reserve(2 * n)
    assert idx.ids is None
    idx.add(X[:500].clone(), ids=ids[:500])
    column = idx._sid
    assert column.shape[0] == 2 * n and column.dtype == torch.int64 and column.is_cuda
    idx.add(X[500:].clone(), ids=dev(ids[500:]))
    assert idx._sid.data_ptr() == column.data_ptr() and np.array_equal(idx.ids.cpu().numpy(), ids)      # filled in place
    idx.update_rows(3, E[:2].contiguous())
    assert np.array_equal(idx.ids.cpu().numpy(), ids)
    with pytest.raises(ValueError, match="carries row ids"):
        idx.add(X[:2].clone())
    with pytest.raises(ValueError):
        idx.add(X[:2].clone(), ids=np.array([1, S.RESERVED_ID]))
    with pytest.raises(ValueError):
        idx.add(X[:2].clone(), ids=torch.tensor([1, S.RESERVED_ID], device="cuda"))
    if storage == "fp16":
        bad = X[:3].clone()
        bad[1, 5] = float("inf")
        with pytest.raises(_lib.ConvdrError, match="unchanged"):
            idx.add(bad, ids=np.array([1, 2, 3]))
    assert idx.ntotal == n and np.array_equal(idx.ids.cpu().numpy(), ids)
    idx.reserve(3 * n)
    assert idx._sid.shape[0] == 3 * n and np.array_equal(idx.ids.cpu().numpy(), ids)
    assert idx.twin().ids is None
    idx.reset()
    assert idx.ids is None and idx.ntotal == 0
    idx.add(X[:4].clone())                       # after a reset the index may go without ids
    assert idx.ids is None and idx.ntotal == 4


@pytest.mark.parametrize("storage,precision", CONFIGS)
@pytest.mark.parametrize("n,d_in", SHAPES)
def test_remove_ids_equals_remove_rows_of_the_isin_mask(storage, precision, n, d_in):
    X, Q, _ = corpus(n, d_in)
    ids = chunk_ids(n)
    a, b = index(storage, precision, X, ids), index(storage, precision, X, ids)
    lst = id_list(ids)
    isin = K.member(ids, lst)
    before = a.id_filter(lst[:5])
    assert same_result(a.search(Q, 10, allowed=before), b.search(Q, 10, allowed=K.member(ids, lst[:5])))
    removed = a.remove_ids(dev(lst))
    assert removed == b.remove_rows(isin.astype(np.uint8)) == int(isin.sum()) and removed > 0
    assert a.stats["removed"] == removed and a.stats["compact_windows"] == b.stats["compact_windows"]
    assert a.stats["ids_missing"] == K.missing(ids, lst) > 0
    assert np.array_equal(a.ids.cpu().numpy(), ids[~isin])
    assert_same_index(a, b, Q, "after remove_ids")
    with pytest.raises(ValueError, match="stale"):
        a.search(Q, 10, allowed=before)
    # ids that are on no row (now): nothing goes, a filter stays valid
    f = a.id_filter(ids[~isin][:3])
    assert a.remove_ids(lst) == 0 and a.stats["ids_missing"] == len(np.unique(lst)) and a.ntotal == n - removed
    assert a.remove_ids(np.zeros(0, np.int64)) == 0 and a.stats["ids_missing"] == 0
    assert same_result(a.search(Q, 10, allowed=f), b.search(Q, 10, allowed=K.member(ids[~isin], ids[~isin][:3])))
    # the next add carries on behind the compacted column
    a.add(X[:4].half() if storage == "fp16" else X[:4].clone(), ids=np.array([1, 2, 3, 4]))
    assert np.array_equal(a.ids.cpu().numpy(), np.concatenate([ids[~isin], [1, 2, 3, 4]]))


@pytest.mark.parametrize("storage,precision", CONFIGS)
@pytest.mark.parametrize("n,d_in", SHAPES)
def test_keep_rows_and_remove_rows_carry_the_id_column(storage, precision, n, d_in):
    X, _, _ = corpus(n, d_in)
    ids = chunk_ids(n)
    for window in (256, 512):
        for name in ("random half", "word and tile edges removed", "one row per tile", "only the last row removed"):
            keep = keep_patterns(n)[name]
            idx = index(storage, precision, X, ids, window)
            idx.keep_rows(keep)
            assert idx.ntotal == int(keep.sum()) and np.array_equal(idx.ids.cpu().numpy(), ids[keep]), (window, name)
        idx = index(storage, precision, X, ids, window)
        gone = np.array([0, 31, 32, 255, 256, n - 1, 31])
        idx.remove_rows(gone)
        assert np.array_equal(idx.ids.cpu().numpy(), np.delete(ids, gone)), window
        idx.remove_rows(np.array([0]))              # the two id buffers have changed roles once: and back
        assert np.array_equal(idx.ids.cpu().numpy(), np.delete(ids, gone)[1:]), window


@pytest.mark.parametrize("storage,precision", CONFIGS)
@pytest.mark.parametrize("n,d_in", SHAPES)
def test_upsert_equals_update_rows_per_row_and_one_add(storage, precision, n, d_in):
    X, Q, E = corpus(n, d_in)
    ids = distinct_ids(n)
    a, b = index(storage, precision, X, ids), index(storage, precision, X, ids)
    rows = np.array(list(dict.fromkeys([0, n - 1, 255, 256, 31, 32] + list(range(100, 160, 3))))[:20])     # 20 distinct rows
    fresh = np.arange(15, dtype=np.int64) * 7 - 999                                               # 15 ids on no row
    lst = np.empty(35, np.int64)
    is_new = np.zeros(35, bool)
    is_new[1::2][:15] = True
    lst[~is_new], lst[is_new] = ids[rows], fresh
    emb = E[:35].contiguous()
    assert a.upsert(lst, emb) == (20, 15)
    for j in np.nonzero(~is_new)[0]:
        b.update_rows(int(np.nonzero(ids == lst[j])[0][0]), emb[j:j + 1])
    new = dev(np.nonzero(is_new)[0])
    b.add(emb[new], ids=lst[is_new])
    assert a.ntotal == n + 15 and np.array_equal(a.ids.cpu().numpy(), np.concatenate([ids, fresh]))
    assert_same_index(a, b, Q, "after upsert")
    assert torch.equal(a._max_norm, b._max_norm)
    if storage == "fp16":
        assert a.update_flags() == b.update_flags() == 0
    assert a.reconstruct_ids(lst).tobytes() == emb.cpu().numpy().tobytes()
    (D, I), (Dk, Ik) = a.search(emb[:4], 3), a.search_ids(emb[:4], 3)
    assert np.array_equal(Ik, a.ids.cpu().numpy()[I]) and Dk.tobytes() == D.tobytes()

    # refused before anything is written: a repeated list id, an id on two rows
    def state(idx):
        return idx.ntotal, {k: bits_of(v).clone() for k, v in held(idx).items()}, idx.ids.clone(), idx._max_norm.clone()

    def unchanged(idx, was):
        now = state(idx)
        return now[0] == was[0] and all(torch.equal(now[1][k], was[1][k]) for k in was[1]) and torch.equal(now[2], was[2]) \
            and torch.equal(now[3], was[3])
    was = state(a)
    with pytest.raises(ValueError, match="repeats an id"):
        a.upsert(np.array([lst[0], 123456, lst[0]]), E[40:43].contiguous())
    assert unchanged(a, was)
    c = index(storage, precision, X, chunk_ids(n))
    twice = chunk_ids(n)[0]
    assert int((chunk_ids(n) == twice).sum()) > 1
    was = state(c)
    with pytest.raises(ValueError, match="sits on"):
        c.upsert(np.array([777, twice]), E[40:42].contiguous())
    assert unchanged(c, was)
    with pytest.raises(ValueError):
        c.upsert(np.array([777, 778]), E[40:43].contiguous())            # two ids, three rows
    assert unchanged(c, was)
