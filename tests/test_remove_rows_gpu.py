"""Removing rows in place: FlatIPIndex.keep_rows / remove_rows / reconstruct* and the convdr_ip_compact_* entries.

Shapes and keep patterns are chosen for the kernels' edges (ragged last tile, one tile and a row, windows of one and two
tiles, every window form), not for the workload.  Everything is compared bit for bit: the compaction moves bytes, and a
search after the removal must equal the row-filtered search before it with the ids renumbered by cumsum(keep) - 1."""
import functools

import numpy as np
import pytest
import torch

from convdr_amd import _lib
from convdr_amd import search as S
from tests.helpers import fill_bytes

pytestmark = pytest.mark.gpu

CONFIGS = (("fp32", "auto"), ("fp32", "bf16"), ("fp32", "fp16x3"), ("fp16", "auto"))
SHAPES = ((1317, 64), (257, 768), (5000, 100), (1317, 768))          # (n, d_in); 100 is padded to 128 columns
WINDOWS = (256, 512)


def patterns(n, w, seed=0):
    """name -> keep mask (numpy bool [n]); w: the window the index will use"""
    rs = np.random.RandomState(seed + n)
    p = {}
    p["none removed"] = np.ones(n, bool)
    p["all removed"] = np.zeros(n, bool)
    for name, r in (("first row", 0), ("last row", n - 1)):
        k = np.zeros(n, bool); k[r] = True
        p["only the %s kept" % name] = k
        p["only the %s removed" % name] = ~k
    k = np.zeros(n, bool)
    for t in range((n + 255) // 256):
        k[min(n - 1, t * 256 + (t * 37 + 5) % 256)] = True
    p["one row per tile"] = k
    k = np.zeros(n, bool); k[::2] = True
    p["alternating"] = k
    k = np.ones(n, bool); k[w:2 * w] = False                      # (n <= w: nothing removed)
    p["one whole window removed"] = k
    k = np.zeros(n, bool); k[:2 * w] = True; k[2 * w::2] = True
    p["untouched prefix of two windows, then every second row"] = k
    k = np.ones(n, bool); k[:n // 2] = False
    p["first half removed"] = k
    k = np.ones(n, bool); k[[r for r in (31, 32, 255, 256) if r < n]] = False
    p["word and tile edges"] = k
    p["random half"] = rs.rand(n) < 0.5
    p["random 1 %"] = rs.rand(n) >= 0.01
    return p


@functools.lru_cache(maxsize=None)
def corpus(n, d_in, seed=3):
    """(X device fp32 [n, d_in] whose values are exact halves, Q device fp32 [6, d_in]); never modified"""
    g = torch.Generator(device="cuda").manual_seed(seed * 1000 + n + d_in)
    X = torch.randn((n, d_in), generator=g, device="cuda").half().float()
    Q = torch.randn((6, d_in), generator=g, device="cuda")
    Q[0] = X[n // 3] * 0.5           # a query that favours one row (and its duplicates, where a test makes some)
    return X, Q


def index(storage, precision, X, window, reserve=0):
    idx = S.FlatIPIndex(X.shape[1], storage=storage, precision=precision, prepin=False)
    idx.compact_window_rows = window
    if reserve:
        idx.reserve(reserve)
    idx.add(X.half() if storage == "fp16" else X.clone())       # (clone: an unreserved index adopts the tensor it is given)
    return idx


def bits_of(t):
    """a buffer's rows as integers (NaN payloads and signed zeros compare as bits)"""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def held(idx):
    return {name: getattr(idx, name) for name in ("_p32", "_pbf", "_plo") if getattr(idx, name) is not None}


def remap_of(keep):
    return np.cumsum(keep) - 1


def remapped(I, keep):
    return np.where(I >= 0, remap_of(keep)[np.maximum(I, 0)], -1)


def assert_same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def window_forms(keep, w):
    """the form every window takes by the rule of include/convdr_hip.h ("Removing rows": windows), from the mask alone"""
    n, dest, forms = len(keep), np.concatenate([[0], np.cumsum(keep)]), []
    for a in range(0, n, w):
        b = min(n, a + w)
        kept = dest[b] - dest[a]
        forms.append("skip" if dest[a] == a and kept == b - a else "direct" if dest[a] + kept <= a else "bounce")
    return forms


def test_the_patterns_reach_every_window_form_at_every_window_size():
    for n, _ in SHAPES:
        for w in WINDOWS:
            seen = {f for keep in patterns(n, w).values() for f in window_forms(keep, w)}
            assert seen == {"skip", "direct", "bounce"}, (n, w, seen)
    forms = window_forms(patterns(1317, 256)["untouched prefix of two windows, then every second row"], 256)
    assert forms[:4] == ["skip", "skip", "bounce", "direct"], forms
    assert set(window_forms(patterns(5000, 512)["first half removed"], 512)[5:]) == {"direct"}


# ---- the buffers, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,precision", CONFIGS)
@pytest.mark.parametrize("n,d_in", SHAPES)
def test_kept_rows_move_to_the_front_of_every_buffer_bit_for_bit(storage, precision, n, d_in):
    X, _ = corpus(n, d_in)
    idx = S.FlatIPIndex(d_in, storage=storage, precision=precision, prepin=False)
    idx.reserve(n)
    for window in WINDOWS:
        idx.compact_window_rows = window
        for name, keep in patterns(n, window).items():
            what = "%s / %s n=%d d=%d window=%d: %s" % (storage, precision, n, d_in, window, name)
            idx.reset()
            idx.add(X.half() if storage == "fp16" else X)
            before = {k: bits_of(v).clone() for k, v in held(idx).items()}
            assert sorted(before) == (["_pbf"] if storage == "fp16" else ["_p32", "_pbf", "_plo"] if precision == "fp16x3"
                                      else ["_p32", "_pbf"]), what
            removed = idx.keep_rows(keep)
            kd = torch.as_tensor(keep, device="cuda")
            assert removed == n - int(keep.sum()) and idx.ntotal == int(keep.sum()), what
            assert idx.stats["removed"] == removed, what
            assert idx.stats["compact_windows"] == (0 if not removed else (n + window - 1) // window), what
            if removed:
                assert int(idx._n_kept.item()) == idx.ntotal, what
            for k, v in held(idx).items():
                assert v.shape[0] == idx.ntotal and torch.equal(bits_of(v), before[k][kd]), "%s: %s" % (what, k)


def test_compact_entries_directly_on_raw_buffers():
    """A plan and convdr_ip_compact_rows on a [n, 16]-byte buffer (the narrowest legal row) and on 3,072-byte rows, without
    FlatIPIndex; the workspace holds NaN bytes before the plan."""
    L, ptr = _lib.lib(), _lib.ptr
    for n in (1317, 257, 5000):
        for window in WINDOWS:
            for name, keep in patterns(n, window).items():
                kd = torch.as_tensor(keep, device="cuda")
                bits = S.pack_row_mask(kd)
                need = L.convdr_ip_compact_workspace_bytes(n, 3072, window)
                assert need > 0
                ws = fill_bytes(torch.empty(need, dtype=torch.uint8, device="cuda"), "N")
                n_kept = torch.full((1,), -7, dtype=torch.int64, device="cuda")
                _lib.check(L.convdr_ip_compact_plan(ptr(bits), bits.numel(), n, ptr(ws), need, ptr(n_kept), _lib.stream_ptr()), "plan")
                for row_bytes in (16, 3072):
                    buf = torch.randint(0, 256, (n, row_bytes), dtype=torch.uint8, device="cuda",
                                        generator=torch.Generator(device="cuda").manual_seed(n + row_bytes))
                    want = buf[kd]
                    _lib.check(L.convdr_ip_compact_rows(ptr(buf), row_bytes, n, ptr(bits), bits.numel(), window, ptr(ws), need,
                                                        _lib.stream_ptr()), "rows")
                    what = "n=%d window=%d row_bytes=%d: %s" % (n, window, row_bytes, name)
                    assert int(n_kept.item()) == int(keep.sum()), what
                    assert torch.equal(buf[:int(keep.sum())], want), what
    # no bitmap: every row kept, n_kept = n; an empty block: n_kept = 0
    ws = fill_bytes(torch.empty(L.convdr_ip_compact_workspace_bytes(1317, 16, 256), dtype=torch.uint8, device="cuda"), "N")
    n_kept = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    _lib.check(L.convdr_ip_compact_plan(None, 0, 1317, ptr(ws), ws.numel(), ptr(n_kept[:1]), _lib.stream_ptr()), "plan")
    _lib.check(L.convdr_ip_compact_plan(None, 0, 0, ptr(ws), ws.numel(), ptr(n_kept[1:]), _lib.stream_ptr()), "plan")
    assert n_kept.tolist() == [1317, 0]


# ---- search equivalence, bit for bit, no tolerance ------------------------------------------------------------------------
def searched_pair(storage, precision, X, Q, keep, window, k):
    """(D, I) of search(Q, k, allowed=keep) on the untouched index and of search(Q, k) after keep_rows(keep)"""
    idx = index(storage, precision, X, window)
    Db, Ib = idx.search(Q, k, allowed=keep)
    idx.keep_rows(keep)
    Da, Ia = idx.search(Q, k)
    return (Db, Ib), (Da, Ia), idx


@pytest.mark.parametrize("storage,precision", CONFIGS)
def test_search_after_keep_rows_equals_the_filtered_search_before(storage, precision):
    n, d_in, window = 1317, 768, 256
    X, Q = corpus(n, d_in)
    X = X.clone()
    t = n // 3
    X[t + 2] = X[t]                   # exact duplicates straddling a removed row: the tie is broken by row, before and after
    X[t + 4] = X[t]
    pats = patterns(n, window)
    for name in ("random half", "untouched prefix of two windows, then every second row", "first half removed", "one row per tile",
                 "random 1 %"):
        keep = pats[name].copy()
        if name != "one row per tile":
            keep[[t, t + 2, t + 4]] = True
            keep[[t + 1, t + 3]] = False
        for k in (10, int(keep.sum()) + 3):
            (Db, Ib), (Da, Ia), idx = searched_pair(storage, precision, X, Q, keep, window, k)
            what = "%s / %s %s k=%d" % (storage, precision, name, k)
            assert_same_bits(Da, Db, what)
            assert np.array_equal(Ia, remapped(Ib, keep)), what
            assert (Ib[:, min(k, int(keep.sum())):] == -1).all(), what
            if name == "random half" and k == 10:
                r = remap_of(keep)
                assert Ia[0, :3].tolist() == [r[t], r[t + 2], r[t + 4]], what


def test_search_after_keep_rows_equals_the_oracle_on_the_kept_rows():
    from oracle import search as OS
    n, d_in = 1317, 768
    X, Q = corpus(n, d_in)
    keep = patterns(n, 512)["random half"]
    idx = index("fp32", "auto", X, 512)
    idx.keep_rows(keep)
    D, I = idx.search(Q, 20)
    Dr, Ir = OS.flat_ip_search(Q.cpu().numpy(), X.cpu().numpy()[keep], 20)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_range_search_and_rank_rows_after_keep_rows(storage):
    n, d_in, window = 5000, 100, 512
    X, Q = corpus(n, d_in)
    keep = patterns(n, window)["random half"]
    idx = index(storage, "auto", X, window)
    radius = np.float32(np.sort((Q @ X.T).cpu().numpy(), axis=1)[:, -40])
    targets = np.nonzero(keep)[0][[0, 7, 100, 1000, -1, 55]]
    lb, Db, Ib = idx.range_search(Q, radius, allowed=keep)
    rb = idx.rank_rows(Q, targets, allowed=keep)
    idx.keep_rows(keep)
    la, Da, Ia = idx.range_search(Q, radius)
    ra = idx.rank_rows(Q, remap_of(keep)[targets])
    assert np.array_equal(la, lb) and la[-1] > 0
    assert_same_bits(Da, Db, "range_search D")
    assert np.array_equal(Ia, remap_of(keep)[Ib])
    assert np.array_equal(ra, rb) and (ra >= 0).all()


# ---- add after remove, with stale memory --------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,precision", CONFIGS)
@pytest.mark.parametrize("reserve", [False, True])
@pytest.mark.parametrize("poison", [False, True])
def test_add_after_remove_equals_one_index_searched_with_a_filter(storage, precision, reserve, poison):
    """A: add X, remove_rows, add Y.  B: add X, add Y, searched with allowed = keep + all of Y.  poison: the workspace and the
    rows past ntotal hold NaN bytes before the removal and again before the add."""
    n, m, d_in, window = 1317, 300, 768, 256
    X, Q = corpus(n, d_in)
    Y = corpus(m, d_in, seed=5)[0]
    cast = (lambda t: t.half()) if storage == "fp16" else (lambda t: t.clone())
    keep = patterns(n, window)["random half"]
    A = index(storage, precision, X, window, reserve=(n + m + 100) if reserve else 0)

    def poison_now():
        if not poison:
            return
        need = _lib.lib().convdr_ip_compact_workspace_bytes(A.ntotal, 4 * A.d, window)
        fill_bytes(A._workspace(need), "N")
        for t in (A._s32, A._s16, A._slo):
            if t is not None and t.shape[0] > A.ntotal:
                fill_bytes(t[A.ntotal:], "N")
    poison_now()
    assert A.remove_rows(np.nonzero(~keep)[0]) == int((~keep).sum())
    poison_now()
    A.add(cast(Y))
    B = index(storage, precision, X, window)
    B.add(cast(Y))
    both = np.concatenate([keep, np.ones(m, bool)])
    assert A.ntotal == int(both.sum())
    for k in (10, 200):
        Da, Ia = A.search(Q, k)
        Db, Ib = B.search(Q, k, allowed=both)
        assert_same_bits(Da, Db, "k=%d" % k)
        assert np.array_equal(Ia, remapped(Ib, both)), k


def test_remove_rows_forms_agree_with_keep_rows():
    n, d_in, window = 1317, 64, 256
    X, Q = corpus(n, d_in)
    keep = patterns(n, window)["random half"]
    gone = np.nonzero(~keep)[0]
    ref = index("fp32", "auto", X, window)
    assert ref.keep_rows(keep) == len(gone)
    forms = (np.concatenate([gone, gone[:50], gone[-1:]]), torch.as_tensor(np.concatenate([gone[::-1], gone[:9]]), device="cuda"),
             ~keep, torch.as_tensor((~keep).astype(np.uint8) * 3, device="cuda"))
    for rows in forms:
        idx = index("fp32", "auto", X, window)
        assert idx.remove_rows(rows) == len(gone) and idx.ntotal == ref.ntotal
        for k, v in held(idx).items():
            assert torch.equal(bits_of(v), bits_of(held(ref)[k])), k
    idx = index("fp32", "auto", X, window)
    with pytest.raises(ValueError):
        idx.remove_rows(torch.as_tensor([5, n], device="cuda"))          # ids on the device: checked with the kept count
    assert idx.ntotal == n and torch.equal(idx._p32, X)


# ---- extra memory is bounded ----------------------------------------------------------------------------------------------
def test_extra_memory_of_keep_rows_is_bounded_by_one_window():
    """n = 20,000 x 768 fp32 (61 MB), windows of 1,024 rows: a 3 MB bounce buffer and masks under 1 MB -- the rise of the
    allocator's peak must stay below a quarter of the fp32 block.  The out-of-place P[keep] needs half of it."""
    n, d = 20000, 768
    g = torch.Generator(device="cuda").manual_seed(9)
    X = torch.randn((n, d), generator=g, device="cuda")
    idx = S.FlatIPIndex(d, precision="auto", prepin=False)
    idx.compact_window_rows = 1024
    idx.add(X)                                            # adopted: the index holds X itself
    keep = torch.rand(n, generator=g, device="cuda") < 0.5
    want = X[keep]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    removed = idx.keep_rows(keep)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("keep_rows: peak rise %d bytes, fp32 block %d bytes" % (rise, n * d * 4))
    assert rise < n * d * 4 // 4, (rise, n * d * 4)
    assert removed == n - want.shape[0] and torch.equal(idx._p32, want)


# ---- reconstruct ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("d_in", [100, 768])
def test_reconstruct_returns_the_corpus_rows(storage, d_in):
    n = 1317
    g = torch.Generator(device="cuda").manual_seed(d_in)
    X = torch.randn((n, d_in), generator=g, device="cuda") * 3.0          # (not exact halves: the half store rounds them)
    Xn = X.cpu().numpy()
    want = Xn.astype(np.float16).astype(np.float32) if storage == "fp16" else Xn
    idx = S.FlatIPIndex(d_in, storage=storage, prepin=False)
    idx.compact_window_rows = 256
    idx.add(X.clone())
    ids = np.array([0, 5, 5, n - 1, 256, 255])
    assert_same_bits(idx.reconstruct_batch(ids), want[ids], "batch")
    assert_same_bits(idx.reconstruct(n - 1), want[n - 1], "one")
    assert_same_bits(idx.reconstruct_n(250, 20), want[250:270], "n")
    t = idx.rows_tensors(torch.as_tensor(ids, device="cuda").reshape(2, 3))
    assert t.is_cuda and t.dtype == torch.float32 and t.shape == (2, 3, d_in)
    assert_same_bits(t.cpu().numpy().reshape(6, d_in), want[ids], "tensors")
    keep = patterns(n, 256)["random half"]
    idx.keep_rows(keep)
    assert_same_bits(idx.reconstruct_n(0, idx.ntotal), want[keep], "after a removal")
    for bad in (lambda: idx.reconstruct(idx.ntotal), lambda: idx.reconstruct(-1), lambda: idx.reconstruct_n(idx.ntotal - 1, 2),
                lambda: idx.reconstruct_batch(np.array([0, n - 1])), lambda: idx.rows_tensors(torch.as_tensor([idx.ntotal], device="cuda"))):
        with pytest.raises(IndexError):
            bad()
