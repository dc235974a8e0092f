"""Snapshots on the device: convdr_digest_rows against the numpy oracle of tests/snapshot_cases.py, and FlatIPIndex.save / load /
fingerprint: an index that no single block file reproduces (three adds, an upsert that appends and overwrites, a removal, an
update) comes back from its snapshot bit for bit -- state, rebuilt scan copy and every kind of answer --, slices, reservations,
precision overrides, corruption, and the staging buffers a save shares with every add.  Every comparison is exact."""
import functools
import os

import numpy as np
import pytest
import torch

from convdr_amd import _lib, snapshot
from convdr_amd import search as S
from tests import snapshot_cases as C
from tests.helpers import fill_bytes

pytestmark = pytest.mark.gpu

W = 256                          # window_rows of the round trips: ~1,300 rows make 6 windows, the last one short
# (n_rows, row_bytes, window_rows, word0)
DIGEST_CASES = ((1, 8, 1, 0), (3, 8, 2, 0), (257, 8, 100, 1 << 40), (5, 1536, 2, 7), (1031, 3072, 256, 0), (70000, 8, 65536, 0))


def device_digest(t, n_rows, row_bytes, window_rows, word0, fill="N", guard=3):
    """convdr_digest_rows into an output pre-filled with `fill`, `guard` slots behind it that must stay as they were"""
    windows = (n_rows + window_rows - 1) // window_rows
    out = fill_bytes(torch.empty((windows + guard, 2), dtype=torch.int64, device="cuda"), fill, 5)
    before = out.clone()
    _lib.check(_lib.lib().convdr_digest_rows(_lib.ptr(t), n_rows, row_bytes, word0, window_rows, _lib.ptr(out), _lib.stream_ptr()),
               "convdr_digest_rows")
    assert torch.equal(out[windows:], before[windows:])
    host = out[:windows].cpu().numpy().astype(np.uint64)
    return [(int(a), int(b)) for a, b in host], before[:windows]


@functools.lru_cache(maxsize=None)
def case_bytes(n_rows, row_bytes):
    raw = np.frombuffer(np.random.RandomState(n_rows + row_bytes).bytes(n_rows * row_bytes), dtype=np.uint8)
    raw.flags.writeable = False
    return raw


@pytest.mark.parametrize("case", DIGEST_CASES)
def test_the_device_digest_equals_the_oracle(case):
    n_rows, row_bytes, window_rows, word0 = case
    raw = case_bytes(n_rows, row_bytes)
    t = torch.from_numpy(np.array(raw)).cuda()
    want = C.window_digests(raw, row_bytes, window_rows, word0)
    got, _ = device_digest(t, n_rows, row_bytes, window_rows, word0, fill="N")
    assert got == want
    again, _ = device_digest(t, n_rows, row_bytes, window_rows, word0, fill="R")           # other garbage in `out`, the same bits
    assert again == want
    assert snapshot.digest_host(raw, word0) == C.digest(raw, word0)                        # device == host on the same bytes
    one, _ = device_digest(t, n_rows, row_bytes, n_rows, word0)
    total = (0, 0)
    for d in got:
        total = C.add(total, d)
    assert one == [total] == [snapshot.digest_host(raw, word0)]                            # the windows sum to the one-window digest


def test_a_view_that_begins_on_an_odd_word_and_the_empty_buffer():
    raw = case_bytes(1031, 3072)
    t = torch.from_numpy(np.array(raw)).cuda()
    assert t.data_ptr() % 16 == 0
    for rows, rb, w, word0 in ((1000, 3072, 256, 3), (4999, 8, 1000, 0), (1, 8, 1, 9)):
        view = t[8:8 + rows * rb]                            # 8 bytes into the allocation: 8-byte aligned, not 16
        got, _ = device_digest(view, rows, rb, w, word0)
        assert got == C.window_digests(raw[8:8 + rows * rb], rb, w, word0), (rows, rb, w)
    out = fill_bytes(torch.empty((4, 2), dtype=torch.int64, device="cuda"), "N", 1)
    before = out.clone()
    assert _lib.lib().convdr_digest_rows(_lib.ptr(t), 0, 3072, 0, 256, _lib.ptr(out), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, before)                          # n_rows == 0: nothing launched, nothing written


# ---- round trips -----------------------------------------------------------------------------------------------------------
def corpus(d_in, seed=0):
    rs = np.random.RandomState(seed)
    rows = (rs.randn(1400, d_in) + 0.7 * rs.randn(1, d_in)).astype(np.float32)      # a common component: the centre matters
    rows *= np.exp(0.3 * rs.randn(1400, 1)).astype(np.float32)
    return rows, rs.randn(5, d_in).astype(np.float32)


def make_index(storage, precision, with_ids, center, d_in, **kw):
    return S.FlatIPIndex(d_in, precision=precision, center=None if storage == "fp16" else center, storage=storage, prepin=False, **kw)


def build(storage, precision, with_ids, center, d_in):
    """~1,300 rows no single block reproduces: three adds, an upsert that overwrites 30 rows and appends 20, a removal of 70
    ids (without ids: the same in row numbers), an update_rows"""
    rows, Q = corpus(d_in)
    idx = make_index(storage, precision, with_ids, center, d_in)
    ids = np.arange(1400, dtype=np.int64) * 7 - 3000
    for a, b in ((0, 500), (500, 950), (950, 1350)):
        idx.add(rows[a:b], ids=ids[a:b] if with_ids else None)
    fresh = torch.from_numpy(rows[1350:1400] * 1.5).cuda()
    if with_ids:
        assert idx.upsert(np.concatenate([ids[100:130], ids[1350:1370]]), fresh) == (30, 20)
        assert idx.remove_ids(ids[600:670]) == 70
    else:
        idx.update_rows(100, fresh[:30].contiguous())
        idx.add(fresh[30:])
        assert idx.remove_rows(np.arange(600, 670)) == 70
    idx.update_rows(7, torch.from_numpy(rows[1380:1400] * 0.5).cuda())
    assert idx.ntotal == 1300
    return idx, Q


def bits(t):
    return None if t is None else t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


def same_state(A, B):
    assert B.fingerprint() == A.fingerprint()
    assert B._scale == A._scale and bits(B._max_norm) == bits(A._max_norm) and bits(B._centre) == bits(A._centre)
    assert B.ntotal == A.ntotal and (B.ids is None) == (A.ids is None)
    assert torch.equal(B._pbf, A._pbf)                       # the rebuilt scan copy
    if A.ids is not None:
        assert torch.equal(B.ids, A.ids)


def same_answers(A, B, Q):
    for k in (10, 5000):
        ra, sa = A.search(Q, k), dict(A.stats)
        rb, sb = B.search(Q, k), dict(B.stats)
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and sa == sb, (k, sa, sb)
    D10, I10 = A.search(Q, 10)
    radius = D10[:, 7].copy()
    for x, y in zip(A.range_search(Q, radius), B.range_search(Q, radius)):
        assert np.array_equal(x, y)
    targets = I10[:, ::3].copy()
    assert np.array_equal(A.rank_rows(Q, targets), B.rank_rows(Q, targets))
    if A.ids is not None:
        da, db = A.search_docs(Q, 10), B.search_docs(Q, 10)
        for x, y in zip(da, db):
            assert torch.equal(x, y)
        for x, y in zip(A.score_ids(Q, da[1]), B.score_ids(Q, da[1])):
            assert np.array_equal(x, y)


def chunk_for(idx, chunks=7):
    return max(4 * idx.d, idx.ntotal * idx.d * (2 if idx.storage == "fp16" else 4) // chunks)


MATRIX = [(storage, precision, with_ids, center, d_in)
          for storage, precision, centers in (("fp32", "auto", (True, False)), ("fp32", "bf16", (True, False)), ("fp16", "auto", (False,)))
          for with_ids in (True, False) for center in centers for d_in in (64, 100, 768)]


@pytest.mark.parametrize("storage,precision,with_ids,center,d_in", MATRIX)
def test_an_index_comes_back_from_its_snapshot_bit_for_bit(tmp_path, storage, precision, with_ids, center, d_in):
    A, Q = build(storage, precision, with_ids, center, d_in)
    A.host_chunk_bytes = chunk_for(A)                       # >= 7 chunks through 4 staging buffers: the ring wraps
    path = str(tmp_path / "a.convdr")
    A.save(path, window_rows=W)
    assert A.stats["save_bytes"] == os.path.getsize(path) and A.stats["save_s"] > 0
    h = S.verify_snapshot(path)
    assert (h["n"], h["d_in"], h["d"], h["storage"], h["precision"], h["center"], h["has_ids"], h["window_rows"]) == \
        (1300, d_in, A.d, storage, precision, A.center, with_ids, W)
    assert len(h["sections"]["rows"]["digests"]) == 6 and ("centre" in h["sections"]) == A.center
    # the file holds the resident rows: the oracle's digest of what reconstruct / the store gives
    assert h["sections"]["rows"]["digests"] == C.window_digests(A._rows.cpu().view(torch.uint8).numpy(), h["sections"]["rows"]["row_bytes"], W)
    B = S.FlatIPIndex.load(path, chunk_bytes=A.host_chunk_bytes, prepin=False)
    assert B.stats["load_bytes"] == sum(s["bytes"] for s in h["sections"].values()) and B.stats["load_s"] > 0
    assert (B.storage, B.precision, B.center, B.d_in, B._x3_first) == (A.storage, A.precision, A.center, A.d_in, A._x3_first)
    same_state(A, B)
    same_answers(A, B, Q)


def test_the_ring_of_staging_buffers_wraps_for_the_id_column_too(tmp_path):
    A, Q = build("fp32", "auto", True, True, 64)
    A.host_chunk_bytes = 1024                               # 4 rows per chunk: 325 chunks of rows, 11 of ids
    path = str(tmp_path / "a.convdr")
    A.save(path, window_rows=W)
    S.verify_snapshot(path)
    B = S.FlatIPIndex.load(path, chunk_bytes=1024, prepin=False)
    same_state(A, B)


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """one fp32 index with ids and its snapshot, shared by the follow-up tests (none of them modifies either)"""
    A, Q = build("fp32", "auto", True, True, 64)
    A.host_chunk_bytes = chunk_for(A)
    path = str(tmp_path_factory.mktemp("snap") / "a.convdr")
    A.save(path, window_rows=W)
    return A, Q, path


def test_a_reserved_load_takes_an_add_like_the_index_built_in_one_process(saved):
    A, Q, path = saved
    rows, _ = corpus(64, seed=9)
    more, more_ids = rows[:300], np.arange(300, dtype=np.int64) + 10 ** 9
    B = S.FlatIPIndex.load(path, reserve=2 * A.ntotal, prepin=False)
    assert B._reserved and B._s32.shape[0] == 2 * A.ntotal and B._sid.shape[0] == 2 * A.ntotal
    base = B._s32.data_ptr()
    B.add(more, ids=more_ids)
    assert B._s32.data_ptr() == base and B.ntotal == 1600                     # filled in place
    whole, _ = build("fp32", "auto", True, True, 64)
    whole.add(more, ids=more_ids)
    assert B.fingerprint() == whole.fingerprint()
    for k in (10, 5000):
        x, y = whole.search(Q, k), B.search(Q, k)
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    assert torch.equal(B.ids, whole.ids)


@pytest.mark.parametrize("precision", ("bf16", "fp16x3", "bf16x3", "fp16"))
def test_a_precision_override_returns_the_same_answers(saved, precision):
    A, Q, path = saved
    B = S.FlatIPIndex.load(path, precision=precision, prepin=False)
    assert B.precision == precision and (B._slo is not None) == precision.endswith("x3")
    assert bits(B._rows) == bits(A._rows) and bits(B._centre) == bits(A._centre)
    assert B._scale == (1.0 if B.kind == "bf16" else A._scale)
    for k in (10, 5000):
        x, y = A.search(Q, k), B.search(Q, k)
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), k


def test_a_half_store_takes_its_own_precisions_and_refuses_the_others(tmp_path):
    A, Q = build("fp16", "auto", True, False, 64)
    path = str(tmp_path / "h.convdr")
    A.save(path, window_rows=W)
    B = S.FlatIPIndex.load(path, precision="fp16x2", prepin=False)
    assert B.precision == "fp16x2" and torch.equal(B.store, A.store) and B._scale == A._scale
    x, y = A.search(Q, 10), B.search(Q, 10)
    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    with pytest.raises(ValueError):
        S.FlatIPIndex.load(path, precision="bf16", prepin=False)


def test_a_slice_of_the_rows_is_one_ranks_share(saved):
    A, Q, path = saved
    B = S.FlatIPIndex.load(path, rows=(256, 768), prepin=False)
    assert B.ntotal == 512 and np.array_equal(B.reconstruct_n(0, 512), A.reconstruct_n(256, 512))
    assert torch.equal(B.ids, A.ids[256:768]) and B._scale == A._scale and bits(B._max_norm) == bits(A._max_norm)
    assert bits(B._centre) == bits(A._centre) and torch.equal(B._pbf, A._pbf[256:768])
    mask = np.zeros(A.ntotal, dtype=bool)
    mask[256:768] = True
    for k in (10, 600):
        Da, Ia = A.search(Q, k, allowed=mask)
        Db, Ib = B.search(Q, k)
        assert np.array_equal(Da, Db) and np.array_equal(np.where(Ia >= 0, Ia - 256, Ia), Ib), k
    tail = S.FlatIPIndex.load(path, rows=(1024, 1300), prepin=False)          # r1 == n: the short last window
    assert np.array_equal(tail.reconstruct_n(0, 276), A.reconstruct_n(1024, 276))
    none = S.FlatIPIndex.load(path, rows=(512, 512), prepin=False)
    assert none.ntotal == 0
    for bad in ((100, 768), (256, 700), (0, 1301), (768, 256), (-256, 256)):
        with pytest.raises(ValueError, match="window_rows"):
            S.FlatIPIndex.load(path, rows=bad, prepin=False)


@pytest.mark.parametrize("storage,with_ids", (("fp32", False), ("fp32", True), ("fp16", False)))
def test_the_empty_index_round_trips(tmp_path, storage, with_ids):
    A = make_index(storage, "auto", with_ids, True, 100)
    if with_ids:                                             # an index that HAD rows with ids and lost them all
        A.add(corpus(100)[0][:40], ids=np.arange(40, dtype=np.int64))
        assert A.remove_ids(np.arange(40, dtype=np.int64)) == 40
    path = str(tmp_path / "e.convdr")
    A.save(path)
    assert S.verify_snapshot(path)["n"] == 0
    B = S.FlatIPIndex.load(path, prepin=False)
    assert B.ntotal == 0 and B.fingerprint() == A.fingerprint()
    rows, Q = corpus(100)
    for idx in (A, B):
        idx.add(rows[:300], ids=np.arange(300, dtype=np.int64) if with_ids else None)
    assert B.fingerprint() == A.fingerprint()
    x, y = A.search(Q, 10), B.search(Q, 10)
    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


# ---- corruption, and the staging buffers a save shares with every add ---------------------------------------------------
def test_a_flipped_byte_and_a_truncated_file_make_load_raise_and_name_the_window(saved, tmp_path):
    A, Q, path = saved
    raw = open(path, "rb").read()
    sec = S.snapshot_info(path)["sections"]["rows"]
    at = sec["offset"] + 4 * W * sec["row_bytes"] + 1001                      # inside window 4 of the rows
    flipped = str(tmp_path / "flipped.convdr")
    with open(flipped, "wb") as f:
        f.write(raw[:at] + bytes([raw[at] ^ 0x40]) + raw[at + 1:])
    with pytest.raises(_lib.ConvdrError, match=r"section 'rows', window 4:"):
        S.FlatIPIndex.load(flipped, prepin=False)
    with pytest.raises(_lib.ConvdrError, match=r"section 'rows', window 4:"):
        S.verify_snapshot(flipped)
    B = S.FlatIPIndex.load(flipped, verify=False, prepin=False)
    assert B.ntotal == A.ntotal and B.fingerprint() != A.fingerprint()
    ok = S.FlatIPIndex.load(flipped, rows=(0, 1024), prepin=False)           # only the covered windows are verified
    assert ok.ntotal == 1024
    cut = str(tmp_path / "cut.convdr")
    with open(cut, "wb") as f:
        f.write(raw[:sec["offset"] + 2 * W * sec["row_bytes"] + 17])
    with pytest.raises(_lib.ConvdrError, match=r"truncated file: section 'rows'.*from window 2 on"):
        S.FlatIPIndex.load(cut, prepin=False)
    with pytest.raises(_lib.ConvdrError, match="truncated"):
        S.FlatIPIndex.load(cut, verify=False, prepin=False)


def test_a_failed_save_leaves_the_existing_snapshot_untouched(saved, tmp_path):
    A, Q, path = saved
    raw = open(path, "rb").read()
    with pytest.raises(OSError):
        A.save(str(tmp_path / "missing" / "a.convdr"), window_rows=W)
    assert open(path, "rb").read() == raw
    A.save(path, window_rows=W)                              # (and a second save of the same index writes the same bytes)
    assert open(path, "rb").read() == raw


@pytest.mark.parametrize("order", ("save_then_add", "add_then_save"))
def test_a_save_and_a_streamed_add_share_the_staging_buffers_and_keep_their_bytes(tmp_path, order):
    """The pinned staging buffers and their events are process-wide: a save right behind a streamed add (its last H2D copies
    still in flight) and a streamed add right behind a save must each leave the other's bytes alone."""
    rs = np.random.RandomState(11)
    block = rs.randn(9000, 768).astype(np.float32)          # 27 MB: streamed through 4 x 2.7 MB buffers below
    alone = S.FlatIPIndex(768, prepin=False)
    alone.host_chunk_bytes = 2700 * 1024
    alone.add(block)
    want = alone._p32.clone()
    A, _ = build("fp32", "auto", True, True, 768)
    A.host_chunk_bytes = 2700 * 1024
    fp = A.fingerprint()
    path = str(tmp_path / "a.convdr")
    other = S.FlatIPIndex(768, prepin=False)
    other.host_chunk_bytes = 2700 * 1024
    if order == "save_then_add":
        A.save(path, window_rows=W)
        other.add(block)
    else:
        other.add(block)
        A.save(path, window_rows=W)
    assert torch.equal(other._p32, want) and torch.equal(other._pbf, alone._pbf)
    S.verify_snapshot(path)
    assert S.FlatIPIndex.load(path, prepin=False).fingerprint() == fp == A.fingerprint()
