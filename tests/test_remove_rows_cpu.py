"""Removing rows, the parts that need no GPU: the three convdr_ip_compact_* entries are declared and exported, every refusal
(argument validation happens before anything touches a device), the workspace size against the documented region order, and
the argument checks of FlatIPIndex.keep_rows / remove_rows / reconstruct* against a scripted index."""

import numpy as np
import pytest
import torch

from convdr_amd import _lib
from convdr_amd import search as S
from tests import capi_decl

ENTRIES = ("convdr_ip_compact_workspace_bytes", "convdr_ip_compact_plan", "convdr_ip_compact_rows")
N = 100000
WORDS = (N + 255) // 256 * 8
BITS = 1 << 20                  # a pointer that is never dereferenced on the host


def test_header_ctypes_and_exports_agree_on_the_entries():
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.exported_symbols() and hasattr(L, name)
        assert len(capi_decl.params(name).split(",")) == len(_lib._SIGNATURES[name][1]), name


def _rows(L, row_bytes=3072, n=N, bits=BITS, words=WORDS, window=1024):
    """rows and workspace are NULL and the workspace has 0 bytes: a call that got past validation could not return these messages"""
    return L.convdr_ip_compact_rows(None, row_bytes, n, bits, words, window, None, 0, None)


def _plan(L, n=N, bits=BITS, words=WORDS):
    return L.convdr_ip_compact_plan(bits, words, n, None, 0, None, None)


def test_every_refusal_of_the_rows_entry_is_a_negative_code_with_a_message():
    L = _lib.lib()
    cases = [
        ({"row_bytes": 3080}, b"row_bytes % 16"),
        ({"row_bytes": 8}, b"row_bytes % 16"),
        ({"row_bytes": 0}, b"row_bytes % 16"),
        ({"row_bytes": 65552}, b"row_bytes % 16"),
        ({"n": -1}, b"bad block size"),
        ({"n": 1 << 31}, b"bad block size"),
        ({"window": 1000}, b"window_rows must be a multiple of 256"),
        ({"window": 0}, b"window_rows must be a multiple of 256"),
        ({"window": -256}, b"window_rows must be a multiple of 256"),
        ({"window": (1 << 20) + 256}, b"window_rows must be a multiple of 256"),
        ({"bits": BITS + 4}, b"16-byte aligned"),
        ({"words": WORDS - 8}, b"the bitmap holds"),
        ({"bits": None, "words": 8}, b"keep_bits is NULL"),
    ]
    for kw, msg in cases:
        rc = _rows(L, **kw)
        assert rc < 0 and msg in L.convdr_last_error(), (kw, rc, L.convdr_last_error())
        assert b"convdr_ip_compact_rows" in L.convdr_last_error()
    # the first check past all of them
    for kw in ({}, {"row_bytes": 16}, {"row_bytes": 65536}, {"window": 256}, {"window": 1 << 20}, {"n": 0}, {"n": (1 << 31) - 1, "words": 1 << 26},
               {"bits": None, "words": 0}):
        assert _rows(L, **kw) < 0 and b"workspace too small" in L.convdr_last_error(), kw


def test_every_refusal_of_the_plan_entry_is_a_negative_code_with_a_message():
    L = _lib.lib()
    for kw, msg in (({"n": -1}, b"bad block size"), ({"n": 1 << 31}, b"bad block size"), ({"bits": BITS + 8}, b"16-byte aligned"),
                    ({"words": WORDS - 1}, b"the bitmap holds"), ({"bits": None, "words": 8}, b"keep_bits is NULL")):
        rc = _plan(L, **kw)
        assert rc < 0 and msg in L.convdr_last_error() and b"convdr_ip_compact_plan" in L.convdr_last_error(), (kw, L.convdr_last_error())
    for kw in ({}, {"n": 0}, {"n": 0, "bits": None, "words": 0}, {"bits": None, "words": 0}):
        assert _plan(L, **kw) < 0 and b"workspace too small" in L.convdr_last_error(), kw
    # a workspace that is large enough: the NULL pointers are the next refusal (still before any device work)
    assert L.convdr_ip_compact_plan(BITS, WORDS, N, None, 1 << 20, None, None) < 0 and b"NULL argument" in L.convdr_last_error()
    assert L.convdr_ip_compact_rows(None, 3072, N, BITS, WORDS, 1024, None, 1 << 30, None) < 0 and b"NULL argument" in L.convdr_last_error()
    # nothing to move: an empty block, or no bitmap (every row kept) -- no pointer is looked at
    assert L.convdr_ip_compact_rows(None, 3072, 0, None, 0, 1024, None, 1 << 30, None) == 0
    assert L.convdr_ip_compact_rows(None, 3072, N, None, 0, 1024, None, 1 << 30, None) == 0


def _up(x):
    return (x + 255) // 256 * 256


def _total(n, row_bytes, window):
    """the documented region order (include/convdr_hip.h, "Removing rows"), every region rounded up to 256 bytes"""
    tiles = (n + 255) // 256
    return _up((tiles + 1) * 4) + _up((tiles + 1 + 8191) // 8192 * 4) + _up(window * row_bytes)


def test_workspace_bytes_follow_the_documented_regions_and_are_zero_outside_the_contract():
    L = _lib.lib()
    ws = L.convdr_ip_compact_workspace_bytes
    for args, msg in (((100, 24, 256), b"row_bytes % 16"), ((100, 0, 256), b"row_bytes % 16"), ((100, 65552, 256), b"row_bytes % 16"),
                      ((-1, 64, 256), b"bad block size"), ((1 << 31, 64, 256), b"bad block size"), ((100, 64, 100), b"window_rows"),
                      ((100, 64, 0), b"window_rows"), ((100, 64, 1 << 21), b"window_rows")):
        assert ws(*args) == 0 and msg in L.convdr_last_error() and b"convdr_ip_compact_rows" in L.convdr_last_error(), args
    for n in (0, 1, 255, 256, 257, 1317, 5000, 8191 * 256, 8191 * 256 + 1, 8192 * 256, 1_000_000, 38_000_000, (1 << 31) - 1):
        for row_bytes in (16, 1536, 3072, 65536):
            for window in (256, 512, 16384, 1 << 20):
                assert ws(n, row_bytes, window) == _total(n, row_bytes, window), (n, row_bytes, window)
    # the plan needs the regions before the bounce buffer and nothing more
    need = _total(N, 16, 256) - _up(256 * 16)
    assert L.convdr_ip_compact_plan(BITS, WORDS, N, None, need - 1, None, None) < 0 and b"workspace too small" in L.convdr_last_error()
    assert L.convdr_ip_compact_plan(BITS, WORDS, N, None, need, None, None) < 0 and b"NULL argument" in L.convdr_last_error()


# ---- the Python argument checks against a scripted index ---------------------------------------------------------------
class CompactStub(S.FlatIPIndex):
    """FlatIPIndex with the attributes keep_rows / remove_rows / reconstruct* read, on the CPU; _compact is a recorder (the
    bitmap arrives unpacked: the rows the device would keep)."""

    def __init__(self, n=1000, d_in=60, half=False, scale=4.0):
        self.device = torch.device("cpu")
        self.kind, self._store = "f16", S.STORES["fp16" if half else "fp32"]
        self._n, self.d_in, self.d = int(n), d_in, 64
        self.compact_window_rows = 512
        self.stats = {}
        self._scale = scale if half else 1.0
        rows = torch.arange(n * 64, dtype=torch.float32).reshape(n, 64) % 1000
        self._s32 = None if half else rows
        self._s16 = (rows * scale).half() if half else rows.half()
        self._slo = None
        self.trace = []

    def _compact(self, f, window_rows):
        self.trace.append((f.rows().tolist(), f.n_allowed, window_rows))


def test_keep_rows_checks_its_mask_and_its_filter_before_any_device_work():
    idx = CompactStub()
    for bad in (np.ones(999, bool), np.ones(1001, np.uint8), np.ones((1000, 1), bool), np.ones((2, 500), bool), None):
        with pytest.raises(ValueError):
            idx.keep_rows(bad)
    with pytest.raises(ValueError, match="stale"):
        idx.keep_rows(S.RowFilter(torch.zeros(32, dtype=torch.int32), 999, 5))
    idx.compact_window_rows = 1000
    with pytest.raises(ValueError, match="compact_window_rows"):
        idx.keep_rows(np.ones(1000, bool))
    assert idx.trace == [] and idx.ntotal == 1000
    idx.compact_window_rows = 512
    # nothing removed: no device work, filters stay valid
    f = idx.row_filter(np.ones(1000, bool))
    assert idx.keep_rows(f) == 0 and idx.trace == [] and idx.ntotal == 1000
    assert idx.stats == {"removed": 0, "compact_windows": 0}
    keep = np.ones(1000, np.uint8)
    keep[[0, 31, 32, 999]] = 0
    assert idx.keep_rows(keep) == 4 and idx.ntotal == 996
    assert idx.trace == [([r for r in range(1000) if keep[r]], 996, 512)]
    assert idx.stats == {"removed": 4, "compact_windows": 2}
    with pytest.raises(ValueError, match="stale"):            # the filter of the old ntotal
        idx.keep_rows(f)


def test_remove_rows_checks_ids_and_masks_and_leaves_the_index_unchanged():
    idx = CompactStub()
    for bad in (np.array([0, 1000]), np.array([-1, 5]), torch.tensor([999, 1 << 40]), [3, 1000, 3]):
        with pytest.raises(ValueError, match="ntotal"):
            idx.remove_rows(bad)
    for bad in (np.zeros(999, bool), np.zeros(1001, np.uint8), np.zeros((1000, 1), bool), np.zeros(3, np.float32),
                np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError):
            idx.remove_rows(bad)
    assert idx.trace == [] and idx.ntotal == 1000
    assert idx.remove_rows(np.zeros(0, np.int64)) == 0 and idx.remove_rows(np.zeros(1000, bool)) == 0 and idx.trace == []
    # ids with duplicates, and the remove mask of the same rows
    gone = [5, 999, 5, 0, 256, 255, 5]
    assert idx.remove_rows(np.asarray(gone)) == 5 and idx.ntotal == 995
    left = [r for r in range(1000) if r not in gone]
    assert idx.trace == [(left, 995, 512)]
    idx2 = CompactStub()
    mask = np.zeros(1000, np.uint8)
    mask[gone] = 7
    assert idx2.remove_rows(torch.as_tensor(mask)) == 5 and idx2.trace == idx.trace
    with pytest.raises(ValueError):
        CompactStub(n=0).remove_rows(np.array([0]))


@pytest.mark.parametrize("half", [False, True])
def test_reconstruct_checks_ids_and_cuts_the_padding_columns(half):
    idx = CompactStub(half=half)
    want = (torch.arange(1000 * 64, dtype=torch.float32).reshape(1000, 64) % 1000).half().float().numpy()[:, :60]
    if not half:
        want = idx._s32.numpy()[:, :60]
    for call, bad in ((idx.reconstruct, 1000), (idx.reconstruct, -1), (idx.reconstruct_batch, np.array([0, 1000])),
                      (idx.reconstruct_batch, np.array([-1])), (idx.rows_tensors, torch.tensor([[1, 2], [3, 1000]])),
                      (idx.reconstruct_batch, np.array([0.5]))):
        with pytest.raises(IndexError):
            call(bad)
    for i0, ni in ((0, 1001), (999, 2), (-1, 2), (5, -1), (1001, 0)):
        with pytest.raises(IndexError):
            idx.reconstruct_n(i0, ni)
    got = idx.reconstruct(7)
    assert got.dtype == np.float32 and got.shape == (60,) and np.array_equal(got, want[7])
    assert np.array_equal(idx.reconstruct_n(998, 2), want[998:]) and idx.reconstruct_n(1000, 0).shape == (0, 60)
    ids = np.array([5, 5, 999, 0])
    assert np.array_equal(idx.reconstruct_batch(ids), want[ids])
    t = idx.rows_tensors(torch.tensor([[1, 2], [3, 4]]))
    assert t.shape == (2, 2, 60) and t.dtype == torch.float32 and np.array_equal(t.numpy(), want[[[1, 2], [3, 4]]])
    assert idx.reconstruct_batch(np.zeros(0, np.int64)).shape == (0, 60)
