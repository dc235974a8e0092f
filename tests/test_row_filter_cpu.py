"""Row filter, the parts that need no GPU: the bit layout of the packed mask, and every refusal of
convdr_ip_search_filtered (argument validation happens before anything touches a device)."""
import os
import re

import numpy as np
import pytest
import torch

from convdr_amd import _lib
from convdr_amd.search import ROW_FILTER_TILE, RowFilter, pack_row_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "convdr_ip_search_filtered"


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 255, 256, 257, 300, 5000])
@pytest.mark.parametrize("dtype", [np.bool_, np.uint8])
def test_packed_mask_is_numpy_packbits_little_viewed_as_uint32(n, dtype):
    """Row r is allowed iff bit r & 31 of word r >> 5 is set; the bitmap is zero padded to whole 256-row tiles."""
    mask = (np.random.RandomState(n).rand(n) < 0.4)
    if n > 40:
        mask[[31, 32, 63, 64]] = [True, False, False, True]
    if dtype is np.uint8:
        mask = mask.astype(np.uint8) * 7            # any non-zero value allows the row
    bits = pack_row_mask(torch.from_numpy(mask))
    padded = np.zeros((n + ROW_FILTER_TILE - 1) // ROW_FILTER_TILE * ROW_FILTER_TILE, bool)
    padded[:n] = mask != 0
    want = np.packbits(padded, bitorder="little").view(np.uint32)
    assert bits.dtype == torch.int32 and bits.numel() == (n + 255) // 256 * 8
    np.testing.assert_array_equal(bits.numpy().view(np.uint32), want)
    for r in range(0, n, 37):
        assert bool((int(want[r >> 5]) >> (r & 31)) & 1) == bool(mask[r])
    f = RowFilter(bits, n, int((mask != 0).sum()))
    assert f.n == n and f.n_allowed == int(np.count_nonzero(mask))
    np.testing.assert_array_equal(f.rows().numpy(), np.flatnonzero(mask))


def _call(L, store=1, deep=0, p_half_lo=None, scale=4.0, two_pass=0, n=100000, d=768, k=100, cap=4096, bits=1 << 20, words=None,
          n_allowed=None):
    """Every pointer but the bitmap is NULL and the workspace has 0 bytes: a call that got past validation could not return
    these messages.  (The bitmap pointer is never dereferenced on the host.)"""
    words = (n + 255) // 256 * 8 if words is None else words
    n_allowed = n // 2 if n_allowed is None else n_allowed
    return L.convdr_ip_search_filtered(store, deep, None, 5, None, None, p_half_lo, scale, two_pass, n, d, k, None, None, cap, 0,
                                       None, 0, bits, words, n_allowed, None, None, None, None, None)


@pytest.mark.parametrize("deep,cap,big_k", [(0, 4096, 2049), (1, 16384, 8193)])
@pytest.mark.parametrize("store", [0, 1, 2])
def test_every_refusal_is_a_negative_code_with_a_message(store, deep, cap, big_k):
    L = _lib.lib()
    cases = [
        ({"bits": None}, b"row_bits is NULL"),
        ({"bits": (1 << 20) + 4}, b"16-byte aligned"),
        ({"words": 100000 // 256 * 8}, b"the bitmap holds"),            # one tile short (100,000 rows: 391 tiles)
        ({"words": 0}, b"the bitmap holds"),
        ({"n_allowed": -1}, b"n_allowed"),
        ({"n_allowed": 100001}, b"n_allowed"),
        ({"store": 3}, b"store must be"),
        ({"store": -1}, b"store must be"),
        ({"deep": 2}, b"store must be"),
        ({"n": 1 << 31, "words": 1 << 30}, b"bad block size"),
        ({"two_pass": 2}, b"two_pass"),
        # the matching entry's size contracts
        ({"d": 70}, b"d % 64"),
        ({"k": big_k}, b"too large for cap"),
        ({"cap": 5000}, b"cap must be a power of two"),
        ({"k": 0}, b"bad sizes"),
    ]
    if store != 2:
        cases.append(({"two_pass": 1}, b"two_pass"))
    else:
        cases += [({"p_half_lo": 1 << 20}, b"no remainder copy"), ({"scale": 0.5}, b"power of two >= 1")]
    if store != 0:
        cases.append(({"scale": 0.75}, b"power of two"))
    for kw, msg in cases:
        rc = _call(L, **{"store": store, "deep": deep, "cap": cap, **kw})
        assert rc < 0 and msg in L.convdr_last_error(), (kw, rc, L.convdr_last_error())
    # the first check past all of them, for n_allowed at both ends of its range and in the one-pass regime
    for n_allowed in (0, 1, 100000):
        assert _call(L, store=store, deep=deep, cap=cap, n_allowed=n_allowed) < 0 and b"workspace too small" in L.convdr_last_error()


def test_header_ctypes_and_exports_agree_on_the_entry():
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "convdr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(convdr_[a-z0-9_]+)\s*\(", src))
    assert NAME in declared and NAME in _lib.exported_symbols() and hasattr(L, NAME)
    params = re.search(r"\b%s\s*\(([^)]*)\)" % NAME, src).group(1)
    assert len(params.split(",")) == len(_lib._SIGNATURES[NAME][1])
    for word in ("row_bits", "row_bits_words", "n_allowed"):
        assert word in params


def test_search_methods_take_the_keyword_and_the_unfiltered_handle_is_unchanged():
    import inspect
    from convdr_amd import search as S
    for name in ("search", "search_tensors", "search_begin", "search_device", "search_deep_device"):
        assert inspect.signature(getattr(S.FlatIPIndex, name)).parameters["allowed"].default is None, name
    for name in ("search_distinct",):                       # out of scope: it does not take the keyword
        assert "allowed" not in inspect.signature(getattr(S.FlatIPIndex, name)).parameters
    assert S._Pending(1, 2, 3, 4, 5, 6).allowed is None


def test_the_filter_rides_through_every_rung_of_the_ladder():
    """The ladder without a GPU (the scripted stub of test_search_ladder_cpu): first pass, RANGE rebuild, retries, the split rung
    and the last rung all receive the handle's RowFilter; without one, no call receives the keyword at all."""
    from tests.test_search_ladder_cpu import DEEP_K, OK, RANGE, SHALLOW_K, UNCERTAIN, LadderStub

    class Stub(LadderStub):
        seen = None

        def _note(self, kw):
            self.seen.append(kw.get("allowed", "absent"))

        def search_device(self, q, k, tau_in=None, cap=None, x3=None, **kw):
            self._note(kw)
            return LadderStub.search_device(self, q, k, tau_in, cap, x3)

        def search_deep_device(self, q, k, tau_in=None, cap=None, x3=False, **kw):
            self._note(kw)
            return LadderStub.search_deep_device(self, q, k, tau_in, cap, x3)

        def _search_exhaustive(self, q, k, **kw):
            self._note(kw)
            return LadderStub._search_exhaustive(self, q, k)

        def _search_large_k(self, q, k, **kw):
            self._note(kw)
            return LadderStub._search_large_k(self, q, k)

    for k in (SHALLOW_K, DEEP_K):
        for use in (True, False):
            s = Stub(n=100000, script=[[RANGE, OK, UNCERTAIN, UNCERTAIN]], default=UNCERTAIN, counts=([5] * 4, [1] * 4))
            s.seen = []
            f = RowFilter(torch.zeros(100000 // 256 * 8 + 8, dtype=torch.int32), 100000, 50000) if use else None
            s.search_finish(s.search_begin(torch.zeros(4, 64), k, allowed=f))
            routes = [t[0] for t in s.trace]
            assert "rebuild" in routes and routes[-1] in ("exhaustive", "large_k") and len(s.seen) > 8, s.trace
            assert all(a is f for a in s.seen) if use else all(a == "absent" for a in s.seen), s.seen
    # a filter that allows nothing: padding, and nothing is enqueued
    s = Stub(n=100000)
    s.seen = []
    D, I = s.search_finish(s.search_begin(torch.zeros(4, 64), SHALLOW_K, allowed=RowFilter(torch.zeros(3128, dtype=torch.int32), 100000, 0)))
    assert s.seen == [] and bool((I == -1).all()) and bool((D == torch.finfo(torch.float32).min).all())
    with pytest.raises(ValueError):
        s.search_begin(torch.zeros(4, 64), SHALLOW_K, allowed=RowFilter(torch.zeros(8, dtype=torch.int32), 99999, 5))
