"""Deep top-k (4096 < k <= 65536) without a GPU: argument validation of the new entry points, the workspace size, the header /
export / binding triple, and the merge rule search_one_by_one uses for lists longer than convdr_topk_merge takes."""
import os
import re

import numpy as np

from convdr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("convdr_ip_search_deep", "convdr_ip_search_deep_f16", "convdr_ip_deep_workspace_bytes")


def _deep(L, f16, nq=3, n=100_000, d=64, k=5000, cap=32768, ws_bytes=None):
    """One call with null pointers: only the argument checks may run."""
    if ws_bytes is None:
        ws_bytes = 1 << 40
    head = (None, nq, None, None, None)
    tail = (n, d, k, None, None, cap, 0, None, ws_bytes, None, None, None, None, None)
    if f16:
        return L.convdr_ip_search_deep_f16(*head, 1.0, *tail)
    return L.convdr_ip_search_deep(*head, *tail)


def test_deep_argument_validation_needs_no_gpu():
    L = _lib.lib()
    for f16 in (False, True):
        for what, kw in (("cap", dict(cap=8192, k=100)),                  # below the deep range (the shallow call's)
                         ("cap", dict(cap=262144)),                       # above it
                         ("cap", dict(cap=40000)),                        # not a power of two
                         ("too large for cap", dict(cap=16384, k=8193)),  # k = cap / 2 + 1
                         ("bad sizes", dict(k=0)),
                         ("d % 64", dict(d=72)),
                         ("2^31", dict(n=1 << 31))):
            assert _deep(L, f16, **kw) != 0, (f16, kw)
            err = L.convdr_last_error()
            assert b"convdr_ip_search_deep: " in err and what.encode() in err, (kw, err)
        need = L.convdr_ip_deep_workspace_bytes(3, 100_000, 64, 5000, 32768)
        assert need > 0
        assert _deep(L, f16, ws_bytes=need - 1) != 0
        assert b"workspace too small" in L.convdr_last_error()
    assert L.convdr_ip_search_deep_f16(None, 3, None, None, None, 3.0, 100_000, 64, 5000, None, None, 32768, 0, None, 1 << 40,
                                       None, None, None, None, None) != 0
    assert b"power of two" in L.convdr_last_error()
    # the shallow entry points keep their own bounds
    assert L.convdr_ip_search(None, 3, None, None, None, 100_000, 64, 5000, None, None, 16384, 0, None, 1 << 40, None, None, None,
                              None, None) != 0
    assert b"[1024, 8192]" in L.convdr_last_error()


def test_deep_workspace_bytes_is_positive_and_monotone():
    L = _lib.lib()
    ws = L.convdr_ip_deep_workspace_bytes
    caps = (16384, 32768, 65536, 131072)
    for n in (0, 10_000, 140_000, 1_000_000, 38_000_000):
        last_q = 0
        for nq in (1, 2, 100, 128, 129, 1000):
            b = [ws(nq, n, 768, 4097, cap) for cap in caps]
            assert all(x > 0 for x in b) and b == sorted(b), (n, nq, b)
            assert b[0] >= last_q, (n, nq)
            last_q = b[0]
            assert b[-1] >= nq * 131072 * 28                # the documented per-slot cost
    # outside the contract: no size
    assert ws(0, 1000, 64, 10, 16384) == 0 and ws(1, 1000, 64, 10, 8192) == 0 and ws(1, 1000, 64, 8193, 16384) == 0
    assert ws(1, 1 << 31, 64, 10, 16384) == 0 and ws(1, 1000, 70, 10, 16384) == 0
    # the documented bound: 1,000 queries at the largest list are under 4 GiB apart from the sample
    assert ws(1000, 100_000, 768, 65536, 131072) < (4 << 30)


def test_header_exports_and_bindings_agree_on_the_deep_entry_points():
    L = _lib.lib()
    src = open(os.path.join(ROOT, "include", "convdr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(convdr_[a-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared, "%s is not declared in include/convdr_hip.h" % name
        assert hasattr(L, name), "libconvdr_hip.so does not export %s" % name
        assert name in _lib.exported_symbols()
    assert declared == set(_lib.exported_symbols()), declared ^ set(_lib.exported_symbols())
    assert L.convdr_ip_search_deep.argtypes == L.convdr_ip_search.argtypes
    assert L.convdr_ip_search_deep_f16.argtypes == L.convdr_ip_search_f16.argtypes


def test_long_lists_merge_as_the_stable_sort_of_the_concatenation():
    """merge_topk_device hands lists longer than convdr_topk_merge's 4096 to merge_topk_sorted; on CPU tensors that helper must
    give the permutation of search.merge_topk (ties keep the earlier block, each list its own order)."""
    import torch
    from convdr_amd import search
    assert search.MERGE_KERNEL_MAX == 4096
    rs = np.random.RandomState(5)
    nq, topN = 3, 5000
    for na, nb in ((topN, topN), (2 * topN, topN), (topN, 4100)):
        # few distinct values: long runs of ties inside and across the lists
        Da = -np.sort(-rs.randint(0, 300, (nq, na)).astype(np.float32), axis=1)
        Db = -np.sort(-rs.randint(0, 300, (nq, nb)).astype(np.float32), axis=1)
        Db[:, nb - 7:] = search.PAD_SCORE
        Ia = rs.randint(0, 1 << 40, (nq, na)).astype(np.int64)
        Ib = rs.randint(0, 1 << 40, (nq, nb)).astype(np.int64)
        Ib[:, nb - 7:] = -1
        Dr, Ir = search.merge_topk((Da, Ia), (Db, Ib), topN)
        t = [torch.from_numpy(x) for x in (Da[:, :topN], Ia[:, :topN], Db[:, :topN], Ib[:, :topN])]
        D, I = search.merge_topk_sorted(*t)
        np.testing.assert_array_equal(D.numpy(), Dr)
        np.testing.assert_array_equal(I.numpy(), Ir)
        assert D.dtype == torch.float32 and I.dtype == torch.int64


def test_deep_route_constants():
    from convdr_amd.search import FlatIPIndex
    assert FlatIPIndex.MAX_K == 4096 and FlatIPIndex.DEEP_MAX_K == 65536
    assert FlatIPIndex.DEEP_WS_BYTES == 4 << 30
    cap = FlatIPIndex._deep_cap
    # between 2k and 4k entries, a power of two the kernel takes
    for k in (4097, 5000, 8192, 8193, 20000, 32768, 32769, 65536):
        c = cap(FlatIPIndex, k)
        assert 16384 <= c <= 131072 and c & (c - 1) == 0 and 2 * k <= c and (c <= 4 * k), (k, c)
    assert cap(FlatIPIndex, 4097) == 16384 and cap(FlatIPIndex, 20000) == 65536 and cap(FlatIPIndex, 65536) == 131072
