"""Ranked lists (D scores, I ids [nq, n]) without an index: the reference's two-way merge and its first-occurrence-per-key walk,
on the host and on the device (convdr_topk_merge, convdr_topk_distinct[_deep]), and the depth limits the lists share with the index."""
import numpy as np

from . import _lib

PAD_SCORE = -3.4028234663852886e38      # what IndexFlatIP.search returns beside id -1

MAX_K, DEEP_MAX_K = 4096, 65536      # convdr_ip_search / _deep: k <= cap / 2, cap <= 8192 / 131072 (FlatIPIndex.MAX_K, .DEEP_MAX_K)
DEEP_WS_BYTES = 4 << 30              # most workspace one deep call may ask for (FlatIPIndex.DEEP_WS_BYTES)


def split_under(ws_bytes, count, budget):
    """(items per call, workspace bytes of one such call): the items of one request -- queries, (query, row) pairs -- are halved
    until ws_bytes(items), the entry's own workspace function, fits `budget` (None: never split); the calls then run back to
    back on the stream and share the buffer.  A single item is never split, and 0 bytes means sizes outside the entry's
    contract: the caller raises, in its own words."""
    step = count
    while budget is not None and step > 1 and ws_bytes(step) > budget:
        step = (step + 1) // 2
    return step, ws_bytes(step)


def merge_topk(merged, cand, topN):
    """The reference's two-way list merge (run_convdr_inference.py:213-229) for all queries at
    once.  merged/cand: (D float64 [nq, >=topN], I int64 [nq, >=topN]), rows sorted descending.
    The reference walks two pointers until one list is exhausted and then appends the other
    list's remainder -- i.e. a complete merge of the two sorted topN-lists in which ties keep the
    earlier block first (`>=`, :218) -- and returns all 2*topN entries.  A stable sort of the
    concatenation on descending score is that same permutation."""
    aD = np.concatenate([merged[0][:, :topN], cand[0][:, :topN]], axis=1)
    aI = np.concatenate([merged[1][:, :topN], cand[1][:, :topN]], axis=1)
    order = np.argsort(-aD, axis=1, kind="stable")
    return np.take_along_axis(aD, order, 1), np.take_along_axis(aI, order, 1)


MERGE_KERNEL_MAX = 4096      # convdr_topk_merge: na, nb <= 4096


def merge_topk_sorted(Da, Ia, Db, Ib):
    """``merge_topk`` as torch operations on whatever device the lists live on: the stable descending sort of [A, B] --
    ties keep A (the earlier blocks) first, each list keeps its own order.  For lists longer than convdr_topk_merge
    takes (topN > 4096, once per block file: not a hot path)."""
    import torch
    aD, aI = torch.cat([Da, Db], dim=1), torch.cat([Ia, Ib], dim=1)
    order = torch.sort(aD, dim=1, descending=True, stable=True).indices
    return torch.gather(aD, 1, order), torch.gather(aI, 1, order)


def merge_topk_device(merged, cand, topN):
    """``merge_topk`` on the device: (D fp32 [nq, na], I int64 [nq, na]) torch tensors in and out, same permutation
    (convdr_topk_merge: A before B on equal scores, each list in its own order; lists longer than MERGE_KERNEL_MAX take
    merge_topk_sorted)."""
    import torch
    Da, Ia = merged[0][:, :topN], merged[1][:, :topN]
    Db, Ib = cand[0][:, :topN], cand[1][:, :topN]
    nq, na, nb = Da.shape[0], Da.shape[1], Db.shape[1]
    if na > MERGE_KERNEL_MAX or nb > MERGE_KERNEL_MAX:
        return merge_topk_sorted(Da, Ia, Db, Ib)
    Do = torch.empty((nq, na + nb), dtype=torch.float32, device=Da.device)
    Io = torch.empty((nq, na + nb), dtype=torch.int64, device=Da.device)
    with torch.cuda.device(Da.device):
        _lib.check(_lib.lib().convdr_topk_merge(_lib.ptr(Da), _lib.ptr(Ia), na, Da.stride(0), _lib.ptr(Db), _lib.ptr(Ib), nb,
                                                Db.stride(0), nq, na + nb, _lib.ptr(Do), _lib.ptr(Io), Do.stride(0),
                                                _lib.stream_ptr()), "convdr_topk_merge")
    return Do, Io


def distinct_topk(D, I, k, key_map=None):
    """The reference's `seen_pid` walk (run_convdr_inference.py:58-69) over ranked lists, as array operations: the numpy
    restatement of convdr_topk_distinct (include/convdr_hip.h) for the host path.  D / I: [nq, n] scores and ids, every row a
    ranked list; key = key_map[I] (or I).  Entries with I < 0 are dropped; an entry is kept iff no earlier one has its key.
    Returns (D [nq, k] in D's dtype, I int64 [nq, k], K int64 [nq, k], counts int32 [nq, 2] = (n_distinct, n_valid));
    slots past a row's last key hold (-3.4028235e38, -1, -1); n_distinct = -1 for a row with an I >= len(key_map)."""
    D, I = np.asarray(D), np.asarray(I, dtype=np.int64)
    nq, k = I.shape[0], int(k)
    km = None if key_map is None else np.asarray(key_map, dtype=np.int64)
    Do = np.full((nq, k), PAD_SCORE, D.dtype)
    Io = np.full((nq, k), -1, np.int64)
    Ko = np.full((nq, k), -1, np.int64)
    counts = np.zeros((nq, 2), np.int32)
    for j in range(nq):
        valid = I[j] >= 0
        oob = False
        if km is not None:
            over = I[j] >= len(km)
            oob = bool((valid & over).any())
            valid &= ~over
        pos = np.nonzero(valid)[0]
        ids = I[j, pos]
        keys = ids if km is None else km[ids]
        _, first = np.unique(keys, return_index=True)       # first occurrence of every key ...
        first.sort()                                        # ... in rank order
        keep = first[:k]
        Do[j, :len(keep)] = D[j, pos[keep]]
        Io[j, :len(keep)] = ids[keep]
        Ko[j, :len(keep)] = keys[keep]
        counts[j] = (-1 if oob else len(first), len(pos))
    return Do, Io, Ko, counts


DISTINCT_KERNEL_MAX = 4096   # convdr_topk_distinct: n, n_out <= 4096 (keys and table in LDS)
DISTINCT_DEEP_WS_BYTES = None   # most workspace one convdr_topk_distinct_deep call may ask for (None: DEEP_WS_BYTES)


def distinct_topk_device(D, I, k, key_map=None):
    """``distinct_topk`` on the device, no sync: D fp32 / I int64 [nq, n <= 65536] torch tensors with unit column stride,
    key_map None or a device int64 vector.  Returns device (D, I, K [nq, k], counts [nq, 2]).
    n, k <= 4096: convdr_topk_distinct, one launch.  Beyond: convdr_topk_distinct_deep, whose keys and table live in a
    workspace allocated per call (n * 8 + at most 4n * 4 bytes per query: 1 MB at n = 65,536); the queries are split so that
    one call never asks for more than DEEP_WS_BYTES (the calls run back to back on the stream and share it)."""
    import torch
    nq, n, k = int(D.shape[0]), int(D.shape[1]), int(k)
    assert D.dtype == torch.float32 and I.dtype == torch.int64 and D.shape == I.shape
    if n and nq and (D.stride(1) != 1 or I.stride(1) != 1 or D.stride(0) != I.stride(0)):
        D, I = D.contiguous(), I.contiguous()
    if key_map is not None:
        assert key_map.dtype == torch.int64 and key_map.dim() == 1 and key_map.device == D.device
        key_map = key_map.contiguous()
    Do = torch.empty((nq, k), dtype=torch.float32, device=D.device)
    Io = torch.empty((nq, k), dtype=torch.int64, device=D.device)
    Ko = torch.empty((nq, k), dtype=torch.int64, device=D.device)
    counts = torch.zeros((nq, 2), dtype=torch.int32, device=D.device)
    L = _lib.lib()
    ld, kml = max(int(D.stride(0)), n), 0 if key_map is None else key_map.numel()
    with torch.cuda.device(D.device):
        if n <= DISTINCT_KERNEL_MAX and k <= DISTINCT_KERNEL_MAX:
            _lib.check(L.convdr_topk_distinct(_lib.ptr(D), _lib.ptr(I), n, ld, nq, _lib.ptr(key_map), kml, k, _lib.ptr(Do),
                                              _lib.ptr(Io), _lib.ptr(Ko), k, _lib.ptr(counts), _lib.stream_ptr()),
                       "convdr_topk_distinct")
            return Do, Io, Ko, counts
        budget = DEEP_WS_BYTES if DISTINCT_DEEP_WS_BYTES is None else int(DISTINCT_DEEP_WS_BYTES)
        step, need = split_under(lambda c: L.convdr_topk_distinct_deep_workspace_bytes(c, n), max(nq, 1), budget)
        if n > DEEP_MAX_K or k > DEEP_MAX_K or not need:
            raise _lib.ConvdrError("convdr_topk_distinct_deep: sizes outside the contract (nq=%d n=%d n_out=%d)" % (nq, n, k))
        ws = torch.empty(need, dtype=torch.uint8, device=D.device)
        for a in range(0, nq, step):
            b = min(nq, a + step)
            _lib.check(L.convdr_topk_distinct_deep(_lib.ptr(D[a:b]), _lib.ptr(I[a:b]), n, ld, b - a, _lib.ptr(key_map), kml, k,
                                                   _lib.ptr(Do[a:b]), _lib.ptr(Io[a:b]), _lib.ptr(Ko[a:b]), k,
                                                   _lib.ptr(counts[a:b]), _lib.ptr(ws), need, _lib.stream_ptr()),
                       "convdr_topk_distinct_deep")
    return Do, Io, Ko, counts


def _check_max_depth(who, max_depth):
    """The row depth a distinct / sharded search may reach: FlatIPIndex.MAX_K unless the caller asks for more."""
    if max_depth is None:
        return MAX_K
    md = int(max_depth)
    if md < 1 or md > DEEP_MAX_K:
        raise ValueError("%s: max_depth = %d is outside 1..%d (FlatIPIndex.DEEP_MAX_K)" % (who, md, DEEP_MAX_K))
    return md


def _distinct_row_depth(who, topN, rows_per_key, limit, limit_name):
    """m = topN * rows_per_key, the row depth at which a walk over block files holds topN keys for every query."""
    m = topN * rows_per_key
    if topN < 1 or rows_per_key < 1 or m > limit:
        raise ValueError("%s: topN * rows_per_key = %d * %d = %d is outside 1..%d (%s)" % (who, topN, rows_per_key, m, limit, limit_name))
    return m
