"""Brute-force inner-product search over passage-embedding blocks on MI355X.

Mirrors, name for name, what the reference does with FAISS:
  * ``FlatIPIndex``         <-> ``faiss.IndexFlatIP(768)`` (+ ``index_cpu_to_gpu_multiple``)
                               /root/reference/drivers/run_convdr_inference.py:353-368,
                               ``.add`` :180, ``.search`` :182, ``.reset`` :202
  * ``search_one_by_one``   <-> run_convdr_inference.py:157-242 (same merge rule, same output shapes)
  * ``EvalDevQuery``        <-> run_convdr_inference.py:21-113  (same .trec / .jsonl text)
  * ``distinct_topk`` / ``FlatIPIndex.search_distinct`` / ``search_distinct_one_by_one``: the first-occurrence-per-pid walk
                               of EvalDevQuery (:58-69) moved in front of the cut to topN, certified exact -- document-level
                               results for blocks whose rows repeat a key (MaxP chunk rows, duplicate pids)
All scoring / selection runs in libconvdr_hip.so (csrc/ip_topk.hip).
"""
import collections
import functools

import numpy as np

from . import _lib
# (what lives in the modules this one was split into stays importable from here)
from .block_search import (EvalDevQuery, _check_distinct_certificate, _load_collection, _Passages, _search_block_list, load_block,
                           search_distinct_one_by_one, search_one_by_one)
from .index_store import (_HALF_PRECISIONS, _KINDS, EXCLUDE_MAX, HALF_NORM_LIMIT, KEY_ST_COLUMN, KEY_ST_LIST, KEY_ST_NOSET, KEY_ST_PROBE,
                          RESERVED_ID, ROW_FILTER_TILE, STORES, DocOrdinals, QueryExclusions, RowFilter, _IndexStore, pack_exclusions, pack_row_mask)
from .snapshot import read_header as snapshot_info, verify_file as verify_snapshot
from .staging import (_NUMA, _POOLS, _STAGING, _STAGING_BUILD, _STAGING_LOCK, _STAGING_THREADS, _copy_pool, _on_cpus, _staging, _staging_key,
                      gpu_numa_cpus, pinned_near)
from .toplists import (DEEP_MAX_K, DEEP_WS_BYTES, DISTINCT_DEEP_WS_BYTES, DISTINCT_KERNEL_MAX, MAX_K, MERGE_KERNEL_MAX, PAD_SCORE,
                       _check_max_depth, _distinct_row_depth, distinct_topk, distinct_topk_device, merge_topk, merge_topk_device, merge_topk_sorted, split_under)


def _torch():
    import torch
    return torch


STATUS_OK, STATUS_OVERFLOW, STATUS_TOO_FEW, STATUS_UNCERTAIN, STATUS_RANGE = 0, 1, 2, 3, 4
_SPLIT = ("bf16x3", "fp16x3", "fp16x2")          # precisions that pin the second rung

_Depth = collections.namedtuple("_Depth", "enqueue max_cap shortcut last_rung last_stat deep_stats")
# what search_begin hands to search_finish: depth None = k > DEEP_MAX_K (nothing enqueued), first = (D, I, status, tau_retry) of
# the enqueued first pass or None (nothing to scan: deep search of an empty index, or a filter that allows no row),
# allowed = the RowFilter of a restricted search or None
_Pending = collections.namedtuple("_Pending", "qt k depth x3 cap first allowed", defaults=(None,))
# the handle of a search with per-query exclusions: the _Pending of the search at the depth k' = k + e_max, the QueryExclusions
# and the caller's k
_PendingExcluded = collections.namedtuple("_PendingExcluded", "pending exclusions k")


def _radius_below(x):
    """the largest fp32 strictly below the fp64 score x: every row that ties with x, or beats it, exceeds this radius"""
    r = np.float32(x)
    return r if np.float64(r) < x else np.nextafter(r, np.float32(-np.inf))


class FlatIPIndex(_IndexStore):
    """Exact inner-product index resident in HBM.  ``add`` keeps the fp32 block and builds its 16-bit scan copy;
    ``search`` returns FAISS-shaped ``(D float32 [nq,k], I int64 [nq,k])`` and is certified exact
    (see include/convdr_hip.h).

    precision: "auto" (default) scans in fp16 (v_mfma_f32_32x32x16_f16: the bf16 rate, 8x tighter error band) and
    re-runs the queries that cannot be certified with the split-fp16 scan (three MFMA passes, another 4x); "fp16" /
    "fp16x3" / "bf16" / "bf16x3" pin one rung (the bf16 pair is the round-1/2 ladder: same engine, u = 2^-8).  Whatever
    the rung, a query it cannot certify ends on the exhaustive rung, so the result never depends on the choice.
    center: subtract the column mean of the first added block from every passage before rounding (ranking-neutral,
    shrinks the error band by |p| / |p - mean|; essential for real encoder outputs, which share a large common
    component).
    reserve(n): allocate the resident block for n passages up front; add() then fills it in place.  Without it every
    add() after the first re-allocates (FAISS semantics need one contiguous block): fine for the reference's one add per
    reset, not for building a 117 GB corpus from slices.
    storage: "fp32" (default) is the index described above.  "fp16" is the HALF STORE: the passage is kept once, in 16 bits,
    and that copy is both the corpus and the scan operand (include/convdr_hip.h, "Half-precision passage store") -- a third
    of the bytes, no fp32 block, no remainder copy, no centre.  The corpus is then DEFINED as the stored halves (float16
    rows are kept bit for bit, fp32 rows are rounded to nearest even once, at add) and ``search`` returns the exact,
    certified top-k of those halves widened to fp32.  Its precisions are "auto" (single pass, then the two-pass rung
    P Qh + P Ql, then the exhaustive rung; `stats["x2_queries"]`), "fp16" and "fp16x2"; add() refuses (ConvdrError, index
    unchanged) rows with a value that is not finite as a half or with a norm above 60,000.
    "sq8" is the 8-BIT STORE: the passage is kept once, as d int8 codes of a scalar quantiser (centre = the first add's column
    mean, step = its largest column deviation / 127, both fixed then; later rows outside saturate, `stats["sq8_saturated"]`), and
    the codes are both the corpus and the operand of an exact integer scan (include/convdr_hip.h, "8-bit store").  The corpus is
    DEFINED as the reconstructed rows fl32(centre + fl32(step * code)) -- what ``reconstruct_n`` returns -- and ``search`` is the
    exact, certified top-k of those.  d is padded to a multiple of 128 and at most 1,024; precisions "auto" / "i8"; always
    centred; add() refuses a value that is not finite; `index_store.SQ8_REFUSED` lists the entries it does not offer."""

    def _ids_arg(self, who, q, ids):
        """(queries as a tensor, ids as a tensor, the shape of `ids`) of a (queries, document ids) call; the checks that need
        no device"""
        import torch
        if isinstance(ids, np.ndarray) and not ids.flags.writeable:
            ids = np.array(ids)
        qt, it, nq, fits = self._pairs_arg(who, q, ids)
        if it.dtype != torch.int64 or not fits:
            raise ValueError("%s: ids must be int64 [nq] or [nq, m] with nq = %d (got %s, shape %s)"
                             % (who, nq, it.dtype, tuple(it.shape)))
        return qt, it, tuple(it.shape)

    def _pairs_arg(self, who, q, items):
        """(queries as a tensor, items as a tensor, nq, whether the items are [nq] or [nq, m]); queries not [nq, d]: ValueError"""
        import torch
        qt, it = torch.as_tensor(q), torch.as_tensor(items)
        if qt.dim() != 2 or qt.shape[1] not in (self.d, self.d_in):
            raise ValueError("%s: queries must be [nq, %d] (got shape %s)" % (who, self.d_in, tuple(qt.shape)))
        nq = int(qt.shape[0])
        return qt, it, nq, it.dim() in (1, 2) and int(it.shape[0]) == nq

    def score_ids(self, q, ids):
        """``score_ids_tensors`` as numpy: (D float32, R int64), the shape of `ids`."""
        D, R = self.score_ids_tensors(q, ids)
        return D.cpu().numpy(), R.cpu().numpy()

    def score_ids_tensors(self, q, ids):
        """MaxP score of given documents: ids int64 [nq] (one document per query) or [nq, m], numpy or torch, host or device.
        Returns device (D float32, R int64) of the shape of `ids`: D = the largest canonical score among the rows that carry
        the id -- the fp32 rounding of the fp64 score ``search`` ranks by, what ``score_rows`` gives for that row -- and R the
        row that attains it, the lowest on equal scores.  An id on no row gives the padding pair (-3.4028235e38, -1): that
        includes INT64_MIN, the natural padding of a device list, and the -1 ``search_ids`` pads with whenever no document has
        the id -1.  Re-ranking a list of documents (BM25 candidates, a known positive) needs no id -> row map on the host:
        one key set and one CSR over the flattened list, one score launch, one host read (the CSR's size)."""
        import torch
        self._store.refuse(self, "score_ids")
        self._need_ids("score_ids")
        qt, it, shape = self._ids_arg("score_ids", q, ids)
        nq, m = int(qt.shape[0]), (shape[1] if len(shape) == 2 else 1)
        qt = self._queries(qt, padded_ok=True)
        D = torch.empty((nq, m), dtype=torch.float32, device=self.device)
        R = torch.empty((nq, m), dtype=torch.int64, device=self.device)
        if nq and m:
            n = self.ntotal
            start, count, rows, _ = self._rows_csr("score_ids", it.to(self.device).reshape(-1).contiguous(), reserved_ok=True)
            store, r32, r16, scale, _ = self._operands(None if n else (None, None))     # (an empty index passes no rows)
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().convdr_ip_score_docs(store, _lib.ptr(qt), nq, r32, r16, scale, n, self.d, _lib.ptr(rows),
                                                           int(rows.numel()), _lib.ptr(start), _lib.ptr(count), m, m, None,
                                                           _lib.ptr(D), _lib.ptr(R), _lib.stream_ptr()), "convdr_ip_score_docs")
        return D.reshape(shape), R.reshape(shape)

    def _ordinals(self, ordinals):
        """ordinals= of a rank_ids call -> None or a DocOrdinals that fits this index"""
        if ordinals is None:
            return None
        if not isinstance(ordinals, DocOrdinals):
            raise ValueError("ordinals must be a DocOrdinals of this index (FlatIPIndex.doc_ordinals)")
        if ordinals.n != self.ntotal or ordinals.ord.device != self.device:
            raise ValueError("stale DocOrdinals: built for ntotal = %d on %s, the index holds %d rows on %s"
                             % (ordinals.n, ordinals.ord.device, self.ntotal, self.device))
        return ordinals

    def search_docs(self, q, k, allowed=None, depth=None, strict=True, max_depth=None):
        """Exact top-k DOCUMENTS: ``search_distinct`` with the index's own id column for keys -- no side table to keep in
        step.  Returns device (D fp32 [nq, k], ids int64 [nq, k], rows int64 [nq, k] = each document's best row, counts int32
        [nq, 2]); padding (-3.4028235e38, -1, -1).  ``score_ids_tensors(q, ids)`` reproduces D and rows.  allowed: as for
        ``search``; a filter may drop some chunk rows of a document (its best ALLOWED row then stands for it) or all of them.
        ``excluding(ex).search_docs`` applies per-query exclusions to the row lists before the distinct cut."""
        return self._search_docs(q, k, allowed, depth, strict, max_depth, None)

    def _search_docs(self, q, k, allowed, depth, strict, max_depth, exclude):
        self._store.refuse(self, "search_docs")
        self._need_ids("search_docs")
        D, I, K, counts = self._search_distinct_rows(q, k, self.ids, depth, strict, max_depth, allowed, exclude)
        return D, K, I, counts

    def search_ids(self, q, k, allowed=None):
        """``search`` with ids for row numbers: numpy (D, ids [nq, k]); FAISS padding stays -1."""
        D, I = self.search_ids_tensors(q, k, allowed=allowed)
        return D.cpu().numpy(), I.cpu().numpy()

    def search_ids_tensors(self, q, k, allowed=None):
        """``search_tensors`` with I mapped through the id column on the device (-1 stays -1)."""
        self._need_ids("search_ids")
        return self._ids_of(*self.search_tensors(q, k, allowed=allowed))

    def _ids_of(self, D, I):
        """(D, I) of a row search -> (D, the rows' ids), -1 kept"""
        import torch
        if not self.ntotal:
            return D, I
        return D, torch.where(I >= 0, self.ids[I.clamp(min=0)], torch.full_like(I, -1))

    def _search_call(self, q, nq, p32, p16, plo, n, k, tau_in, cap, rank_target, ws, D, I, status, tau_retry, split=False,
                     deep=False, allowed=None):
        """One call of convdr_ip_search[_deep][_f16 | _h16 | _q8]: the entry of this index's scan copy and of the depth, each with
        the operands it declares (the store description's `call`); with a RowFilter, convdr_ip_search_filtered[_q8] with the same
        operands."""
        ptr = _lib.ptr
        what = "search" if allowed is None else "filtered"
        suffix, head, rows = self._store.call(what, self._operands((p32, p16)), plo, split)
        tail = (n, self.d, k, ptr(self._max_norm), ptr(tau_in), cap, rank_target, ptr(ws), ws.numel())
        out = (ptr(D), ptr(I), ptr(status), ptr(tau_retry), _lib.stream_ptr())
        if allowed is not None:
            name = "convdr_ip_search_filtered" + suffix
            _lib.check(getattr(_lib.lib(), name)(*head, int(bool(deep)), ptr(q), nq, *rows, *tail, ptr(allowed.bits), allowed.bits.numel(),
                                                 allowed.n_allowed, *out), name)
        else:
            name = "convdr_ip_search" + ("_deep" if deep else "") + suffix
            _lib.check(getattr(_lib.lib(), name)(ptr(q), nq, *rows, *tail, *out), name)

    def _enqueue(self, q, k, tau_in, cap, x3, deep=False, rows=None, rank_target=None, allowed=None):
        """One enqueue of the kernel pipeline, shallow or deep, over the resident block or over `rows` = (re-score rows, scan
        copy) of an exhaustive slice: allocates (D, I, status, tau_retry), sizes the workspace and calls the entry.  No sync.
        Memory bound of the deep pipeline: its workspace is ~ nq * cap * 28 bytes (list id + scan score, band id + fp64 score,
        ordered fp64 score) plus the threshold sample's scores (sampled rows x padded queries x 4); 1,000 queries at
        cap = 131,072 would be 3.7 GB beside the resident corpus.  The queries are therefore split so that ONE call never asks
        for more than DEEP_WS_BYTES = 4 GiB of workspace (the calls run back to back on the stream and share the buffer)."""
        import torch
        L = _lib.lib()
        if x3:
            self._ensure_lo()
        p32, p16 = (self._rows, self._pbf) if rows is None else rows
        nq, n = int(q.shape[0]), self.ntotal if rows is None else int(p16.shape[0])
        if n == 0:
            p32 = p16 = q               # never dereferenced when n == 0
        plo = self._plo if (x3 and n) else None
        D = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        I = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        status = torch.empty(nq, dtype=torch.int32, device=self.device)
        tau_retry = torch.empty(nq, dtype=torch.float32, device=self.device)
        ws_bytes = L.convdr_ip_deep_workspace_bytes if deep else L.convdr_ip_workspace_bytes
        step, need = split_under(lambda c: ws_bytes(c, n, self.d, k, cap), nq, self.DEEP_WS_BYTES if deep else None)
        if deep and not need:
            raise _lib.ConvdrError("convdr_ip_search_deep: sizes outside the contract (nq=%d n=%d d=%d k=%d cap=%d)"
                                   % (nq, n, self.d, k, cap))
        ws = self._workspace(need)
        rank_target = self.rank_target if rank_target is None else rank_target
        with torch.cuda.device(self.device):
            if step >= nq:
                self._search_call(q, nq, p32, p16, plo, n, k, tau_in, cap, rank_target, ws, D, I, status, tau_retry, x3, deep,
                                  allowed)
            else:
                for a in range(0, nq, step):
                    b = min(nq, a + step)
                    self._search_call(q[a:b], b - a, p32, p16, plo, n, k, None if tau_in is None else tau_in[a:b], cap, rank_target,
                                      ws, D[a:b], I[a:b], status[a:b], tau_retry[a:b], x3, deep, allowed)
        return D, I, status, tau_retry

    def search_device(self, q, k, tau_in=None, cap=None, x3=None, allowed=None):
        """One enqueue of the kernel pipeline; q is a device fp32 [nq, d] tensor.  allowed: a RowFilter (or a mask, packed for
        this call): only its rows can be returned, and the certificate holds over them.
        Returns device tensors (D, I, status, tau_retry); no sync.
        status (per query): 0 = certified exact; 1 / 2 / 3 = not certified, re-run with tau_retry (search_tensors walks that
        ladder); 4 = CONVDR_IP_RANGE, fp16 rungs only: the scan copy was built with a scale that later, longer rows (or an
        astronomically long query) overflow -- D / I of such a query are NOT usable, and no retry with another threshold
        helps: call ``_rebuild_scaled()`` (search_tensors / search_finish do) and search again.  Callers that take one
        uncertified pass (search_sharded_device(certify=False), the C ABI) must treat any non-zero status as "no result"."""
        cap = cap or self.cap
        while cap < 2 * k and cap < 8192:      # the candidate list holds at least 2k entries (csrc/ip_host.hpp, ip_check_sizes: k <= cap / 2)
            cap *= 2
        return self._enqueue(q, k, tau_in, cap, self.precision in _SPLIT if x3 is None else x3, allowed=self._filter(allowed))

    def last_counts(self, nq, k, cap=None):
        """(emitted, band) int32 tensors [nq] of the last search_device call (instrumentation)."""
        L = _lib.lib()
        cap = cap or self.cap
        out = []
        for fn in (L.convdr_ip_debug_counts, L.convdr_ip_debug_band):
            off = fn(_lib.ptr(self._ws), nq, self.ntotal, self.d, k, cap) - self._ws.data_ptr()
            out.append(self._ws[off:off + 4 * nq].view(_torch().int32))
        return tuple(out)

    def _certify(self, depth, qt, k, D, I, status, tau_retry, x3, cap, kw=None):
        """Host loop around the kernel's certificate: re-run the queries that are not OK with the threshold the kernel
        proposes, the candidate capacity doubled on OVERFLOW up to the depth's limit.  Returns the indices still uncertified.
        kw: None or {"allowed": RowFilter}, handed to every enqueue."""
        import torch
        kw = kw or {}
        st = status.cpu().numpy()
        bad = np.nonzero(st != 0)[0]
        rounds = 0
        while len(bad) and rounds < 6:
            rounds += 1
            self.stats["rounds"] += 1
            idx = torch.as_tensor(bad, device=self.device)
            tau = tau_retry[idx].contiguous()
            if (st[bad] == STATUS_OVERFLOW).any():
                if cap >= depth.max_cap:
                    break
                cap *= 2
                if depth.deep_stats:
                    self.stats["deep_cap"] = max(self.stats["deep_cap"], cap)
            Db, Ib, sb, tb = getattr(self, depth.enqueue)(qt[idx].contiguous(), k, tau_in=tau, cap=cap, x3=x3, **kw)
            D[idx], I[idx], tau_retry[idx] = Db, Ib, tb
            sb = sb.cpu().numpy()
            st[bad] = sb
            bad = bad[sb != 0]
        return bad

    def search(self, q, k, allowed=None):
        """FAISS ``index.search``: numpy in, numpy (D, I) out; always the exact top-k (queries no scan can certify take the
        exhaustive rung, `stats["exhaustive_queries"]`).  allowed: a RowFilter (``row_filter``) or a bool / uint8 mask
        [ntotal], packed for this call -- the search is restricted to those rows (FAISS ``IDSelector``): the exact top-k of the
        allowed rows, I in the index's row numbers, padding where fewer than k rows are allowed.  Rows left out PER QUERY:
        ``excluding(ex).search`` (ExcludedSearch)."""
        D, I = self.search_tensors(q, k, allowed=allowed)
        return D.cpu().numpy(), I.cpu().numpy()

    def search_tensors(self, q, k, allowed=None):
        """``search`` with the certified result left on the device (torch fp32 [nq, k], int64 [nq, k]).

        precision="auto": the fp16 scan first; queries it cannot certify are re-run -- with a lower threshold while their
        error band still fits the candidate list, with the split scan (4x tighter band) once the band has swallowed
        the whole list.  The index remembers when most queries of a block ended on the split scan and starts there next
        time (`x3_first`)."""
        return self.search_finish(self.search_begin(q, k, allowed=allowed))

    def search_begin(self, q, k, allowed=None):
        """First half of search_tensors: the first scan pass is ENQUEUED (no host round trip) and a handle returned;
        search_finish(handle) reads the certificates and walks the ladder for whatever the first pass left open.  Between the
        two the host is free -- search_one_by_one loads the next block file meanwhile."""
        qt = self._queries(q)
        k = int(k)
        f = self._filter(allowed)
        kw = {} if f is None else {"allowed": f}
        if k > self.DEEP_MAX_K:
            # the reference takes any --top_n (run_convdr_inference.py:316-319); the deep kernel pipeline's candidate lists end
            # at 131,072 entries, so larger k takes the chunked host-side route (exact, slow): see _search_large_k
            return _Pending(qt, k, None, None, None, None, f)
        x3 = self.precision in _SPLIT or (self.precision == "auto" and self._x3_first and self.ntotal > 0)
        # 4096 < k <= 65536: the same pipeline with the lists in global memory (convdr_ip_search_deep*)
        depth, cap = (self._DEEP, self._deep_cap(k)) if k > self.MAX_K else (self._SHALLOW, self.cap)
        if (depth is self._DEEP and not self.ntotal) or (f is not None and f.n_allowed == 0):
            return _Pending(qt, k, depth, x3, cap, None, f)     # (the shallow kernels pad an empty index's result themselves)
        return _Pending(qt, k, depth, x3, cap, getattr(self, depth.enqueue)(qt, k, cap=cap, x3=x3, **kw), f)

    def search_finish(self, handle):
        """The ladder, at either depth: fp16 (or pinned) first pass -> rebuild on RANGE -> retries with tau_retry / a doubled
        list -> split scan -> whatever is still open takes the depth's last rung."""
        import torch
        if isinstance(handle, _PendingExcluded):
            return self._finish_excluded(handle)
        qt, k, depth, x3, cap, first, allowed = handle
        kw = {} if allowed is None else {"allowed": allowed}    # (allowed=None: today's calls, argument for argument)
        nq = int(qt.shape[0])
        split_key = self._split_key
        self.stats = {"retried": 0, "rounds": 1, "x3_queries": 0, "x3_first": bool(x3), "rescaled": 0}
        self.stats[split_key] = nq if x3 else 0
        if depth is None:
            self.stats.update(rounds=0, large_k=k, deep=0, deep_cap=0, chunked_queries=nq)
            return self._search_large_k(qt, k, **kw)
        if depth.deep_stats:
            self.stats.update(large_k=k, deep=nq, deep_cap=cap, chunked_queries=0)
        if first is None:               # empty index, or no row allowed: FAISS padding
            return (torch.full((nq, k), PAD_SCORE, dtype=torch.float32, device=self.device),
                    torch.full((nq, k), -1, dtype=torch.int64, device=self.device))
        enqueue = functools.partial(getattr(self, depth.enqueue), **kw)
        D, I, status, tau_retry = first
        n_range, n_bad = torch.stack([(status == STATUS_RANGE).sum(), (status != 0).sum()]).tolist()   # one host round trip
        if n_range and self._store.final_range(self):
            raise _lib.ConvdrError("convdr_ip_search: " + self._store.final_range(self))     # no threshold and no retry changes this verdict
        if n_range:
            self._rebuild_scaled()
            self.stats["rescaled"] = 1
            D, I, status, tau_retry = enqueue(qt, k, cap=cap, x3=x3)
            n_bad = int((status != 0).sum().item())
        self.stats["retried"] = int(n_bad)
        self.stats.update(self._store.search_stats(self, nq, n_bad))
        second = self.precision == "auto" and not x3 and self._store.second_rung      # the split scan is still ahead
        bad = []
        if n_bad and second and depth.shortcut:
            # a band that already covers every emitted candidate only grows with a lower threshold: those queries go
            # straight to the split scan, the others get their single-pass retries
            emitted, band = self.last_counts(nq, k)
            st = status.cpu().numpy()
            sat = ((band >= emitted) & (emitted > 0)).cpu().numpy() & (st == STATUS_UNCERTAIN)
            retry_idx = np.nonzero((st != 0) & ~sat)[0]
            bad = list(np.nonzero(sat)[0])
            if len(retry_idx):
                sub = torch.as_tensor(retry_idx, device=self.device)
                Db, Ib, sb, tb = D[sub], I[sub], status[sub], tau_retry[sub]
                left = self._certify(depth, qt[sub].contiguous(), k, Db, Ib, sb, tb, False, cap, kw)
                D[sub], I[sub] = Db, Ib
                bad += list(retry_idx[np.asarray(left, dtype=np.int64)]) if len(left) else []
            bad = np.asarray(sorted(bad), dtype=np.int64)
        elif n_bad:
            bad = self._certify(depth, qt, k, D, I, status, tau_retry, x3, cap, kw)
        if len(bad) and second:
            # second rung: split scan for the queries the single-pass error band cannot separate
            idx = torch.as_tensor(bad, device=self.device)
            qs = qt[idx].contiguous()
            self.stats[split_key] = len(bad)
            Db, Ib, sb, tb = enqueue(qs, k, cap=cap, x3=True)
            self.stats["rounds"] += 1
            bad2 = self._certify(depth, qs, k, Db, Ib, sb, tb, True, cap, kw) if int((sb != 0).sum().item()) else []
            D[idx], I[idx] = Db, Ib
            bad = bad[np.asarray(bad2, dtype=np.int64)] if len(bad2) else []
        if self.precision == "auto":
            self._x3_first = self.stats[split_key] > nq // 2
        if len(bad):
            # last rung: more than the largest list's worth of passages inside the error band of the k-th score even with the
            # split scan (blocks whose norms spread over orders of magnitude: eps scales with the LARGEST norm).  Shallow:
            # every slice of <= cap rows is searched with all of its rows as candidates -- exact by construction -- and the
            # slices are merged in row order (earlier rows win ties): slow (one small launch chain per slice) but always an
            # answer.  Deep: the chunked route of k > DEEP_MAX_K
            idx = torch.as_tensor(np.asarray(bad, dtype=np.int64), device=self.device)
            Db, Ib = getattr(self, depth.last_rung)(qt[idx].contiguous(), k, **kw)
            D[idx], I[idx] = Db, Ib
            self.stats[depth.last_stat] = len(bad)
            if depth.deep_stats:
                self.stats["deep"] = nq - len(bad)
        return D, I

    def excluding(self, exclude):
        """The exact entries of this index with rows left out PER QUERY: an ExcludedSearch.  exclude: a QueryExclusions
        (``exclude_rows`` / ``exclude_ids``, reusable across calls), or a raw int64 [nq, e] array or list of nq lists, built
        for each call.  ``idx.excluding(ex).search(Q, k, allowed=f)`` is the exact top-k of the (allowed) rows that query j does
        not exclude; likewise search_tensors, search_begin, search_ids(_tensors), search_docs, range_search(_tensors),
        range_count and rank_rows(_tensors)."""
        self._store.refuse(self, "excluding")
        return ExcludedSearch(self, exclude)

    def _search_begin_excluded(self, q, k, allowed, exclude):
        """search_begin with per-query exclusions: the first pass is enqueued at the depth k' = k + e_max, the handle carries
        the exclusions and the caller's k, search_finish drops and cuts."""
        qt = self._queries(q)
        k = int(k)
        f = self._filter(allowed)
        ex = self._exclusions(exclude, int(qt.shape[0]))
        if k < 1:
            raise ValueError("search: k = %d with exclusions" % k)
        # all of the residual top-k lies in the first k + e_q entries of the (allowed) order; never deeper than the rows the
        # search can return ("Per-query exclusions")
        rows = self.ntotal if f is None else f.n_allowed
        deep = min(k + ex.e_max, max(k, rows))
        return _PendingExcluded(self.search_begin(q, deep, **({} if f is None else {"allowed": f})), ex, k)

    def _finish_excluded(self, handle):
        """search_finish of a handle with exclusions: the certified lists at the depth k' the handle was begun with, then
        convdr_excl_drop_topk -- per query the first k entries whose row it does not exclude.  A call whose lists are all
        empty returns the search's own tensors."""
        import torch
        pending, ex, k = handle
        deep = pending.k
        D, I = self.search_finish(pending)
        self.stats.update(exclude_depth=deep, excluded_dropped=0)
        nq = int(D.shape[0])
        if ex.e_max == 0 or nq == 0:
            return D, I
        D, I = D.contiguous(), I.contiguous()
        Do = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        Io = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        kept = torch.empty(nq, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().convdr_excl_drop_topk(_lib.ptr(D), _lib.ptr(I), nq, deep, deep, _lib.ptr(ex.rows), int(ex.rows.shape[1]),
                                                        _lib.ptr(ex.count), k, _lib.ptr(Do), _lib.ptr(Io), _lib.ptr(kept),
                                                        _lib.stream_ptr()), "convdr_excl_drop_topk")
        self.stats["excluded_dropped"] = int(((I >= 0).sum() - kept.sum()).item())
        return Do, Io

    def search_distinct(self, q, k, keys, depth=None, strict=True, max_depth=None):
        """Exact top-k DISTINCT keys (documents) of a block whose rows carry keys with repeats (MaxP chunk rows, duplicate
        pids): per query the k best keys, each with its best row, in the canonical order of ``search``.
        keys: device int64 [ntotal], the key of every row (``embid``, or ``offset2pid[embid]``).
        The certified row search runs at depth m (``depth``, default min(MAX_K, 2k, ntotal)) and convdr_topk_distinct keeps the
        first row per key.  A query is CERTIFIED -- its result is what the walk over ALL rows gives -- iff it found k keys, or
        the list ran out of rows (n_valid < m), or m is the whole block: the first k distinct keys of the full order lie
        inside any prefix that already holds k of them.  Only the uncertified queries are searched
        again, at min(2m, MAX_K, ntotal).  A query still uncertified at the limit raises ConvdrError (strict) or keeps its
        short, padded row (its counts tell).
        max_depth (default MAX_K, at most DEEP_MAX_K) takes MAX_K's place in all of the above -- the bound of k, of ``depth``
        and of the doubling: beyond 4,096 rows the row search is the deep one and the cut convdr_topk_distinct_deep.
        Returns device tensors (D fp32 [nq, k], I int64 [nq, k] rows, K int64 [nq, k] keys, counts int32 [nq, 2] =
        (n_distinct, n_valid) of the pass that produced the row); slots past a query's last key hold (-3.4028235e38, -1, -1)."""
        return self._search_distinct(q, k, keys, depth, strict, max_depth, None)

    def _search_distinct(self, q, k, keys, depth, strict, max_depth, allowed):
        """``_search_distinct_rows`` without exclusions"""
        return self._search_distinct_rows(q, k, keys, depth, strict, max_depth, allowed, None)

    def _search_distinct_rows(self, q, k, keys, depth, strict, max_depth, allowed, exclude):
        """``search_distinct`` with a row filter (``search_docs``).  allowed: a RowFilter or a mask as for ``search``, packed
        once for all passes, or None.  With a filter the result is the walk over the ALLOWED rows, the filter's ``n_allowed``
        takes ntotal's place in the depth defaults, and a query is certified iff it found k keys, or the list ran out of rows,
        or m >= n_allowed.  None: search_distinct as it was.
        exclude (``excluding(ex).search_docs``): per-query exclusions handed to the row search, sub-selected to the open queries.  The list
        that comes back is a complete prefix of the residual order, so the certificate is the same one."""
        import torch
        self._store.refuse(self, "search_distinct")
        qt = torch.as_tensor(q)
        k, nq, nt = int(k), int(qt.shape[0]), self.ntotal
        max_depth = _check_max_depth("search_distinct", max_depth)
        if k < 1 or k > max_depth:
            raise ValueError("search_distinct: k = %d is outside 1..%d" % (k, max_depth))
        if keys.dtype != torch.int64 or keys.dim() != 1 or keys.device != self.device:
            raise ValueError("search_distinct: keys must be an int64 vector on %s" % (self.device,))
        keys = keys.contiguous()
        f = self._filter(allowed)
        kw = {} if f is None else {"allowed": f}
        ex = self._exclusions(exclude, nq)
        rows = nt if f is None else f.n_allowed          # the rows the search can return
        limit = min(max_depth, rows)
        m = int(depth) if depth else min(max_depth, 2 * k, rows)
        m = max(1, min(m, max_depth))
        D = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        I = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        K = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        counts = torch.zeros((nq, 2), dtype=torch.int32, device=self.device)
        if nq == 0:
            return D, I, K, counts
        qt = (qt if qt.dtype == torch.float32 else qt.float()).to(self.device)
        todo = todo_host = None                         # indices of the queries still open (None: all)
        self.distinct_stats = {"depths": [], "searched": []}
        while True:
            qs = qt if todo is None else qt[todo].contiguous()
            who = self if ex is None else self.excluding(ex if todo is None else ex.select(todo_host))
            Dm, Im = who.search_tensors(qs, m, **kw)
            Dd, Id, Kd, cd = distinct_topk_device(Dm, Im, k, keys)
            self.distinct_stats["depths"].append(m)
            self.distinct_stats["searched"].append(int(qs.shape[0]))
            if todo is None:
                D, I, K, counts = Dd, Id, Kd, cd
            else:
                D[todo], I[todo], K[todo], counts[todo] = Dd, Id, Kd, cd
            c = cd.cpu().numpy()                        # the one host round trip of a pass: the certificate
            if (c[:, 0] < 0).any():
                raise _lib.ConvdrError("search_distinct: keys has %d entries, the block %d rows" % (keys.numel(), nt))
            open_ = np.nonzero(~((c[:, 0] >= k) | (c[:, 1] < m) | (m >= rows)))[0]
            if not len(open_):
                return D, I, K, counts
            if m >= limit:
                if strict:
                    raise _lib.ConvdrError("search_distinct: %d queries hold fewer than %d distinct keys in their top %d rows, the "
                                           "deepest row search (%s = %d)"
                                           % (len(open_), k, m, "FlatIPIndex.MAX_K" if max_depth == self.MAX_K else "max_depth",
                                              max_depth))
                return D, I, K, counts
            sub = torch.as_tensor(open_, device=self.device)
            todo = sub if todo is None else todo[sub]
            todo_host = open_ if todo_host is None else todo_host[open_]
            m = min(2 * m, limit)

    @property
    def _split_key(self):
        """stats key that counts the queries of the second rung: the three-pass split scan, or the half store's two passes"""
        return self._store.split_key

    MAX_K, DEEP_MAX_K = MAX_K, DEEP_MAX_K        # convdr_ip_search / _deep: k <= cap / 2, cap <= 8192 / 131072
    DEEP_MIN_CAP, DEEP_MAX_CAP = 16384, 131072
    DEEP_WS_BYTES = DEEP_WS_BYTES        # most workspace one deep call may ask for; search_deep_device splits the queries to stay under it
    # the two depths of the ladder (search_begin / search_finish): the method that enqueues a pass, where the doubling of the
    # candidate capacity ends, whether last_counts serves the saturated-band shortcut, the last rung and the stat it reports, whether stats carries
    # the deep keys (large_k, deep, deep_cap, chunked_queries)
    _SHALLOW = _Depth("search_device", 8192, True, "_search_exhaustive", "exhaustive_queries", False)
    _DEEP = _Depth("search_deep_device", DEEP_MAX_CAP, False, "_search_large_k", "chunked_queries", True)

    def _deep_cap(self, k):
        """Candidate capacity of the first deep pass: the largest power of two <= 4k inside the kernel's range -- between 2k
        (the kernel's k <= cap / 2) and 4k entries per query."""
        cap = self.DEEP_MIN_CAP
        while 2 * cap <= 4 * k and cap < self.DEEP_MAX_CAP:
            cap *= 2
        return cap

    def search_deep_device(self, q, k, tau_in=None, cap=None, x3=False, allowed=None):
        """``search_device`` for MAX_K < k <= DEEP_MAX_K: enqueues convdr_ip_search_deep[_f16 | _h16]; device (D, I, status,
        tau_retry) with the meanings of search_device; no sync.  The queries are split under DEEP_WS_BYTES (see _enqueue)."""
        cap = int(cap or self._deep_cap(k))
        allowed = self._filter(allowed)
        if self.ntotal <= cap or (allowed is not None and allowed.n_allowed <= cap):
            tau_in = None               # every row is a candidate: the list is complete whatever threshold a retry proposes
        return self._enqueue(q, k, tau_in, cap, x3, deep=True, allowed=allowed)

    def _exact_slice(self, rows, kq, qq, cap):
        """Top-kq of the slice `rows` = (re-score rows, scan copy) of at most `cap` rows: the plan takes every row as a candidate
        (no threshold pass, tau = -inf), so the result is exact by construction."""
        D, I, status, _ = self._enqueue(qq, kq, None, cap, False, rows=rows, rank_target=0)
        if int((status != 0).sum().item()):
            if self._store.final_range(self) and int((status == STATUS_RANGE).sum().item()):
                raise _lib.ConvdrError("convdr_ip_search: " + self._store.final_range(self))
            raise _lib.ConvdrError("convdr_ip_search: exhaustive slice of %d rows not certified" % rows[1].shape[0])
        return D, I

    def _row_chunks(self, step, allowed):
        """The rows the last rungs rank, in ascending chunks of at most `step`: ((re-score rows, scan copy), back) per chunk,
        where back maps a chunk-local index tensor I >= 0 to row numbers.  Without a filter the chunks are slices of the
        resident block; with one they are gathered from the ascending list of allowed row ids -- ascending chunks keep the rule
        that the earlier row wins a tie, and no filtered kernel is needed."""
        if allowed is None:
            for s0 in range(0, self.ntotal, step):
                e0 = min(self.ntotal, s0 + step)
                yield (self._rows[s0:e0], self._pbf[s0:e0]), (lambda I, s0=s0: I + s0)
        else:
            ids = allowed.rows()
            for s0 in range(0, int(ids.numel()), step):
                chunk = ids[s0:s0 + step]
                yield self._row_pair(chunk), (lambda I, chunk=chunk: chunk[I])

    def _search_large_k(self, q, k, q_chunk=8, allowed=None):
        """Exact top-k for k > MAX_K (any --top_n, run_convdr_inference.py:316-319) by chunking on the host side of the
        same kernels: every slice of <= 4096 rows is RANKED COMPLETELY by the exhaustive plan (all rows candidates, canonical
        fp64 scores, kq = rows), the slices' sorted lists are merged by a stable descending sort of the fp32-rounded scores
        (rounding is monotone: only rows whose scores round to the SAME fp32 value can be out of canonical order, and only
        across slices), and every run of equal fp32 scores that spans slices or straddles rank k is ranked once more as one
        slice.  Slow (n / 4096 launch chains per 8 queries, an [8, n] sort), always the exhaustive exact answer."""
        import torch
        nq, n = int(q.shape[0]), self.ntotal if allowed is None else allowed.n_allowed      # n: the rows that can be returned
        Dout = torch.full((nq, k), PAD_SCORE, dtype=torch.float32, device=self.device)
        Iout = torch.full((nq, k), -1, dtype=torch.int64, device=self.device)
        if n == 0:
            return Dout, Iout
        cap, step = 8192, 4096

        with torch.cuda.device(self.device):
            for j0 in range(0, nq, q_chunk):
                qq = q[j0:j0 + q_chunk].contiguous()
                Ds, Is = [], []
                for pair, back in self._row_chunks(step, allowed):
                    D, I = self._exact_slice(pair, int(pair[1].shape[0]), qq, cap)
                    Ds.append(D)
                    Is.append(back(I))
                Dall, Iall = torch.cat(Ds, 1), torch.cat(Is, 1)
                order = torch.sort(Dall, dim=1, descending=True, stable=True).indices
                Dall, Iall = torch.gather(Dall, 1, order), torch.gather(Iall, 1, order)
                kk = min(k, n)
                for j in range(qq.shape[0]):
                    d, i = Dall[j], Iall[j]
                    # end of the run of equal fp32 scores that contains rank kk - 1
                    end = kk + int((d[kk:] == d[kk - 1]).sum().item()) if kk < n else kk
                    d, i = d[:end].clone(), i[:end].clone()
                    # runs of equal scores (start, length) with more than one member
                    new = torch.ones(end, dtype=torch.bool, device=self.device)
                    new[1:] = d[1:] != d[:-1]
                    starts = torch.nonzero(new).flatten()
                    lens = torch.diff(torch.cat([starts, torch.tensor([end], device=self.device)]))
                    for b, ln in zip(starts[lens > 1].tolist(), lens[lens > 1].tolist()):
                        if ln > step:
                            raise _lib.ConvdrError("FlatIPIndex.search: %d passages share one fp32 score around rank %d; "
                                                   "k > %d cannot order a tie group that large" % (ln, b, self.MAX_K))
                        rows = torch.sort(i[b:b + ln]).values
                        Dj, Ij = self._exact_slice(self._row_pair(rows), ln, qq[j:j + 1].contiguous(), cap)
                        d[b:b + ln], i[b:b + ln] = Dj[0], rows[Ij[0]]
                    Dout[j0 + j, :kk], Iout[j0 + j, :kk] = d[:kk], i[:kk]
        return Dout, Iout

    def _search_exhaustive(self, q, k, allowed=None):
        import torch
        nq = int(q.shape[0])
        kk = min(2 * k, 4096)           # candidates carried through the merges (see the re-ranking below)
        cap = 4096
        while cap < 2 * kk:
            cap *= 2
        step = cap                      # n <= cap: the plan takes every row as a candidate (no threshold pass, tau = -inf)

        merged = None
        with torch.cuda.device(self.device):
            for pair, back in self._row_chunks(step, allowed):
                D, I = self._exact_slice(pair, kk, q, cap)
                I = torch.where(I >= 0, back(I.clamp_min(0)), I)
                merged = (D, I) if merged is None else tuple(t[:, :kk].contiguous() for t in merge_topk_device(merged, (D, I), kk))
            # The merges compare the fp32-rounded scores; the result's order is defined on the canonical fp64 scores (two
            # rows whose scores round to the same fp32 value are NOT a tie).  So each query's <= 2k survivors -- a superset
            # of its top-k: rounding is monotone -- are gathered in row order and ranked once more, exactly, as one slice.
            Dout = torch.empty((nq, k), dtype=torch.float32, device=self.device)
            Iout = torch.empty((nq, k), dtype=torch.int64, device=self.device)
            for j in range(nq):
                rows = merged[1][j] if merged is not None else Iout.new_empty(0)
                rows = torch.sort(rows[rows >= 0]).values
                m = int(rows.numel())
                if m == 0:
                    Dout[j] = PAD_SCORE
                    Iout[j] = -1
                    continue
                Dj, Ij = self._exact_slice(self._row_pair(rows), k, q[j:j + 1].contiguous(), cap)
                Dout[j] = Dj[0]
                Iout[j] = torch.where(Ij[0] >= 0, rows[Ij[0].clamp_min(0)], Ij[0])
        return Dout, Iout

    # -- range search: every row scoring above a per-query radius ----------------------------------------------------
    RANGE_MAX_CAP = 131072      # longest candidate list of convdr_ip_range_search (a power of two); beyond it: row slices

    def range_search(self, q, radius, allowed=None):
        """FAISS ``index.range_search`` with one radius per query: numpy ``(lims int64 [nq + 1], D float32, I int64)``; query j
        owns D / I [lims[j], lims[j + 1]) = every row whose canonical fp64 score is STRICTLY greater than float64(radius[j]),
        ordered by (score desc, row asc); D is that score rounded to fp32 (so it may equal the radius for a score above it by
        less than half an ulp).  radius: a float, or an fp32 vector [nq] (numpy or torch, host or device); a wrong length or a
        NaN raises ValueError.  allowed: a RowFilter or a mask, as for ``search`` -- the same set intersected with the allowed
        rows.  Exact whatever the store and the precision (include/convdr_hip.h, "Range search")."""
        lims, D, I = self.range_search_tensors(q, radius, allowed=allowed)
        return lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()

    def range_search_tensors(self, q, radius, allowed=None):
        """``range_search`` with the result left on the device.

        The ladder is a host loop with ONE host read (status, counts, total) per pass: the first pass lists up to ``self.cap``
        rows per query; a query whose scan hit more is re-run at the smallest power of two that holds its reported hit count
        (exact: no doubling), up to RANGE_MAX_CAP; CONVDR_IP_RANGE rebuilds the scan copy once (as search_finish).  Queries
        with more than RANGE_MAX_CAP hits take the last rung: the index is searched in row slices of at most RANGE_MAX_CAP
        rows (with a filter: slices of the ascending allowed rows), none of which can overflow, and the slices are merged on
        the device by the fp64 scores.  Memory bound of that rung: the result itself (fp64 score, row and query number per
        result row while merging) beside one call's workspace, which stays under DEEP_WS_BYTES.
        ``stats``: range_results, range_rounds (passes), range_cap (the longest list used), range_chunked_queries."""
        self._store.refuse(self, "range_search")
        return self._range(q, radius, allowed, False)

    def range_count(self, q, radius, allowed=None):
        """int64 numpy [nq]: how many rows ``range_search`` would return per query, without ordering or packing them
        (1 + range_count(q, score of a known positive) is that positive's exact rank in the whole index)."""
        self._store.refuse(self, "range_count")
        return self._range(q, radius, allowed, True)

    def _excluded_ahead(self, ex, f, qt, pairq, x_thr, row_thr):
        """convdr_ip_excl_count_ahead: device int64 [np], per pair (query pairq[p] of `qt`, threshold (x_thr[p], row_thr[p])) the
        rows of that query's exclusion list that are allowed by `f` and precede the threshold in the canonical order.  No sync."""
        import torch
        ptr = _lib.ptr
        npairs = int(pairq.numel())
        ahead = torch.zeros(npairs, dtype=torch.int64, device=self.device)
        if not npairs:
            return ahead
        store, r32, r16, scale, _ = self._operands(None if self.ntotal else (None, None))
        bits = None if f is None else f.bits
        pairq, x_thr, row_thr = pairq.to(torch.int32).contiguous(), x_thr.to(torch.float64).contiguous(), row_thr.to(torch.int64).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().convdr_ip_excl_count_ahead(
                store, ptr(qt), int(qt.shape[0]), r32, r16, scale, self.ntotal, self.d, ptr(bits), 0 if bits is None else bits.numel(),
                ptr(ex.rows), int(ex.rows.shape[1]), ptr(ex.count), npairs, ptr(pairq), ptr(x_thr), ptr(row_thr), ptr(ahead),
                _lib.stream_ptr()), "convdr_ip_excl_count_ahead")
        return ahead

    def _range_excluded(self, q, radius, allowed, count_only, exclude):
        """range_search / range_count with per-query exclusions: today's result, then the excluded rows taken out of it on the
        device (convdr_excl_count_ragged, the exclusive scan, convdr_excl_pack_ragged; one host read, the new total) -- or, for
        the count, the excluded allowed rows above the radius subtracted (nothing is listed).  ``stats`` gains excluded_dropped;
        range_results counts what is returned."""
        import torch
        L, ptr = _lib.lib(), _lib.ptr
        qt = self._queries(q)
        nq = int(qt.shape[0])
        f = self._filter(allowed)
        ex = self._exclusions(exclude, nq)
        res = self._range(q, radius, f, count_only)
        self.stats["excluded_dropped"] = 0
        if not nq or not ex.e_max:
            return res
        if count_only:
            rad = self._range_radius(radius, nq)
            ahead = self._excluded_ahead(ex, f, qt, torch.arange(nq, device=self.device), rad,
                                         torch.full((nq,), -1, dtype=torch.int64, device=self.device)).cpu().numpy()
            self.stats.update(excluded_dropped=int(ahead.sum()), range_results=int((res - ahead).sum()))
            return res - ahead
        lims, D, I = res
        total = int(I.numel())
        if not total:
            return res
        lims = lims.contiguous()
        ld = int(ex.rows.shape[1])
        out = torch.zeros(nq + 1, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.convdr_excl_count_ragged(ptr(lims), ptr(I), total, nq, ptr(ex.rows), ld, ptr(ex.count), ptr(out[1:]),
                                                  _lib.stream_ptr()), "convdr_excl_count_ragged")
            lims_out = torch.cumsum(out, 0)
            total_out = int(lims_out[-1].item())                # the one host read: it sizes the result
            Do = torch.empty(total_out, dtype=torch.float32, device=self.device)
            Io = torch.empty(total_out, dtype=torch.int64, device=self.device)
            if total_out:
                _lib.check(L.convdr_excl_pack_ragged(ptr(lims), ptr(D), ptr(I), total, nq, ptr(ex.rows), ld, ptr(ex.count), ptr(lims_out),
                                                     ptr(Do), ptr(Io), total_out, _lib.stream_ptr()), "convdr_excl_pack_ragged")
        self.stats.update(excluded_dropped=total - total_out, range_results=total_out)
        return lims_out, Do, Io

    def _range_radius(self, radius, nq):
        import torch
        r = torch.as_tensor(radius)
        if r.dim() == 0:
            r = r.reshape(1).expand(nq)
        elif r.dim() != 1 or int(r.numel()) != nq:
            raise ValueError("range_search: radius must be a number or a vector of nq = %d entries (got shape %s)"
                             % (nq, tuple(r.shape)))
        r = r.to(torch.float32).to(self.device).contiguous()
        if nq and bool(torch.isnan(r).any()):
            raise ValueError("range_search: a radius is NaN")
        return r

    def _range_pass(self, q, rad, cap, count_only, allowed=None, rows=None, want_x=False):
        """One pass of convdr_ip_range_search (+ convdr_ip_range_pack) over the resident block, or over `rows` = (re-score rows,
        scan copy) of a slice.  Returns (counts int64 numpy [nq], status numpy [nq], lims, D, I, X): the device result of the
        queries whose status is OK (the others own an empty run); lims / D / I / X are None when count_only, X unless want_x.
        One host read per call (status, counts and the total that sizes D and I)."""
        import torch
        L, ptr = _lib.lib(), _lib.ptr
        nq, n = int(q.shape[0]), self.ntotal if rows is None else int(rows[1].shape[0])
        # queries per call, so that one call's workspace stays under DEEP_WS_BYTES (as _enqueue splits the deep search)
        step, need = split_under(lambda c: L.convdr_ip_range_workspace_bytes(c, n, self.d, cap), nq, self.DEEP_WS_BYTES)
        if not need:
            raise _lib.ConvdrError("convdr_ip_range_search: sizes outside the contract (nq=%d n=%d d=%d cap=%d)" % (nq, n, self.d, cap))
        ws = self._workspace(need)
        store, r32, r16, scale, centre = self._operands(rows)
        bits = None if allowed is None else allowed.bits
        counts, status, parts = [], [], []
        with torch.cuda.device(self.device):
            for a in range(0, nq, step):
                b = min(nq, a + step)
                out = torch.empty(3 * (b - a) + 1, dtype=torch.int64, device=self.device)     # counts | lims | status (int32)
                cnt, lims, st = out[:b - a], out[b - a:2 * (b - a) + 1], out[2 * (b - a) + 1:].view(torch.int32)[:b - a]
                _lib.check(L.convdr_ip_range_search(
                    store, ptr(q[a:b]), b - a, r32, r16, scale, centre, n, self.d, ptr(self._max_norm), ptr(rad[a:b]), cap, int(count_only),
                    ptr(bits), 0 if bits is None else bits.numel(), ptr(ws), ws.numel(), ptr(cnt), ptr(lims), ptr(st),
                    _lib.stream_ptr()), "convdr_ip_range_search")
                host = out.cpu().numpy()                                                       # the pass's one host read
                counts.append(host[:b - a])
                status.append(host[2 * (b - a) + 1:].view(np.int32)[:b - a])
                if count_only:
                    continue
                total = int(host[2 * (b - a)])
                D = torch.empty(total, dtype=torch.float32, device=self.device)
                I = torch.empty(total, dtype=torch.int64, device=self.device)
                X = torch.empty(total, dtype=torch.float64, device=self.device) if want_x else None
                if total:       # (an empty tensor has no storage: its pointer is NULL, which the entry refuses)
                    _lib.check(L.convdr_ip_range_pack(ptr(ws), b - a, n, self.d, cap, ptr(lims), ptr(D), ptr(I), ptr(X),
                                                      _lib.stream_ptr()), "convdr_ip_range_pack")
                parts.append((lims, D, I, X, total))
        counts, status = np.concatenate(counts), np.concatenate(status)
        if count_only:
            return counts, status, None, None, None, None
        if len(parts) == 1:
            return (counts, status) + parts[0][:4]
        offs = np.concatenate([[0], np.cumsum([p[4] for p in parts])])
        lims = torch.cat([p[0][:-1] + int(o) for p, o in zip(parts, offs)] + [torch.tensor([int(offs[-1])], device=self.device)])
        return (counts, status, lims, torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]),
                torch.cat([p[3] for p in parts]) if want_x else None)

    def _range_chunked(self, q, rad, allowed, count_only):
        """The last rung: row slices of at most RANGE_MAX_CAP rows, each searched by the same entry with a list that holds the
        whole slice, merged per query into the canonical order -- stable sorts by row, then by fp64 score (descending), then
        by query.  Returns (counts numpy [nq], lims, D, I)."""
        import torch
        nq, cap = int(q.shape[0]), int(self.RANGE_MAX_CAP)
        counts = np.zeros(nq, np.int64)
        Xs, Is, Js = [], [], []
        for pair, back in self._row_chunks(cap, allowed):
            cnt, st, lims, D, I, X = self._range_pass(q, rad, cap, count_only, rows=pair, want_x=True)
            if (st != STATUS_OK).any():
                raise _lib.ConvdrError("convdr_ip_range_search: a slice of %d rows came back with status %s" % (pair[1].shape[0], st))
            counts += cnt
            if not count_only:
                Xs.append(X)
                Is.append(back(I))
                Js.append(torch.repeat_interleave(torch.arange(nq, device=self.device), torch.diff(lims)))
        if count_only:
            return counts, None, None, None
        X, I, J = torch.cat(Xs), torch.cat(Is), torch.cat(Js)
        for key, desc in ((lambda: I, False), (lambda: X, True), (lambda: J, False)):
            o = torch.sort(key(), stable=True, descending=desc).indices
            X, I, J = X[o], I[o], J[o]
        lims = torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]), device=self.device)
        return counts, lims, X.to(torch.float32), I

    def _count_ladder(self, who, n_items, one_pass, accept):
        """The ladder of the entries that report an EXACT count (range search: hits per query; rank: band rows per pair).
        A queue of (item numbers, cap) groups, one pass per group, starting with every item at min(self.cap, RANGE_MAX_CAP):
        one_pass(idx, sub, cap) -> (status, counts, result) runs the items idx (numpy; `sub` the same as a device index
        tensor, None for all items); accept(idx, sub, cap, ok, counts, result) keeps what a pass certified.  CONVDR_IP_RANGE
        rebuilds the scan copy once (as search_finish) and the group runs again; an item that overflowed is re-run once, at the
        smallest power of two that holds its count.  Returns (passes, the longest list used, the items whose count no list up
        to RANGE_MAX_CAP holds: the caller's last rung)."""
        import torch
        cap_max = int(self.RANGE_MAX_CAP)
        groups = [(np.arange(n_items), min(int(self.cap), cap_max))]
        passes, longest, beyond = 0, 0, []
        while groups:
            idx, cap = groups.pop(0)
            sub = None if len(idx) == n_items else torch.as_tensor(idx, device=self.device)
            st, cnt, result = one_pass(idx, sub, cap)
            passes, longest = passes + 1, max(longest, cap)
            if (st == STATUS_RANGE).any():
                if self._store.final_range(self):
                    raise _lib.ConvdrError("%s: %s" % (who, self._store.final_range(self)))
                if self.stats["rescaled"]:
                    raise _lib.ConvdrError("%s: CONVDR_IP_RANGE after the scan copy was rebuilt" % who)
                self._rebuild_scaled()
                self.stats["rescaled"] = 1
                groups.insert(0, (idx, cap))
                continue
            ok, over = st == STATUS_OK, st == STATUS_OVERFLOW
            if not (ok | over).all() or passes > 64:
                raise _lib.ConvdrError("%s: unexpected status %s" % (who, st))
            accept(idx, sub, cap, ok, cnt, result)
            # the reported count is exact and the thresholds do not change: the list that holds it cannot overflow -- one
            # jump, no doubling
            need = np.asarray([1 << int(c - 1).bit_length() for c in cnt[over]], dtype=np.int64)
            beyond += list(idx[over][need > cap_max])
            for c in sorted(set(need[need <= cap_max].tolist())):
                groups.append((idx[over][need == c], int(c)))
        return passes, longest, beyond

    def _range(self, q, radius, allowed, count_only):
        import torch
        qt = self._queries(q)
        nq = int(qt.shape[0])
        rad = self._range_radius(radius, nq)
        f = self._filter(allowed)
        self.stats = {"range_results": 0, "range_rounds": 0, "range_cap": 0, "range_chunked_queries": 0, "rescaled": 0}
        counts = np.zeros(nq, np.int64)
        pieces = []                         # (query numbers, lims, D, I) of every pass that certified a query

        def one_pass(idx, sub, cap):
            cnt, st, lims, D, I, _ = self._range_pass(qt if sub is None else qt[sub].contiguous(),
                                                      rad if sub is None else rad[sub].contiguous(), cap, count_only, allowed=f)
            return st, cnt, (lims, D, I)

        def accept(idx, sub, cap, ok, cnt, result):
            counts[idx[ok]] = cnt[ok]
            if not count_only and ok.any():
                pieces.append((idx,) + result)
        chunked = []
        if nq and self.ntotal and (f is None or f.n_allowed):
            rounds, longest, chunked = self._count_ladder("convdr_ip_range_search", nq, one_pass, accept)
            self.stats.update(range_rounds=rounds, range_cap=longest)
        if chunked:
            idx = np.asarray(sorted(chunked), dtype=np.int64)
            sub = torch.as_tensor(idx, device=self.device)
            cnt, lims, D, I = self._range_chunked(qt[sub].contiguous(), rad[sub].contiguous(), f, count_only)
            counts[idx] = cnt
            self.stats["range_chunked_queries"] = len(idx)
            self.stats["range_cap"] = max(self.stats["range_cap"], int(self.RANGE_MAX_CAP))     # (every slice's list)
            if not count_only:
                pieces.append((idx, lims, D, I))
        self.stats["range_results"] = int(counts.sum())
        if count_only:
            return counts
        if len(pieces) == 1 and len(pieces[0][0]) == nq:
            return pieces[0][1:]
        lims = torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]), device=self.device)
        total = self.stats["range_results"]
        Dout = torch.empty(total, dtype=torch.float32, device=self.device)
        Iout = torch.empty(total, dtype=torch.int64, device=self.device)
        for idx, lp, D, I in pieces:
            # result row e of the piece, owned by its query j, goes to lims[idx[j]] + (e - lp[j])
            shift = lims[torch.as_tensor(idx, device=self.device)] - lp[:-1]
            dest = torch.repeat_interleave(shift, torch.diff(lp)) + torch.arange(int(D.numel()), device=self.device)
            Dout[dest], Iout[dest] = D, I
        return lims, Dout, Iout

    # -- score and rank of given rows: where does a known row stand, and what does it score? -------------------------
    def score_rows(self, q, rows):
        """Canonical score of given rows (FAISS ``compute_distance_subset``): rows int64 [nq] (one row per query) or [nq, m],
        -1 = padding; float32 numpy of the same shape, the fp32 rounding of the canonical fp64 score that ``search`` ranks by
        (``search(q, k)`` followed by ``score_rows(q, I)`` reproduces D bit for bit), padding -> -3.4028235e38.  numpy (or
        host tensor) ids >= ntotal raise ValueError; ids in a device tensor are not read on the host: outside [0, ntotal)
        they score as padding."""
        return self.score_rows_tensors(q, rows)[0].cpu().numpy()

    def score_rows_tensors(self, q, rows):
        """``score_rows`` on the device: (D float32, X float64), both of the shape of `rows`; X is the canonical score itself."""
        import torch
        qt, rt, shape = self._rows_arg("score_rows", q, rows)
        nq, m = int(rt.shape[0]), int(rt.shape[1])
        D = torch.empty((nq, m), dtype=torch.float32, device=self.device)
        X = torch.empty((nq, m), dtype=torch.float64, device=self.device)
        if nq and m:
            n = self.ntotal
            ops = self._operands(None if n else (None, None))      # (an empty index passes no rows)
            suffix, head, rows = self._store.call("score", ops)
            with torch.cuda.device(self.device):
                name = "convdr_ip_score_rows" + suffix
                _lib.check(getattr(_lib.lib(), name)(*head, _lib.ptr(qt), nq, *rows, n, self.d, _lib.ptr(rt), m, m, _lib.ptr(X), _lib.ptr(D),
                                                     _lib.stream_ptr()), name)
        return D.reshape(shape), X.reshape(shape)

    def rank_rows(self, q, rows, allowed=None):
        """Exact rank of given rows: rows int64 [nq] or [nq, m], -1 = padding; int64 numpy of the same shape: the number of rows
        of the index (with ``allowed``: of the allowed rows) that precede the given row in the canonical order of ``search`` --
        canonical fp64 score descending, row ascending --, 0-based, -1 for padding.  ``search(q, k)[1][j, rank] == row``
        whenever rank < k.  The row itself need not be allowed: with the known positives masked out this is "the rank among
        the rows that are not known positives".  Exact at any depth, whatever the store and the precision; exact ties (duplicate
        rows) are ordered by row, as ``search`` orders them.  ids are checked as for ``score_rows``."""
        return self.rank_rows_tensors(q, rows, allowed=allowed).cpu().numpy()

    def rank_rows_tensors(self, q, rows, allowed=None):
        """``rank_rows`` with the result left on the device (int64, the shape of `rows`).

        Every (query, row) pair becomes one query of convdr_ip_rank_rows (include/convdr_hip.h, "Score and rank of given
        rows"): one scan counts the rows that certainly precede the target and lists only those within the scan's error band
        of its score, which are re-scored exactly.  The host loop and its fallback are ``_rank_ladder``.
        ``stats``: rank_rounds (passes), rank_cap (the longest band list used), rank_band_rows (band entries re-scored, all
        passes), rank_above (rows counted without a re-score, final passes), rank_fallback_pairs, rescaled."""
        return self._rank_rows_tensors(q, rows, allowed, None)

    def _rank_rows_tensors(self, q, rows, allowed, exclude):
        """rank_rows_tensors, with per-query exclusions (``excluding(ex).rank_rows_tensors``) or None"""
        import torch
        self._store.refuse(self, "rank_rows")
        qt, rt, shape = self._rows_arg("rank_rows", q, rows)
        f = self._filter(allowed)
        ex = self._exclusions(exclude, int(qt.shape[0]))
        tp = rt.reshape(-1).contiguous()
        out, X = self._rank_ladder_scores("convdr_ip_rank_rows", qt, tp, f, lambda qs, ts, cap: self._rank_pass(qs, ts, cap, f),
                                          lambda I, ahead, t: ahead.sum())
        if ex is not None and ex.e_max and X is not None:
            # whatever rung ranked a pair: minus the excluded allowed rows that precede its target, counted against the
            # target's fp64 score the ladder holds on the device (a padding target keeps its -1)
            pairq = torch.arange(int(tp.numel()), device=self.device) // int(rt.shape[1])
            out = torch.where(out >= 0, out - self._excluded_ahead(ex, f, qt, pairq, X, tp), out)
        return out.reshape(shape)

    def _rank_ladder(self, who, qt, tp, f, run_pass, count_ahead, **more_stats):
        """``_rank_ladder_scores`` without the scores"""
        return self._rank_ladder_scores(who, qt, tp, f, run_pass, count_ahead, **more_stats)[0]

    def _rank_ladder_scores(self, who, qt, tp, f, run_pass, count_ahead, **more_stats):
        """The host loop of rank_rows_tensors / rank_ids_tensors: device int64 [np], the rank of every pair (query j // m of `qt`,
        target row tp[j]).  It reads ONE tensor per pass, run_pass(queries, targets, cap) = _rank_pass / _rank_docs_pass: the first
        pass runs at ``self.cap``; a pair whose band overflowed is re-run once at the smallest power of two that holds the reported
        band count, up to RANGE_MAX_CAP; CONVDR_IP_RANGE rebuilds the scan copy once (as search_finish).  A pair whose band holds
        more than RANGE_MAX_CAP rows -- more duplicates or near-duplicates of the target than that -- takes the fallback: a
        ``range_search`` just below the target's score (which has its own row-slice rung), the canonical fp64 scores of the rows
        I it returns, and count_ahead(I, mask of the rows that precede the target, target row).  Correct, not fast.
        Returns (ranks, X): X the targets' canonical fp64 scores, device float64 [np], as the entry wrote them on whatever
        rung (None when nothing was ranked: no pair, or an empty index)."""
        import torch
        npairs = int(tp.numel())
        self.stats = {"rank_rounds": 0, "rank_cap": 0, "rank_band_rows": 0, "rank_above": 0, "rank_fallback_pairs": 0, "rescaled": 0,
                      **more_stats}
        out = torch.full((npairs,), -1, dtype=torch.int64, device=self.device)
        if not npairs or not self.ntotal:
            return out, None
        qt = self._queries(qt, padded_ok=True)
        qp = qt if npairs == int(qt.shape[0]) else qt.repeat_interleave(npairs // int(qt.shape[0]), dim=0)
        tp = tp.contiguous()
        X = torch.empty(npairs, dtype=torch.float64, device=self.device)

        def one_pass(idx, sub, cap):
            rank, cnt, above, st, Xs = run_pass(qp if sub is None else qp[sub].contiguous(),
                                                tp if sub is None else tp[sub].contiguous(), cap)
            return st, cnt, (rank, above, Xs)

        def accept(idx, sub, cap, ok, cnt, result):
            nonlocal out, X
            rank, above, Xs = result
            self.stats["rank_band_rows"] += int(np.minimum(cnt, cap).sum())
            self.stats["rank_above"] += int(above[ok].sum())
            if sub is None:
                out, X = torch.as_tensor(rank, device=self.device), Xs
            else:
                out[sub], X[sub] = torch.as_tensor(rank, device=self.device), Xs
        rounds, longest, fallback = self._count_ladder(who, npairs, one_pass, accept)
        self.stats.update(rank_rounds=rounds, rank_cap=longest)
        if fallback:
            stats = self.stats
            stats["rank_fallback_pairs"] = len(fallback)
            xs = X[torch.as_tensor(np.asarray(fallback, dtype=np.int64), device=self.device)].cpu().numpy()
            for j, x in zip(fallback, xs):
                t = tp[j]
                qj = qp[j:j + 1].contiguous()
                _, _, I = self.range_search_tensors(qj, _radius_below(x), allowed=f)
                Xr = self.score_rows_tensors(qj, I[None, :])[1][0]
                out[j] = count_ahead(I, (Xr > float(x)) | ((Xr == float(x)) & (I < t)), t)
            self.stats = stats
        return out, X

    def _rows_arg(self, who, q, rows):
        """(queries device fp32 [nq, d], rows device int64 [nq, m], the shape of `rows`); the checks that need no device"""
        import torch
        qt, rt, nq, fits = self._pairs_arg(who, q, rows)
        if not fits:
            raise ValueError("%s: rows must be [nq] or [nq, m] with nq = %d (got shape %s)" % (who, nq, tuple(rt.shape)))
        if rt.is_floating_point() or rt.dtype == torch.bool:
            raise ValueError("%s: rows must be integers (got %s)" % (who, rt.dtype))
        shape = tuple(rt.shape)
        if rt.device.type == "cpu" and rt.numel() and int(rt.max()) >= self.ntotal:
            raise ValueError("%s: row id %d >= ntotal = %d" % (who, int(rt.max()), self.ntotal))
        qt = self._queries(qt, padded_ok=True)
        rt = rt.to(torch.int64).to(self.device).reshape(nq, -1).contiguous()
        return qt, rt, shape

    def _rank_pass(self, qp, tp, cap, allowed=None):
        """One pass of convdr_ip_rank_rows over the resident block: (rank, band counts, above, status) numpy [np] and the
        targets' fp64 scores (device).  One host read per call."""
        return self._rank_entry_pass(qp, tp, cap, allowed, None)

    def _rank_docs_pass(self, qp, tp, cap, ordinals, allowed=None):
        """One pass of convdr_ip_rank_docs: as _rank_pass, `rank` counting documents and `above` the rows the scan marked."""
        return self._rank_entry_pass(qp, tp, cap, allowed, ordinals)

    def _rank_entry_pass(self, qp, tp, cap, allowed, ordinals):
        """convdr_ip_rank_rows (ordinals None) or convdr_ip_rank_docs over the resident block"""
        import torch
        L, ptr = _lib.lib(), _lib.ptr
        npairs, n = int(qp.shape[0]), self.ntotal
        who = "convdr_ip_rank_rows" if ordinals is None else "convdr_ip_rank_docs"
        if ordinals is None:
            ws_bytes = lambda c: L.convdr_ip_rank_workspace_bytes(c, n, self.d, cap)
        else:
            ws_bytes = lambda c: L.convdr_ip_rank_docs_workspace_bytes(c, n, self.d, cap, ordinals.ndocs)
        # pairs per call, so that one call's workspace stays under DEEP_WS_BYTES (as _range_pass)
        step, need = split_under(ws_bytes, npairs, self.DEEP_WS_BYTES)
        if not need:
            raise _lib.ConvdrError("%s: sizes outside the contract (np=%d n=%d d=%d cap=%d)" % (who, npairs, n, self.d, cap))
        ws = self._workspace(need)
        store, r32, r16, scale, centre = self._operands()
        bits = None if allowed is None else allowed.bits
        X = torch.empty(npairs, dtype=torch.float64, device=self.device)
        hosts = []
        with torch.cuda.device(self.device):
            for a in range(0, npairs, step):
                b = min(npairs, a + step)
                c = b - a
                out = torch.empty(4 * c, dtype=torch.int64, device=self.device)      # rank | counts | above | status (int32)
                block = (store, ptr(qp[a:b]), c, ptr(tp[a:b]), r32, r16, scale, centre, n, self.d, ptr(self._max_norm), ptr(bits),
                         0 if bits is None else bits.numel(), 0 if allowed is None else allowed.n_allowed)
                outs = (cap, ptr(ws), ws.numel(), ptr(out[:c]), ptr(X[a:b]), ptr(out[c:2 * c]), ptr(out[2 * c:3 * c]), ptr(out[3 * c:]),
                        _lib.stream_ptr())
                if ordinals is None:
                    _lib.check(L.convdr_ip_rank_rows(*block, *outs), who)
                else:
                    _lib.check(L.convdr_ip_rank_docs(*block, ptr(ordinals.ord), ordinals.ndocs, *outs), who)
                host = out.cpu().numpy()                                             # the pass's one host read
                hosts.append((host[:c], host[c:2 * c], host[2 * c:3 * c], host[3 * c:].view(np.int32)[:c]))
        return tuple(np.concatenate([h[i] for h in hosts]) for i in range(4)) + (X,)

    # -- document rank: where does a known DOCUMENT stand among the documents? ----------------------------------------------
    def rank_ids(self, q, ids, allowed=None, ordinals=None):
        """Exact rank of given documents: ids int64 [nq] (one document per query) or [nq, m], numpy or torch, host or device;
        int64 numpy of the same shape: the number of documents that precede the document ids[j, c] in the order of
        ``search_docs`` -- a document stands where its best row stands: canonical fp64 score descending, row ascending --,
        0-based; -1 for an id on no row (INT64_MIN included).  ``search_docs(q, k)[1][j, rank] == id`` whenever 0 <= rank < k;
        on an index whose ids are all distinct, ``rank_ids(q, ids) == rank_rows(q, rows_of(ids))``.  Exact at any depth,
        whatever the store and the precision.
        allowed (as for ``rank_rows``): the document's best row is taken over ALL its rows, as ``score_ids`` does -- it need
        not be allowed --, and the competitors are counted among the allowed rows only: "the rank among the documents that
        are not known positives".  Consequently ``search_docs(q, k, allowed=f)`` places the document at `rank` whenever its
        best row is allowed.  ordinals: a DocOrdinals of this index (``doc_ordinals()``), built here when not given."""
        return self.rank_ids_tensors(q, ids, allowed=allowed, ordinals=ordinals)[0].cpu().numpy()

    def rank_ids_tensors(self, q, ids, allowed=None, ordinals=None):
        """``rank_ids`` on the device: (rank int64, D float32, R int64), all of the shape of `ids`; (D, R) is the MaxP pair of
        ``score_ids_tensors``: the document's score and its best row.

        ``score_ids_tensors`` finds every document's best row; every (query, best row) pair becomes one query of
        convdr_ip_rank_docs (include/convdr_hip.h, "Document rank"): the band-count scan of ``rank_rows`` whose rows above
        the band mark their document in a bitmap of ndocs bits per pair instead of being counted only, the re-scored band
        rows that precede the target mark theirs afterwards, and the rank is the bitmap's population with the target's own
        document left out.  The host loop is ``_rank_ladder``; its fallback counts the distinct ids of the rows that precede the
        target, the target's own id dropped.
        ``stats``: rank_rounds, rank_cap, rank_band_rows (band entries re-scored, all passes), rank_above (ROWS marked without
        a re-score, final passes), rank_fallback_pairs, rescaled, ndocs."""
        import torch
        self._store.refuse(self, "rank_ids")
        self._need_ids("rank_ids")
        qt, it, shape = self._ids_arg("rank_ids", q, ids)
        f = self._filter(allowed)
        o = self._ordinals(ordinals)
        D, R = self.score_ids_tensors(qt, it)
        o = o or self.doc_ordinals()
        col = self.ids

        def docs_ahead(I, ahead, t):            # the distinct ids on the rows that precede the target row, its own left out
            ahead = col[I[ahead]]
            return torch.unique(ahead[ahead != col[t]]).numel()
        # (an id on no row has best row -1: the entry's padding, rank -1)
        out = self._rank_ladder("convdr_ip_rank_docs", qt, R.reshape(-1), f, lambda qs, ts, cap: self._rank_docs_pass(qs, ts, cap, o, f),
                                docs_ahead, ndocs=o.ndocs)
        return out.reshape(shape), D, R


class ExcludedSearch:
    """``FlatIPIndex.excluding(exclude)``: the exact entries of an index with rows left out PER QUERY -- the known positives of
    each query, the passages of its earlier turns, the stored row that is the query itself -- where ``allowed=`` is one set for the
    whole call.  Every entry has the name, the arguments and the result of the index's own and is exact and certified at every
    depth, for both stores and every precision, alone or with ``allowed=``: the canonical order of the (allowed) rows with query
    j's rows removed.  exclude: a QueryExclusions (reusable), or a raw int64 [nq, e] array / list of nq lists built for each call.
    No new scan ("Per-query exclusions"): the certified search runs at ONE depth for the whole call,
    k + e_max (the longest list; `stats["exclude_depth"]`), and the excluded rows are dropped from its lists on the device
    (`stats["excluded_dropped"]`) -- callers whose lists are very uneven should group their queries by list length; ranks and
    range counts subtract the excluded allowed rows that precede the threshold (the target of a rank never counts, so a query
    may exclude its own target).  Not offered: rank_ids, the single uncertified pass, search_distinct with caller keys, the
    block-file and sharded searches."""

    def __init__(self, index, exclude):
        self.index, self.exclude = index, exclude

    def search(self, q, k, allowed=None):
        D, I = self.search_tensors(q, k, allowed=allowed)
        return D.cpu().numpy(), I.cpu().numpy()

    def search_tensors(self, q, k, allowed=None):
        return self.index.search_finish(self.search_begin(q, k, allowed=allowed))

    def search_begin(self, q, k, allowed=None):
        """the handle for ``index.search_finish``: opaque, it carries the exclusions and the caller's k"""
        return self.index._search_begin_excluded(q, k, allowed, self.exclude)

    def search_ids(self, q, k, allowed=None):
        D, I = self.search_ids_tensors(q, k, allowed=allowed)
        return D.cpu().numpy(), I.cpu().numpy()

    def search_ids_tensors(self, q, k, allowed=None):
        self.index._need_ids("search_ids")
        return self.index._ids_of(*self.search_tensors(q, k, allowed=allowed))

    def search_docs(self, q, k, allowed=None, depth=None, strict=True, max_depth=None):
        """the exclusion is applied to the row lists before the distinct cut: a document whose rows are all excluded
        disappears for that query, one with some rows excluded is represented by its best remaining row"""
        return self.index._search_docs(q, k, allowed, depth, strict, max_depth, self.exclude)

    def range_search(self, q, radius, allowed=None):
        lims, D, I = self.range_search_tensors(q, radius, allowed=allowed)
        return lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()

    def range_search_tensors(self, q, radius, allowed=None):
        return self.index._range_excluded(q, radius, allowed, False, self.exclude)

    def range_count(self, q, radius, allowed=None):
        return self.index._range_excluded(q, radius, allowed, True, self.exclude)

    def rank_rows(self, q, rows, allowed=None):
        """``search(q, k)[1][j, rank] == row`` of this view whenever rank < k and the row is not excluded itself"""
        return self.rank_rows_tensors(q, rows, allowed=allowed).cpu().numpy()

    def rank_rows_tensors(self, q, rows, allowed=None):
        return self.index._rank_rows_tensors(q, rows, allowed, self.exclude)
