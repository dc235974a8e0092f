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
import json
import os
import pickle
import warnings

import numpy as np

from . import _lib

def _torch():
    import torch
    return torch


STATUS_OK, STATUS_OVERFLOW, STATUS_TOO_FEW, STATUS_UNCERTAIN, STATUS_RANGE = 0, 1, 2, 3, 4
PAD_SCORE = -3.4028234663852886e38      # what IndexFlatIP.search returns beside id -1

_KINDS = {"auto": "f16", "fp16": "f16", "fp16x3": "f16", "bf16": "bf16", "bf16x3": "bf16", "fp16x2": "f16"}
_SPLIT = ("bf16x3", "fp16x3", "fp16x2")          # precisions that pin the second rung
_HALF_PRECISIONS = ("auto", "fp16", "fp16x2")    # the rungs of a half store (storage="fp16")
HALF_NORM_LIMIT = 60000.0                        # csrc/ip_topk.hip: IP_F16_NORM_LIMIT


_Depth = collections.namedtuple("_Depth", "enqueue max_cap shortcut last_rung last_stat deep_stats")
# what search_begin hands to search_finish: depth None = k > DEEP_MAX_K (nothing enqueued), first = (D, I, status, tau_retry) of
# the enqueued first pass or None (nothing to scan: deep search of an empty index, or a filter that allows no row),
# allowed = the RowFilter of a restricted search or None
_Pending = collections.namedtuple("_Pending", "qt k depth x3 cap first allowed", defaults=(None,))

RESERVED_ID = -(1 << 63)    # INT64_MIN: the free-slot marker of the key set (csrc/ip_keys.hpp), no legal row id
KEY_ST_LIST, KEY_ST_PROBE, KEY_ST_COLUMN, KEY_ST_NOSET = 1, 2, 4, 8      # status bits of convdr_keyset_build / the row passes
ROW_FILTER_TILE = 256       # the bitmap covers whole scan tiles of this many rows (csrc/ip_topk.hip: Tile256::TR)


def pack_row_mask(mask):
    """bool / uint8 vector [n] (a torch tensor, on any device) -> the bitmap of convdr_ip_search_filtered: int32 words (the bytes
    of uint32), row r allowed iff bit r & 31 of word r >> 5 is set, zero padded to whole 256-row tiles (ceil(n / 256) * 8 words).
    Torch ops on the mask's device: eight rows make a byte (least significant bit first), four bytes a little-endian word."""
    import torch
    m = mask.reshape(-1) != 0
    n = int(m.numel())
    padded = (n + ROW_FILTER_TILE - 1) // ROW_FILTER_TILE * ROW_FILTER_TILE
    if padded != n:
        m = torch.cat([m, torch.zeros(padded - n, dtype=torch.bool, device=m.device)])
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=m.device)
    by = (m.view(-1, 8).to(torch.int32) * weights).sum(1).to(torch.uint8)         # (at most 255)
    return by.contiguous().view(torch.int32)


def split_under(ws_bytes, count, budget):
    """(items per call, workspace bytes of one such call): the items of one request -- queries, (query, row) pairs -- are halved
    until ws_bytes(items), the entry's own workspace function, fits `budget` (None: never split); the calls then run back to
    back on the stream and share the buffer.  A single item is never split, and 0 bytes means sizes outside the entry's
    contract: the caller raises, in its own words."""
    step = count
    while budget is not None and step > 1 and ws_bytes(step) > budget:
        step = (step + 1) // 2
    return step, ws_bytes(step)


class RowFilter:
    """An allowed subset of an index's rows (FlatIPIndex.row_filter): `bits` the device bitmap (pack_row_mask), `n` the ntotal
    it was built for -- searching an index of another size with it raises ValueError --, `n_allowed` the number of allowed rows."""

    def __init__(self, bits, n, n_allowed):
        self.bits, self.n, self.n_allowed = bits, int(n), int(n_allowed)
        self._rows = None

    def rows(self):
        """ascending ids of the allowed rows (device int64 [n_allowed]), unpacked from the bitmap on first use: the last rungs
        of the ladder rank explicit row lists"""
        import torch
        if self._rows is None:
            by = self.bits.view(torch.uint8).to(torch.int32)
            shifts = torch.arange(8, dtype=torch.int32, device=by.device)
            self._rows = torch.nonzero(((by[:, None] >> shifts) & 1).reshape(-1)[:self.n]).flatten()
        return self._rows


class DocOrdinals:
    """Dense document numbers of an index's id column (FlatIPIndex.doc_ordinals): `ord` the device vector [ntotal] (int32
    words, the bytes of uint32: ord[r] = the number of distinct ids whose first row lies below the first row of ids[r]),
    `ndocs` the distinct ids, `n` the ntotal it was built for -- ranking with it on an index of another size raises ValueError.
    Query independent: build once, pass as ``ordinals=`` to rank_ids / rank_ids_tensors."""

    def __init__(self, ord, ndocs, n):
        self.ord, self.ndocs, self.n = ord, int(ndocs), int(n)


class FlatIPIndex:
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
    unchanged) rows with a value that is not finite as a half or with a norm above 60,000."""

    def __init__(self, d, device=None, cap=4096, rank_target=0, precision="auto", center=None, prepin=True, storage="fp32"):
        if storage not in ("fp32", "fp16"):
            raise ValueError("FlatIPIndex: storage must be 'fp32' or 'fp16' (got %r)" % (storage,))
        if storage == "fp16":
            if precision not in _HALF_PRECISIONS:
                raise ValueError("FlatIPIndex(storage='fp16'): precision must be one of %s (got %r)" % (_HALF_PRECISIONS, precision))
            if center:
                raise ValueError("FlatIPIndex(storage='fp16'): the half store is not centred (center=True)")
            center = False
        elif center is None:
            center = True
        import torch
        if not torch.cuda.is_available():
            raise _lib.ConvdrError("FlatIPIndex needs a GPU (no CPU fallback)")
        assert precision in _KINDS and (storage == "fp16" or precision != "fp16x2"), precision
        self.storage, self._half = storage, storage == "fp16"
        _lib.lib()
        # the scan contracts in 64-wide K steps: other widths get zero columns, which add exact zeros to every score
        self.d_in = int(d)
        self.d = (self.d_in + 63) // 64 * 64
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.cap, self.rank_target = int(cap), int(rank_target)
        self.precision, self.center = precision, bool(center)
        self.kind = _KINDS[precision]
        self._half_dtype = torch.float16 if self.kind == "f16" else torch.bfloat16
        self.host_chunk_bytes = 64 << 20       # staging-buffer size of the streamed host -> HBM path (add); 64 MB x 16
                                               # threads measured best on the bench host (tools/dbg/block_load_sweep.py)
        self.host_copy_threads = 16            # file reads / memcpy slices in flight while filling a staging buffer
        self.host_stage_buffers = 4            # pinned staging buffers (3 chunks being read while one crosses PCIe; 37-41 GB/s of a
                                               # 44 GB/s pinned-H2D ceiling on the r03 box, tools/dbg/block_load_sweep.py)
        self.compact_window_rows = 65536       # rows per window of keep_rows / remove_rows (a multiple of 256): the bounce buffer
                                               # holds one window of the widest buffer, 192 MB at d = 768; best of the sweep
                                               # 1,024 .. 262,144 at 1 M rows (profiles/compact_rows_time.txt)
        self.stats = {}
        self._s32 = self._s16 = self._slo = None
        self.reset()
        if prepin:
            self.prepin_staging()

    def prepin_staging(self, wait=False):
        """Allocate and page-lock the process-wide staging buffers of the block loader (4 x 64 MB on the GPU's NUMA node, ~60 ms)
        NOW, on a background thread: the first add() of a block file used to pay for it (19 GB/s against 49 GB/s for every
        later block; the reference's flow constructs the index, then loads 8 block files: run_convdr_inference.py:353,164-180).
        Called by the constructor (prepin=True); add() joins the thread if it is still running."""
        import threading
        key = _staging_key(self.device, self.d, max(2, int(self.host_stage_buffers)))
        rows = max(1, int(self.host_chunk_bytes) // (4 * self.d))
        with _STAGING_LOCK:
            ent = _STAGING.get(key)
            th = _STAGING_THREADS.get(key)
            if (ent is not None and ent[0][0].shape[0] >= rows) or (th is not None and th.is_alive()):
                pass
            else:
                th = threading.Thread(target=_staging, args=(self.device, rows, self.d, key[2]), daemon=True, name="convdr-prepin")
                _STAGING_THREADS[key] = th
                th.start()
        if wait and th is not None:
            th.join()

    def twin(self):
        """An empty index with this one's parameters (search_one_by_one keeps two blocks in flight: one being searched, one
        being loaded)."""
        t = FlatIPIndex(self.d_in, device=self.device, cap=self.cap, rank_target=self.rank_target, precision=self.precision,
                        center=None if self._half else self.center, prepin=False, storage=self.storage)
        t.host_chunk_bytes, t.host_copy_threads, t.host_stage_buffers = self.host_chunk_bytes, self.host_copy_threads, self.host_stage_buffers
        return t

    # -- faiss-like surface ---------------------------------------------------
    @property
    def ntotal(self):
        return self._n

    # the resident block (views of the used rows of the backing storage)
    @property
    def _p32(self):
        return None if self._s32 is None else self._s32[:self._n]

    @property
    def _pbf(self):
        return None if self._s16 is None else self._s16[:self._n]

    @property
    def _plo(self):
        return None if self._slo is None else self._slo[:self._n]

    @property
    def _rows(self):
        """The rows the canonical re-score reads: the fp32 block, or the half store itself."""
        return self._pbf if self._half else self._p32

    @property
    def store(self):
        """storage="fp16": the resident halves [ntotal, d] = 2^s x the stored passages (s: ``_scale``)."""
        return self._pbf if self._half else None

    def _row_pair(self, sel):
        """(re-score rows, scan copy) of a slice or an index vector of the resident rows, contiguous"""
        if self._half:
            r = self._pbf[sel].contiguous()
            return r, r
        return self._p32[sel].contiguous(), self._pbf[sel].contiguous()

    def _operands(self, rows=None):
        """What a block looks like to the C ABI: (store code 0 bf16 / 1 fp16 / 2 half store, fp32 rows or NULL, 16-bit operand,
        scale of that operand, centre or NULL) of the resident block, or of `rows` = (re-score rows, scan copy) of a slice.  The
        half store has no fp32 rows and no centre, the bf16 copy no scale."""
        ptr = _lib.ptr
        p32, p16 = (self._rows, self._pbf) if rows is None else rows
        store = 2 if self._half else (1 if self.kind == "f16" else 0)
        return (store, None if self._half else ptr(p32), ptr(p16), float(self._scale) if store else 1.0,
                None if self._half else ptr(self._centre))

    def _queries(self, q, padded_ok=False):
        """The queries as every entry reads them: fp32 [nq, d] on the index's device, contiguous, the zero columns of a padded
        width appended (padded_ok: a tensor that already has them is taken as it is)."""
        import torch
        qt = torch.as_tensor(q)
        if qt.dtype != torch.float32:
            qt = qt.float()
        if self.d != self.d_in and not (padded_ok and qt.dim() == 2 and qt.shape[1] == self.d):
            qt = self._pad_columns(qt)
        qt = qt.to(self.device).contiguous()
        assert qt.dim() == 2 and qt.shape[1] == self.d
        return qt

    def reset(self):
        """faiss ``index.reset()``: forget the passages.  A reservation made with reserve() survives (its memory is reused
        by the next block); ``release()`` drops it."""
        import torch
        self._n = 0
        if not getattr(self, "_reserved", False):
            self._s32 = self._s16 = self._slo = None
        self._sid = self._sid_spare = None      # the id column and its ping-pong partner (keep_rows): an index has ids or not,
                                                # from its first add on; a reset forgets that too
        self._centre = None
        self._scale = 1.0                       # power of two applied to the fp16 scan copy (1 for bf16)
        self._max_norm = torch.zeros(1, dtype=torch.float32, device=self.device)
        if self._half:
            # max norm and the flag word of convdr_ip_store_rows_f16 side by side: ONE host read at the end of an add()
            self._mf = torch.zeros(3, dtype=torch.float32, device=self.device)
            self._max_norm, self._flags = self._mf[:1], self._mf[1:2].view(torch.int32)
            self._uflags = self._mf[2:].view(torch.int32)       # update_rows has a flag word of its own: update_flags()
        self._ws = None
        self._x3_first = False
        if not hasattr(self, "_copy_stream"):
            self._copy_stream, self._stage = None, None

    def release(self):
        self._reserved = False
        self.reset()

    def reserve(self, n, lo=None):
        """Backing storage for n passages (fp32 block + 16-bit scan copy, + the remainder copy of the split scan when
        `lo`, default: only if the precision pins it; + the id column of an index that carries ids).  Existing rows are kept."""
        import torch
        held = {"_s16": self._half_dtype}          # the buffers this index holds: a half store keeps its 16-bit rows and nothing else
        if not self._half:
            held["_s32"] = torch.float32
            if self._slo is not None or ((self.precision in ("bf16x3", "fp16x3")) if lo is None else bool(lo)):
                held["_slo"] = self._half_dtype
        rows = max(int(n), 0 if self._s16 is None else self._s16.shape[0])      # (all of them keep one row count)
        with torch.cuda.device(self.device):
            for name, dtype in held.items():
                old = getattr(self, name)
                if old is None or old.shape[0] < rows:
                    t = torch.empty((rows, self.d), dtype=dtype, device=self.device)
                    if old is not None and self._n:
                        t[:self._n].copy_(old[:self._n])
                    setattr(self, name, t)
            if getattr(self, "_sid", None) is not None:
                self._reserve_ids(rows)
        self._reserved = True

    def _reserve_ids(self, rows, keep=None):
        """the id column for `rows` rows (the first `keep` entries kept, default ntotal); its ping-pong partner is re-made on
        its next use"""
        import torch
        keep = self._n if keep is None else keep
        if self._sid is None or self._sid.shape[0] < rows:
            t = torch.empty(int(rows), dtype=torch.int64, device=self.device)
            if self._sid is not None and keep:
                t[:keep].copy_(self._sid[:keep])
            self._sid, self._sid_spare = t, None

    def _prepare_into(self, src32, dst16, dstlo):
        """scan copy (and remainder copy) of the fp32 rows `src32`; folds their norms into the block's max norm"""
        L = _lib.lib()
        if self.kind == "f16":
            _lib.check(L.convdr_ip_prepare_block_f16(_lib.ptr(src32), src32.shape[0], self.d, _lib.ptr(self._centre),
                                                     float(self._scale), _lib.ptr(dst16), _lib.ptr(dstlo),
                                                     _lib.ptr(self._max_norm), _lib.stream_ptr()), "convdr_ip_prepare_block_f16")
        else:
            _lib.check(L.convdr_ip_prepare_block(_lib.ptr(src32), src32.shape[0], self.d, _lib.ptr(self._centre), _lib.ptr(dst16),
                                                 _lib.ptr(dstlo), _lib.ptr(self._max_norm), _lib.stream_ptr()),
                       "convdr_ip_prepare_block")

    def _first_rows(self, t):
        """The first rows an empty index sees fix its centring vector and, for the fp16 scan, the power-of-two scale of the
        scan copy (from these rows' largest centred norm: one extra pass over them and one host read per index
        lifetime; later rows may be up to 7x longer before the copy has to be rebuilt, see _rebuild_scaled)."""
        if self.center:
            self._set_centre(t)
        if self.kind == "f16":
            L = _lib.lib()
            _lib.check(L.convdr_ip_prepare_block_f16(_lib.ptr(t), t.shape[0], self.d, _lib.ptr(self._centre), 1.0, None, None,
                                                     _lib.ptr(self._max_norm), _lib.stream_ptr()), "convdr_ip_prepare_block_f16")
            self._scale = float(L.convdr_ip_f16_scale(float(self._max_norm.item())))

    def _rebuild_scaled(self):
        """CONVDR_IP_RANGE: rows added after the scale was fixed are more than 7x longer than the first block's longest.
        Re-derive the scale from the block's max norm and rebuild the fp16 copies from the resident fp32 rows."""
        import torch
        if self._half:
            # the half store is rescaled IN PLACE by 2^(s_new - s_old) <= 1, s_new >= 0: exact (convdr_ip_store_rows_f16)
            new = max(1.0, float(_lib.lib().convdr_ip_f16_scale(float(self._max_norm.item()))))
            with torch.cuda.device(self.device):
                if self._n and new != self._scale:
                    self._store_rows(self._pbf, self._pbf, new / self._scale, fold_norm=False)
                    if int(self._flags.item()):
                        raise _lib.ConvdrError("half store: the in-place rescale %g -> %g was not exact" % (self._scale, new))
            self._scale = new
            return
        with torch.cuda.device(self.device):
            self._scale = float(_lib.lib().convdr_ip_f16_scale(float(self._max_norm.item())))
            if self._n:
                self._prepare_into(self._p32, self._pbf, self._plo)

    def _grow_for(self, m, want_lo=False):
        """rows [n, n + m) of the backing storage (fp32 block, scan copy, remainder copy; None for a buffer the index does not
        hold), growing it when needed (exact fit unless reserved larger)"""
        need = self._n + m
        if self._s16 is None or self._s16.shape[0] < need or (want_lo and self._slo is None):
            keep = getattr(self, "_reserved", False)
            self.reserve(need, lo=want_lo)
            self._reserved = keep
        return tuple(None if t is None else t[self._n:need] for t in (self._s32, self._s16, self._slo))

    def _source(self, x, chunk_bytes, np_dtype, keep):
        """What add() was given, normalised.  (host array, reader) when it is to be streamed: a `np_dtype` [n, d] array of more
        than chunk_bytes // 2 that is a numpy array, a pageable CPU tensor (of keep[0], np_dtype's torch name) or the payload
        of a blocks.BlockView (reader: its positioned reads from the file).  Otherwise (contiguous device tensor [n, d], None);
        dtypes outside `keep` become fp32."""
        import torch
        if self.d != self.d_in:
            x = self._pad_columns(x.array if hasattr(x, "array") else x)
        reader = None
        if hasattr(x, "read_rows_into") and hasattr(x, "array"):        # a blocks.BlockView
            reader, x = x.read_rows_into, x.array
        arr = x
        if isinstance(x, torch.Tensor) and x.device.type == "cpu" and not x.is_pinned() and x.dtype == keep[0]:
            arr = x.numpy()
        if isinstance(arr, np.ndarray) and arr.dtype == np_dtype and arr.ndim == 2 and arr.nbytes > chunk_bytes // 2:
            assert arr.shape[1] == self.d, "expected [n, %d], got %s" % (self.d, arr.shape)
            return arr, reader
        from_host = not (isinstance(x, torch.Tensor) and x.is_cuda)
        if isinstance(x, np.ndarray) and not x.flags.writeable:
            # a read-only array (the mmap of a small block file): torch.as_tensor would alias it without knowing it must
            # never write (a UserWarning today, undefined behaviour the day someone does) -- small by construction (large
            # host blocks are streamed), so it is copied first
            x = np.array(x, order="C")
        t = torch.as_tensor(x)
        if t.dtype not in keep:
            t = t.float()
        # (a host source that is not pinned -- e.g. the mmap of a small block file, which search_one_by_one closes right
        #  after add() returns -- is copied synchronously: nothing may still be reading it when add() is back)
        t = t.to(self.device, non_blocking=not from_host or t.is_pinned()).contiguous()
        assert t.dim() == 2 and t.shape[1] == self.d, "expected [n, %d], got %s" % (self.d, tuple(t.shape))
        return t, None

    def add(self, x, chunk_bytes=None, ids=None):
        """x: numpy / torch [n, d] float32 (host or device).  Appends to the index.
        A HOST array -- typically the memory-mapped payload of a block file (blocks.BlockView) -- is streamed: chunks of
        ~chunk_bytes (default 64 MB) go through pinned staging buffers, the H2D copy of chunk i + 1 (copy stream) runs under the
        centring / rounding / norm pass of chunk i (convdr_ip_prepare_block*), and the host fills one staging buffer
        (page faults on the mmap = the disk read) while the others are in flight.  The reference does pickle.load (a full
        host copy of the 14.6 GB block) and a pageable copy (run_convdr_inference.py:164-180).

        ids (FAISS ``add_with_ids``): an int64 vector [n], numpy or torch, host or device -- the rows' ids (``passage_embedding2id``,
        ``offset2pid``), kept in a device column beside the rows (``idx.ids``) and carried through keep_rows / remove_rows.  Ids
        need not be distinct: the chunk rows of one document share theirs.  Every add of an index carries ids or none does;
        a mixed add, a vector of another length or dtype, or the reserved id INT64_MIN raises ValueError and leaves the index
        as it was (ids on the device cost one host read for that check), and an add the index refuses leaves the column as it
        was, too."""
        if ids is None:
            if self._n and getattr(self, "_sid", None) is not None:
                raise ValueError("FlatIPIndex.add: this index carries row ids (%d rows), an add without ids= would leave rows "
                                 "without one; the index is unchanged" % self._n)
            return self._add_rows(x, chunk_bytes)
        if self._n and getattr(self, "_sid", None) is None:
            raise ValueError("FlatIPIndex.add: this index holds %d rows without ids, ids= cannot start now; the index is unchanged"
                             % self._n)
        rows = x.array if hasattr(x, "array") else x
        m = int(rows.shape[0]) if hasattr(rows, "shape") else len(rows)
        self._add_keyed(x, chunk_bytes, self._id_list("add", ids, length=m))

    def _add_keyed(self, x, chunk_bytes, t):
        """the rows `x` and their checked ids `t` (device int64, one per row) behind the resident rows and the column"""
        n0, m = self._n, int(t.numel())
        self._add_rows(x, chunk_bytes)                  # (raises: nothing below has touched the column)
        if m:
            self._reserve_ids(max(n0 + m, 0 if self._s16 is None else self._s16.shape[0]), keep=n0)
            self._sid[n0:n0 + m].copy_(t)

    def _id_list(self, who, ids, length=None):
        """ids of a caller -> device int64 vector, contiguous.  ValueError: not an int64 vector, not `length` entries, or the
        reserved id INT64_MIN (looked for here only where that costs no more than it does for add: `length` given, or the
        ids are on the host; the kernels flag it for the others)."""
        import torch
        if isinstance(ids, np.ndarray) and not ids.flags.writeable:
            ids = np.array(ids)                     # (a read-only array -- a memory-mapped id table: as in _source)
        t = torch.as_tensor(ids)
        if t.dtype != torch.int64 or t.dim() != 1:
            raise ValueError("%s: ids must be an int64 vector (got %s, shape %s)" % (who, t.dtype, tuple(t.shape)))
        if length is not None and int(t.numel()) != length:
            raise ValueError("%s: %d ids for %d rows" % (who, int(t.numel()), length))
        if (length is not None or t.device.type == "cpu") and t.numel() and bool((t == RESERVED_ID).any()):
            raise ValueError("%s: the id %d (INT64_MIN) is reserved" % (who, RESERVED_ID))
        return t.to(self.device).contiguous()

    def _add_rows(self, x, chunk_bytes=None):
        """add() without the id column"""
        import time
        import torch
        chunk_bytes = int(chunk_bytes or self.host_chunk_bytes)
        if self._half:
            return self._add_half(x, chunk_bytes)
        t, reader = self._source(x, chunk_bytes, np.float32, (torch.float32,))
        m = int(t.shape[0])
        if m == 0:
            return
        want_lo = self.precision in ("bf16x3", "fp16x3") or self._slo is not None
        with torch.cuda.device(self.device):
            if isinstance(t, np.ndarray):
                t0 = time.perf_counter()
                p32, p16, plo = self._grow_for(m, want_lo)
                first = self._n == 0

                def prepare(ci, s, e):
                    if first and ci == 0:
                        # centre = column mean of the first chunk (>= 40 k passages): any centre keeps the search exact -- it
                        # shifts every score of a query by the same constant -- it only has to be close to the mean to shrink
                        # the rounding-error band; likewise the fp16 scale comes from the first chunk's norms
                        self._first_rows(p32[s:e])
                    self._prepare_into(p32[s:e], p16[s:e], plo[s:e] if plo is not None else None)
                self._stream_rows(t, p32, reader, chunk_bytes, prepare, t0)
            else:
                if self._n == 0:
                    self._first_rows(t)
                if self._s32 is None and not want_lo:
                    # first block of an unreserved index: adopt the caller's device tensor instead of copying it
                    self._s32 = t
                    self._s16 = torch.empty((m, self.d), dtype=self._half_dtype, device=self.device)
                    dst32, dst16, dstlo = self._s32, self._s16, None
                else:
                    dst32, dst16, dstlo = self._grow_for(m, want_lo)
                    dst32.copy_(t)
                self._prepare_into(dst32, dst16, dstlo)
        self._n += m

    # -- the half store (storage="fp16") ----------------------------------------
    def _store_rows(self, src, dst, scale, fold_norm=True, flags=None):
        """convdr_ip_store_rows_f16: dst = half(src) * scale (dst None: norms and the non-finite flag only)"""
        import torch
        _lib.check(_lib.lib().convdr_ip_store_rows_f16(_lib.ptr(src), int(src.dtype == torch.float32), src.shape[0], self.d,
                                                       float(scale), _lib.ptr(dst), _lib.ptr(self._max_norm) if fold_norm else None,
                                                       _lib.ptr(self._flags if flags is None else flags), _lib.stream_ptr()),
                   "convdr_ip_store_rows_f16")

    def update_flags(self):
        """Flag word of the update_rows calls so far (one host read): bit 0 = a new row held a value that is not finite as
        a half, bit 1 = a scaled value overflowed (the rows outgrew the scale by more than CONVDR_IP_RANGE catches)."""
        return int(self._uflags.item())

    def _half_first_scale(self, src):
        """An empty half store takes its scale from the first rows' largest norm (one pass, one host read), never below 1."""
        self._store_rows(src, None, 1.0)
        self._scale = max(1.0, float(_lib.lib().convdr_ip_f16_scale(float(self._max_norm.item()))))

    def _add_half(self, x, chunk_bytes):
        """add() of a half store.  `write(dst)` below puts the new rows into dst = store[n, n + m) (rounded, scaled, norms
        and flags folded); the flag word and the max norm are read ONCE, at the end, and decide: keep, refuse (the index is
        left exactly as it was), or -- a scaled value overflowed: the new rows are too long for the scale -- lower the scale,
        rescale the resident rows in place and write the new rows once more (the only case with a second read)."""
        import torch
        t, reader = self._source(x, chunk_bytes, np.float16, (torch.float16, torch.float32))
        m = int(t.shape[0])

        def write(dst, first):
            if not isinstance(t, np.ndarray):
                if first:
                    self._half_first_scale(t)
                return self._store_rows(t, dst, self._scale)

            def scale_in_place(ci, s, e):       # the copy stream wrote the halves straight into the store
                if first and ci == 0:
                    self._half_first_scale(dst[s:e])
                self._store_rows(dst[s:e], dst[s:e], self._scale)
            self._stream_rows(t, dst, reader, chunk_bytes, scale_in_place)
        if m == 0:
            return
        n0, scale0 = self._n, self._scale
        with torch.cuda.device(self.device):
            mn0 = self._max_norm.clone()
            dst = self._grow_for(m)[1]
            for attempt in (0, 1):
                write(dst, n0 == 0 and attempt == 0)
                got = self._mf[:2].cpu()                                    # the one host read of this add()
                mn, fl = float(got[0]), int(got.view(torch.int32)[1])
                self._flags.zero_()
                if (fl & 1) or not mn <= HALF_NORM_LIMIT:
                    self._scale = scale0
                    self._max_norm.copy_(mn0)
                    raise _lib.ConvdrError("FlatIPIndex(storage='fp16').add: %s; the index is unchanged (%d rows)"
                                           % ("a value is not finite as a half" if fl & 1 else
                                              "a row's norm %g exceeds %g" % (mn, HALF_NORM_LIMIT), n0))
                if not (fl & 2):
                    break
                if attempt:
                    raise _lib.ConvdrError("half store: scaled values overflow at scale %g, max norm %g" % (self._scale, mn))
                self._rebuild_scaled()          # the scale that fits the new max norm; rows [0, n0) rescaled in place
            self._n = n0 + m

    def _stream_rows(self, arr, dst, reader, chunk_bytes, each, t0=None):
        """Host rows `arr` -> device rows `dst` (same shape and element type) through the pinned staging buffers -- viewed as
        dst's element type, so a buffer holds twice the rows of halves -- with the H2D copies on the copy stream; each(ci, s, e)
        is called on the main stream's side once chunk ci = rows [s, e) is ordered before it (its copy enqueued and waited
        for by the main stream).  reader: a BlockView's positioned reads instead of slices of `arr`.  t0: when the add()
        began to enqueue, for `stats["add_host_s"]` (default: now)."""
        import time
        import torch
        n, d = arr.shape
        t0 = time.perf_counter() if t0 is None else t0
        per32 = max(1, int(chunk_bytes) // (4 * d))     # the pinned bytes per buffer, as fp32 rows
        rows_per = per32 * 4 // dst.element_size()
        nbuf = max(2, int(self.host_stage_buffers))
        main = torch.cuda.current_stream()
        if getattr(self, "_copy_stream", None) is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        stage, freed = _staging(self.device, min(per32, (n * dst.element_size() + 3) // 4), d, nbuf)
        stage = [b.view(dst.dtype).view(-1, d) for b in stage]
        cs = self._copy_stream
        cs.wait_stream(main)                    # (allocation order / the copy of the old rows in _grow_for)
        avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        threads = max(1, min(int(self.host_copy_threads), avail))
        pool = _copy_pool(threads * (nbuf - 1), self.device)
        chunks = [(s, min(n, s + rows_per)) for s in range(0, n, rows_per)]

        def fill(ci):
            """start filling staging buffer ci % nbuf with chunk ci: `threads` positioned reads / memcpy slices"""
            s, e = chunks[ci]
            bi = ci % nbuf
            # staging buffer bi may be refilled once its previous H2D copy has completed.  The events live with the
            # buffers (module-level, shared by every index of the process): the last copies of one add() are still in
            # flight when the next add() starts filling (1 run in ~500 put rows of a second block into the first
            # before they did, tests/test_ip_search_gpu.py::test_back_to_back_streamed_adds_keep_their_rows)
            if freed[bi] is not None:
                freed[bi].synchronize()
            buf = stage[bi].numpy()[:e - s]
            if reader is not None:
                return reader(buf, s, e, pool=pool, parts=threads, wait=False)
            step = (e - s + threads - 1) // threads
            return [pool.submit(np.copyto, buf[a:a + step], arr[s + a:min(e, s + a + step)]) for a in range(0, e - s, step)]
        inflight = {ci: fill(ci) for ci in range(min(nbuf - 1, len(chunks)))}
        for ci, (s, e) in enumerate(chunks):
            for f in inflight.pop(ci):
                f.result()
            bi = ci % nbuf
            with torch.cuda.stream(cs):
                dst[s:e].copy_(stage[bi][:e - s], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(cs)
            freed[bi] = ev
            main.wait_event(ev)
            if ci + nbuf - 1 < len(chunks):
                # nbuf - 1 chunks are being read while this one crosses PCIe (the copy stream never waits for the host;
                # with two buffers -- round 2 -- the reads of chunk i + 1 only started after chunk i had been enqueued)
                inflight[ci + nbuf - 1] = fill(ci + nbuf - 1)
            each(ci, s, e)
        self.stats["add_host_s"] = time.perf_counter() - t0     # host time to enqueue (the last chunks are still in flight)
        self.stats["add_host_bytes"] = n * d * dst.element_size()

    def _pad_columns(self, x):
        import torch
        t = torch.as_tensor(x)
        t = (t if t.dtype == torch.float32 else t.float()).to(self.device)
        assert t.dim() == 2 and t.shape[1] == self.d_in, "expected [n, %d], got %s" % (self.d_in, tuple(t.shape))
        return torch.nn.functional.pad(t, (0, self.d - self.d_in))

    def _set_centre(self, t):
        import torch
        self._centre = torch.empty(self.d, dtype=torch.float32, device=self.device)
        scratch = torch.empty(1024 * self.d, dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().convdr_ip_column_mean(_lib.ptr(t), t.shape[0], self.d, _lib.ptr(scratch),
                                                   _lib.ptr(self._centre), _lib.stream_ptr()), "convdr_ip_column_mean")

    def _ensure_lo(self):
        """Remainder copy for the split scan, built on first use."""
        import torch
        if not self._half and self._slo is None and self._s32 is not None:
            with torch.cuda.device(self.device):
                self._slo = torch.empty((self._s32.shape[0], self.d), dtype=self._half_dtype, device=self.device)
                if self._n:
                    self._prepare_into(self._p32, self._pbf, self._plo)

    def update_rows(self, row0, emb):
        """Overwrite rows [row0, row0 + len(emb)) of the resident block with freshly encoded embeddings
        (device fp32 [m, d]) and refresh their scan copy / the block's max norm.  No sync."""
        import torch
        m = int(emb.shape[0])
        assert emb.dtype == torch.float32 and emb.is_contiguous() and row0 + m <= self.ntotal
        if self._half:
            # the new rows are rounded to half and scaled; a row the store cannot hold is an error AFTER the write (the caller
            # owns the rows it overwrites), a scale the rows outgrow is CONVDR_IP_RANGE at the next search, as for add()
            src = emb if self.d == self.d_in else torch.nn.functional.pad(emb, (0, self.d - self.d_in))
            with torch.cuda.device(self.device):
                self._store_rows(src.contiguous(), self._pbf[row0:row0 + m], self._scale, flags=self._uflags)
            return
        dst32, dstbf = self._p32[row0:row0 + m], self._pbf[row0:row0 + m]
        dstlo = None if self._slo is None else self._plo[row0:row0 + m]
        dst32[:, :self.d_in].copy_(emb)      # (zero columns of a padded width stay zero)
        with torch.cuda.device(self.device):
            self._prepare_into(dst32, dstbf, dstlo)

    def row_filter(self, mask):
        """A RowFilter of this index from a bool / uint8 vector [ntotal] (numpy or torch, host or device; non-zero = allowed):
        packed on the index's device with torch ops, the allowed count read ONCE, here (one host round trip at build time, none
        per search).  Pass it as ``allowed=`` to search / search_tensors / search_begin / search_device / search_deep_device.
        Valid while ntotal stays what it was: update_rows keeps it, add and reset do not."""
        import torch
        m = torch.as_tensor(mask)
        if m.dim() != 1 or int(m.numel()) != self.ntotal:
            raise ValueError("row_filter: the mask must be a vector of ntotal = %d entries (got shape %s)"
                             % (self.ntotal, tuple(m.shape)))
        m = m.to(self.device) != 0
        return RowFilter(pack_row_mask(m), self.ntotal, int(m.sum().item()))

    def _filter(self, allowed):
        """allowed= of a search call -> None or a RowFilter that fits this index"""
        if allowed is None:
            return None
        if not isinstance(allowed, RowFilter):
            return self.row_filter(allowed)
        if allowed.n != self.ntotal or allowed.bits.device != self.device:
            raise ValueError("stale RowFilter: built for ntotal = %d on %s, the index holds %d rows on %s"
                             % (allowed.n, allowed.bits.device, self.ntotal, self.device))
        return allowed

    def _workspace(self, nbytes):
        import torch
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self._ws

    # -- removing rows (FAISS remove_ids) and reading rows back (reconstruct) -------------------------------------------
    def keep_rows(self, allowed):
        """Compact the index to the allowed rows, IN PLACE: `allowed` is a RowFilter of this index or a bool / uint8 mask
        [ntotal] (non-zero = keep; a stale filter raises ValueError, as in search).  Returns the number of rows removed.

        The kept rows move to the front of every resident buffer (fp32 block, scan copy, remainder copy; the half store: its
        one buffer) in their old order, bit for bit: row r becomes row #{kept rows before r}, so ``search`` afterwards equals
        ``search(..., allowed=keep)`` before, with the ids renumbered by ``cumsum(keep) - 1``.  No buffer is copied: the device
        works through windows of ``compact_window_rows`` rows (convdr_ip_compact_*, include/convdr_hip.h "Removing rows") and
        the extra memory is one window of the widest buffer.  ntotal becomes the filter's ``n_allowed``, which is already on
        the host: nothing is read back, the whole removal is enqueued.

        What stays: the centre and the scale (any centre keeps the search exact, and the scale still fits); ``_max_norm``,
        which remains an UPPER bound of the kept rows' norms -- all the certificate needs, so it is not recomputed; a
        reservation and the backing storage, which is not shrunk: the next ``add`` fills rows [ntotal, ...).
        The id column of an index that carries ids (add(ids=)) is compacted with the same bitmap and plan: ``idx.ids`` stays in
        step, nothing is cut by hand.
        What the caller does: filters built for the old ntotal are stale (unless nothing was removed); side tables the index
        does not hold (the keys of search_distinct) are cut with the same mask, ``keys[keep]``; a first block adopted from
        the caller's device tensor is modified in place, as by update_rows; a search_begin handle is finished first.
        ``stats``: removed, compact_windows (windows per buffer)."""
        f = self._filter(allowed)
        if f is None:
            raise ValueError("keep_rows: a RowFilter or a mask of ntotal = %d entries is needed (got None)" % self.ntotal)
        n, w = self.ntotal, int(self.compact_window_rows)
        if w < ROW_FILTER_TILE or w % ROW_FILTER_TILE:
            raise ValueError("keep_rows: compact_window_rows must be a positive multiple of %d (got %d)" % (ROW_FILTER_TILE, w))
        removed = n - f.n_allowed
        self.stats = {"removed": removed, "compact_windows": 0}
        if removed:
            self._compact(f, w)
            self._n = f.n_allowed
            self.stats["compact_windows"] = (n + w - 1) // w
        return removed

    def remove_rows(self, rows):
        """FAISS ``remove_ids``: `rows` is an int64 id vector (numpy or torch, host or device; duplicates allowed) or a bool /
        uint8 mask [ntotal] (non-zero = remove).  An id outside [0, ntotal) raises ValueError and leaves the index as it was.
        The keep mask is built on the device and handed to ``keep_rows`` (one host read: the kept count and the range check
        together).  Returns the number of rows removed."""
        import torch
        n = self.ntotal
        t = torch.as_tensor(rows)
        if t.dtype in (torch.bool, torch.uint8):
            if t.dim() != 1 or int(t.numel()) != n:
                raise ValueError("remove_rows: the mask must be a vector of ntotal = %d entries (got shape %s)" % (n, tuple(t.shape)))
            return self.keep_rows(t.to(self.device) == 0)
        if t.is_floating_point() or t.is_complex() or t.dim() != 1:
            raise ValueError("remove_rows: rows must be an integer id vector or a bool / uint8 mask (got %s, shape %s)"
                             % (t.dtype, tuple(t.shape)))
        if not t.numel():
            self.stats = {"removed": 0, "compact_windows": 0}
            return 0
        if t.device.type == "cpu" and (int(t.min()) < 0 or int(t.max()) >= n):
            raise ValueError("remove_rows: row ids %d..%d outside [0, ntotal = %d)" % (int(t.min()), int(t.max()), n))
        if n == 0:
            raise ValueError("remove_rows: the index is empty, no id is inside [0, ntotal = 0)")
        t = t.to(torch.int64).to(self.device)
        keep = torch.ones(n, dtype=torch.bool, device=self.device)
        keep[t.clamp(0, n - 1)] = False                    # (a scratch mask: the index is untouched until the ids are known good)
        counts = torch.stack([keep.sum(), ((t < 0) | (t >= n)).sum()]).cpu()
        if int(counts[1]):
            raise ValueError("remove_rows: %d row ids outside [0, ntotal = %d)" % (int(counts[1]), n))
        return self.keep_rows(RowFilter(pack_row_mask(keep), n, int(counts[0])))

    def _compact(self, f, window_rows):
        """convdr_ip_compact_plan once, convdr_ip_compact_rows per resident buffer; no host read.  The plan's device scalar
        stays in ``_n_kept`` (int64 [1])."""
        import torch
        L, ptr = _lib.lib(), _lib.ptr
        n = self.ntotal
        # (a block shorter than the window is one window either way: the bounce buffer need not be larger than the block)
        window_rows = min(int(window_rows), (n + ROW_FILTER_TILE - 1) // ROW_FILTER_TILE * ROW_FILTER_TILE)
        bufs = [t for t in (self._s32, self._s16, self._slo) if t is not None]
        widest = max(int(t.shape[1]) * t.element_size() for t in bufs)
        need = L.convdr_ip_compact_workspace_bytes(n, widest, window_rows)
        if not need:
            raise _lib.ConvdrError("convdr_ip_compact_rows: sizes outside the contract: %s" % L.convdr_last_error().decode())
        ws = self._workspace(need)
        words = int(f.bits.numel())
        with torch.cuda.device(self.device):
            self._n_kept = torch.empty(1, dtype=torch.int64, device=self.device)
            _lib.check(L.convdr_ip_compact_plan(ptr(f.bits), words, n, ptr(ws), ws.numel(), ptr(self._n_kept), _lib.stream_ptr()),
                       "convdr_ip_compact_plan")
            for t in bufs:
                _lib.check(L.convdr_ip_compact_rows(ptr(t), int(t.shape[1]) * t.element_size(), n, ptr(f.bits), words, window_rows,
                                                    ptr(ws), ws.numel(), _lib.stream_ptr()), "convdr_ip_compact_rows")
            if getattr(self, "_sid", None) is not None:
                # the id column: 8-byte rows, out of place into its partner by the same plan; the two then change roles
                if self._sid_spare is None or self._sid_spare.shape[0] != self._sid.shape[0]:
                    self._sid_spare = torch.empty_like(self._sid)
                _lib.check(L.convdr_ip_compact_ids(ptr(self._sid), ptr(self._sid_spare), n, ptr(f.bits), words, ptr(ws), ws.numel(),
                                                   _lib.stream_ptr()), "convdr_ip_compact_ids")
                self._sid, self._sid_spare = self._sid_spare, self._sid

    # -- row ids (FAISS IndexIDMap2): the column add(ids=) fills, and the operations that speak in ids ---------------------
    # No key -> row table is kept: every call builds a hash set of ITS list on the device (convdr_keyset_build) and all rows
    # probe it in one pass over the column (convdr_keys_member / convdr_keys_locate; include/convdr_hip.h "Row ids").
    @property
    def ids(self):
        """The rows' ids: device int64 [ntotal], a view of the column; None for an index that never got ids."""
        sid = getattr(self, "_sid", None)
        return None if sid is None else sid[:self._n]

    def _need_ids(self, who):
        if self.ids is None:
            raise ValueError("%s: this index carries no row ids (give them to add: add(x, ids=...))" % who)

    def _keyset(self, who, t, need=None):
        """convdr_keyset_build of the device int64 list `t` -> (workspace, status int32 [1]); enqueued, no host read.
        need: bytes of a workspace that keeps more behind the set (0: sizes outside that entry's contract)"""
        import torch
        L, ptr = _lib.lib(), _lib.ptr
        m = int(t.numel())
        need = int(L.convdr_keyset_workspace_bytes(m)) if need is None else need
        if not need:
            raise ValueError("%s: %s" % (who, L.convdr_last_error().decode()))
        ws = getattr(self, "_key_ws", None)
        if ws is None or ws.numel() < need:
            self._key_ws = ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        status = torch.empty(1, dtype=torch.int32, device=self.device)
        _lib.check(L.convdr_keyset_build(ptr(t), m, ptr(ws), ws.numel(), ptr(status), _lib.stream_ptr()), "convdr_keyset_build")
        return ws, status

    @staticmethod
    def _key_codes(ws, status):
        """the two status words (the build's, the row pass's) as device int64 [2], to ride along with the caller's host read"""
        import torch
        return torch.cat([status, ws[:4].view(torch.int32)]).to(torch.int64)

    @staticmethod
    def _key_status(who, code):
        if code & (KEY_ST_LIST | KEY_ST_COLUMN):
            raise ValueError("%s: the id %d (INT64_MIN) is reserved; %s holds it" %
                             (who, RESERVED_ID, "the list" if code & KEY_ST_LIST else "the index's id column"))
        if code:
            raise _lib.ConvdrError("%s: the key set reported status %d (2: a probe hit its bound, 8: no set in the workspace)" % (who, code))

    def _member(self, who, ids, invert):
        """(bitmap of the rows whose id is / is not in `ids`, bits set, distinct listed ids on no row): ONE host read"""
        import torch
        self._need_ids(who)
        t = self._id_list(who, ids)
        L, ptr = _lib.lib(), _lib.ptr
        n = self.ntotal
        words = (n + ROW_FILTER_TILE - 1) // ROW_FILTER_TILE * 8
        with torch.cuda.device(self.device):
            ws, status = self._keyset(who, t)
            bits = torch.empty(words, dtype=torch.int32, device=self.device)
            counts = torch.empty(2, dtype=torch.int64, device=self.device)
            _lib.check(L.convdr_keys_member(ptr(self.ids), n, ptr(ws), ws.numel(), int(bool(invert)), ptr(bits), words, ptr(counts),
                                            _lib.stream_ptr()), "convdr_keys_member")
            got = [int(v) for v in torch.cat([counts, self._key_codes(ws, status)]).cpu()]
        self._key_status(who, got[2] | got[3])
        return bits, got[0], got[1]

    def remove_ids(self, ids):
        """FAISS ``IndexIDMap2.remove_ids``: every row whose id is in `ids` (int64 vector, numpy or torch, host or device;
        repeats allowed) goes -- all chunk rows of a repeated id included --, ids that are on no row are ignored.  Returns the
        number of rows removed.  The keep bitmap is built on the device and handed to ``keep_rows``, which compacts the rows
        and the id column; one host read (the kept count, the missing count and the status words together).
        ``stats``: removed, compact_windows, ids_missing (distinct listed ids found on no row)."""
        n = self.ntotal
        bits, kept, missing = self._member("remove_ids", ids, True)
        removed = self.keep_rows(RowFilter(bits, n, kept))
        self.stats["ids_missing"] = missing
        return removed

    def id_filter(self, ids, invert=False):
        """A RowFilter of the rows whose id is in `ids` (invert: is NOT in it) -- a sub-collection, the judged pool of a topic
        set -- for ``allowed=`` of the searches and for keep_rows.  Built on the device straight into the bitmap layout of
        pack_row_mask; one host read (the allowed count), as for row_filter, and the same staleness rule: valid while ntotal
        stays what it was."""
        bits, n_allowed, _ = self._member("id_filter", ids, invert)
        return RowFilter(bits, self.ntotal, n_allowed)

    def _locate(self, who, ids, want_dup=False):
        import torch
        self._need_ids(who)
        t = self._id_list(who, ids)
        L, ptr = _lib.lib(), _lib.ptr
        m = int(t.numel())
        with torch.cuda.device(self.device):
            ws, status = self._keyset(who, t)
            first = torch.empty(m, dtype=torch.int64, device=self.device)
            count = torch.empty(m, dtype=torch.int32, device=self.device)
            dup = torch.empty(m, dtype=torch.int32, device=self.device) if want_dup else None
            _lib.check(L.convdr_keys_locate(ptr(self.ids), self.ntotal, ptr(ws), ws.numel(), ptr(t), m, ptr(first), ptr(count), ptr(dup),
                                            _lib.stream_ptr()), "convdr_keys_locate")
        return t, first, count, dup, ws, status

    def rows_of(self, ids):
        """Where the ids are: device (first_row int64 [m], count int32 [m]) -- the smallest row holding ids[j] or -1, and the
        number of rows holding it.  Enqueued, no sync (so a reserved id in a device list is not an error here: it is on no
        row, -1 and 0)."""
        _, first, count, _, _, _ = self._locate("rows_of", ids)
        return first, count

    def reconstruct_ids(self, ids):
        """FAISS ``IndexIDMap2.reconstruct`` for a list: float32 numpy [m, d_in], the first row of every id (rows_tensors of
        rows_of).  An id that is on no row raises IndexError."""
        first, _ = self.rows_of(ids)
        if first.numel():
            absent = int((first < 0).sum().item())
            if absent:
                raise IndexError("reconstruct_ids: %d of the %d ids are on no row" % (absent, int(first.numel())))
        return self.rows_tensors(first).cpu().numpy()

    def upsert(self, ids, emb):
        """Re-encoded passages: `emb` (device fp32 [m, d_in]) replaces the rows of `ids` (int64 [m]).  An id that is on exactly
        one row gets that row overwritten in place (the scan copies and the max norm refreshed as by update_rows; the half
        store's update_flags() rule applies); an id on no row is appended, in list order, with its id.  Returns
        (n_updated, n_added).  A list that repeats an id, or an id that sits on more than one row (chunk rows: which one?),
        raises ValueError BEFORE anything is written -- one host read, the one that also splits the list."""
        import torch
        t, first, count, dup, ws, status = self._locate("upsert", ids, want_dup=True)
        m = int(t.numel())
        if not (isinstance(emb, torch.Tensor) and emb.dtype == torch.float32 and emb.device == self.device
                and tuple(emb.shape) == (m, self.d_in)):
            raise ValueError("upsert: emb must be a float32 tensor [%d, %d] on %s" % (m, self.d_in, self.device))
        got = torch.cat([first, count.to(torch.int64), dup.to(torch.int64), self._key_codes(ws, status)]).cpu().numpy()
        self._key_status("upsert", int(got[3 * m] | got[3 * m + 1]))
        fr, cnt, dp = got[:m], got[m:2 * m], got[2 * m:3 * m]
        rep = np.nonzero(dp != np.arange(m))[0]
        if rep.size:
            raise ValueError("upsert: the list repeats an id (position %d repeats position %d); nothing was written"
                             % (int(rep[0]), int(dp[rep[0]])))
        many = np.nonzero(cnt > 1)[0]
        if many.size:
            raise ValueError("upsert: the id at position %d sits on %d rows; nothing was written" % (int(many[0]), int(cnt[many[0]])))
        upd, new = np.nonzero(cnt == 1)[0], np.nonzero(cnt == 0)[0]
        emb = emb.contiguous()
        with torch.cuda.device(self.device):
            if upd.size:
                sel = torch.as_tensor(upd, device=self.device)
                self._overwrite_rows(torch.as_tensor(fr[upd], device=self.device), emb if upd.size == m else emb[sel])
            if new.size:
                sel = torch.as_tensor(new, device=self.device)
                self.add(emb[sel], ids=t[sel])
        return int(upd.size), int(new.size)

    def _overwrite_rows(self, rows, emb):
        """update_rows for scattered rows: the scan copies of `emb` are made by the same pass on a contiguous temporary (norms
        folded into the max norm, the half store's flags into the update word), then every resident buffer takes its rows."""
        import torch
        m = int(emb.shape[0])
        src = (emb if self.d == self.d_in else torch.nn.functional.pad(emb, (0, self.d - self.d_in))).contiguous()
        t16 = torch.empty((m, self.d), dtype=self._half_dtype, device=self.device)
        if self._half:
            self._store_rows(src, t16, self._scale, flags=self._uflags)
            self._s16.index_copy_(0, rows, t16)
            return
        tlo = None if self._slo is None else torch.empty_like(t16)
        self._prepare_into(src, t16, tlo)
        self._s32.index_copy_(0, rows, src)
        self._s16.index_copy_(0, rows, t16)
        if tlo is not None:
            self._slo.index_copy_(0, rows, tlo)

    # -- documents by id: a document is EVERY row that carries one id (the chunk rows of a MaxP block share theirs) ----------
    # Two device primitives (include/convdr_hip.h, "Documents by id"): all rows of the listed ids as a CSR
    # (convdr_keys_rows_count / convdr_keys_rows_fill) and the MaxP score of (query, document) pairs (convdr_ip_score_docs).
    def _rows_csr(self, who, t, reserved_ok=False, host=False):
        """The CSR of the device id list `t` (int64 [m]): (start int64 [m], count int32 [m], rows int64 [total], host) --
        convdr_keyset_build, convdr_keys_rows_count, ONE host read (total and the status words; with `host` also start, count
        and dup_of, returned as numpy int64 [3, m]), convdr_keys_rows_fill into a list of exactly `total` entries.
        reserved_ok: INT64_MIN in the list is padding (on no row), not an error."""
        import torch
        L, ptr = _lib.lib(), _lib.ptr
        m, n = int(t.numel()), self.ntotal
        need0 = int(L.convdr_keys_rows_workspace_bytes(m, 0))
        with torch.cuda.device(self.device):
            ws, status = self._keyset(who, t, need0)
            start = torch.empty(m, dtype=torch.int64, device=self.device)
            count = torch.empty(m, dtype=torch.int32, device=self.device)
            dup = torch.empty(m, dtype=torch.int32, device=self.device) if host else None
            total = torch.empty(1, dtype=torch.int64, device=self.device)
            _lib.check(L.convdr_keys_rows_count(ptr(self.ids), n, ptr(ws), ws.numel(), ptr(t), m, ptr(start), ptr(count), ptr(dup),
                                                ptr(total), _lib.stream_ptr()), "convdr_keys_rows_count")
            parts = [total, self._key_codes(ws, status)]
            if host:
                parts += [start, count.to(torch.int64), dup.to(torch.int64)]
            got = torch.cat(parts).cpu().numpy()
            code = int(got[1] | got[2])
            self._key_status(who, code & ~KEY_ST_LIST if reserved_ok else code)
            tot = int(got[0])
            need = int(L.convdr_keys_rows_workspace_bytes(m, tot))
            if ws.numel() < need:
                # the two lists of the fill lie behind what the count wrote: a larger buffer takes that part over
                grown = torch.empty(need, dtype=torch.uint8, device=self.device)
                grown[:need0].copy_(ws[:need0])
                self._key_ws = ws = grown
            rows = torch.empty(tot, dtype=torch.int64, device=self.device)
            _lib.check(L.convdr_keys_rows_fill(ptr(self.ids), n, ptr(ws), ws.numel(), m, ptr(rows), tot, _lib.stream_ptr()),
                       "convdr_keys_rows_fill")
        return start, count, rows, (got[3:].reshape(3, m) if host else None)

    def rows_all(self, ids):
        """ALL rows of the listed ids (int64 vector, numpy or torch, host or device; repeats allowed): device (start int64 [m],
        count int32 [m], rows int64 [total]).  The rows that carry ids[j] are rows[start[j] : start[j] + count[j]], ascending;
        an id on no row has count 0; a repeated id shares the segment of its first occurrence, so total = the rows of the
        DISTINCT listed ids.  The same bits in every run.  One host read (total, to size `rows`, and the status words; a
        device list that holds the reserved id INT64_MIN raises ValueError there, as for remove_ids)."""
        self._need_ids("rows_all")
        start, count, rows, _ = self._rows_csr("rows_all", self._id_list("rows_all", ids))
        return start, count, rows

    def _ids_arg(self, who, q, ids):
        """(queries as a tensor, ids as a tensor, the shape of `ids`) of a (queries, document ids) call; the checks that need
        no device"""
        import torch
        if isinstance(ids, np.ndarray) and not ids.flags.writeable:
            ids = np.array(ids)
        qt, it = torch.as_tensor(q), torch.as_tensor(ids)
        if qt.dim() != 2 or qt.shape[1] not in (self.d, self.d_in):
            raise ValueError("%s: queries must be [nq, %d] (got shape %s)" % (who, self.d_in, tuple(qt.shape)))
        nq = int(qt.shape[0])
        if it.dtype != torch.int64 or it.dim() not in (1, 2) or int(it.shape[0]) != nq:
            raise ValueError("%s: ids must be int64 [nq] or [nq, m] with nq = %d (got %s, shape %s)"
                             % (who, nq, it.dtype, tuple(it.shape)))
        return qt, it, tuple(it.shape)

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

    def doc_ordinals(self):
        """The DocOrdinals of this index: every row's dense document number (convdr_doc_ordinals; include/convdr_hip.h,
        "Document rank"), 0 .. ndocs - 1 in the order of the documents' first rows -- what numpy gives as
        ``argsort(argsort(first))[inv]`` of ``np.unique(ids, return_index=True, return_inverse=True)``, the same bits in every
        run.  Query independent: one pass over the id column, ONE host read (ndocs together with the status words).  Valid while
        the column stays as it was; ntotal is what is checked (a stale one raises ValueError in rank_ids).  As for a RowFilter,
        ``upsert_docs`` of documents whose chunk count changed moves rows without changing ntotal: rebuild after it."""
        import torch
        self._need_ids("doc_ordinals")
        L, ptr = _lib.lib(), _lib.ptr
        n = self.ntotal
        need = int(L.convdr_doc_ordinals_workspace_bytes(n))
        if not need:
            raise ValueError("doc_ordinals: %s" % L.convdr_last_error().decode())
        with torch.cuda.device(self.device):
            ws = getattr(self, "_key_ws", None)
            if ws is None or ws.numel() < need:
                self._key_ws = ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            ord_ = torch.empty(n, dtype=torch.int32, device=self.device)
            nd = torch.empty(1, dtype=torch.int64, device=self.device)
            _lib.check(L.convdr_doc_ordinals(ptr(self.ids), n, ptr(ws), ws.numel(), ptr(ord_), ptr(nd), _lib.stream_ptr()),
                       "convdr_doc_ordinals")
            got = [int(v) for v in torch.cat([nd, ws[:4].view(torch.int32).to(torch.int64)]).cpu()]     # the one host read
        self._key_status("doc_ordinals", got[1])
        return DocOrdinals(ord_, got[0], n)

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
        ``search``; a filter may drop some chunk rows of a document (its best ALLOWED row then stands for it) or all of them."""
        self._need_ids("search_docs")
        D, I, K, counts = self._search_distinct(q, k, self.ids, depth, strict, max_depth, allowed)
        return D, K, I, counts

    def reconstruct_docs(self, ids):
        """All chunk rows of the listed documents: numpy (start int64 [m], count int32 [m], emb float32 [total, d_in]) --
        ``rows_all`` followed by ``rows_tensors``; the rows of ids[j] are emb[start[j] : start[j] + count[j]], in ascending row
        order.  An id on no row has count 0 (``reconstruct_ids`` raises for it)."""
        start, count, rows = self.rows_all(ids)
        return start.cpu().numpy(), count.cpu().numpy(), self.rows_tensors(rows).cpu().numpy()

    def upsert_docs(self, ids, counts, emb):
        """Re-encoded documents: document ids[j] (int64 [m]) now has counts[j] >= 1 chunk rows (host integers [m]), given in
        list order in `emb` (device fp32 [sum(counts), d_in]).
          * a document on no row is appended with its id repeated;
          * a document that sits on counts[j] rows has them overwritten in place, in ascending row order (``_overwrite_rows``:
            the scan copies and the max norm refreshed, the half store's update_flags() rule applies);
          * a document on another number of rows has ALL its old rows removed -- one ``keep_rows`` for all such documents --
            and its new rows appended, in list order among the appended documents.
        Returns (n_in_place, n_replaced, n_added) in documents.  A list that repeats an id, or counts / emb of another shape,
        dtype or device, raises ValueError BEFORE anything is written; one host read (total, status, and what splits the list).
        Consequences: replaced documents move to the END of the index; and whenever a document was replaced, rows were
        removed and others added, so a RowFilter built before the call must not be reused even where ntotal happens to come
        out equal -- the staleness check compares ntotal only.  Side tables in row order are cut as for keep_rows."""
        import torch
        self._need_ids("upsert_docs")
        t = self._id_list("upsert_docs", ids)
        m = int(t.numel())
        if isinstance(counts, torch.Tensor):
            if counts.device.type != "cpu":
                raise ValueError("upsert_docs: counts must be host integers (got a tensor on %s)" % (counts.device,))
            counts = counts.numpy()
        cn = np.asarray(counts)
        if cn.ndim != 1 or cn.shape[0] != m or cn.dtype.kind not in "iu" or (m and int(cn.min()) < 1):
            raise ValueError("upsert_docs: counts must be an integer vector [%d] with every entry >= 1 (got %s, shape %s)"
                             % (m, cn.dtype, tuple(cn.shape)))
        cn = cn.astype(np.int64)
        if not (isinstance(emb, torch.Tensor) and emb.dtype == torch.float32 and emb.device == self.device
                and tuple(emb.shape) == (int(cn.sum()), self.d_in)):
            raise ValueError("upsert_docs: emb must be a float32 tensor [%d, %d] on %s" % (int(cn.sum()), self.d_in, self.device))
        if not m:
            return 0, 0, 0
        _, _, rows, (st, cur, dp) = self._rows_csr("upsert_docs", t, host=True)
        rep = np.nonzero(dp != np.arange(m))[0]
        if rep.size:
            raise ValueError("upsert_docs: the list repeats an id (position %d repeats position %d); nothing was written"
                             % (int(rep[0]), int(dp[rep[0]])))

        def spans(first, length):
            """the concatenation of arange(first[j], first[j] + length[j]), on the device"""
            begin = np.cumsum(length) - length
            at = np.repeat(first, length) + (np.arange(int(length.sum()), dtype=np.int64) - np.repeat(begin, length))
            return torch.as_tensor(at, device=self.device)
        off = np.cumsum(cn) - cn                                   # first row of document j in emb
        same, new = cur == cn, cur == 0
        repl = ~same & ~new
        emb, n = emb.contiguous(), self.ntotal
        with torch.cuda.device(self.device):
            if same.any():
                self._overwrite_rows(rows[spans(st[same], cn[same])], emb if same.all() else emb[spans(off[same], cn[same])])
            if repl.any():
                keep = torch.ones(n, dtype=torch.bool, device=self.device)
                keep[rows[spans(st[repl], cur[repl])]] = False
                self.keep_rows(RowFilter(pack_row_mask(keep), n, n - int(cur[repl].sum())))
            if not same.all():
                app = ~same
                who = torch.as_tensor(np.repeat(np.nonzero(app)[0], cn[app]), device=self.device)
                self._add_keyed(emb[spans(off[app], cn[app])], None, t[who])       # (the list's ids are known clean)
        return int(same.sum()), int(repl.sum()), int(new.sum())

    def search_ids(self, q, k, allowed=None):
        """``search`` with ids for row numbers: numpy (D, ids [nq, k]); FAISS padding stays -1."""
        D, I = self.search_ids_tensors(q, k, allowed=allowed)
        return D.cpu().numpy(), I.cpu().numpy()

    def search_ids_tensors(self, q, k, allowed=None):
        """``search_tensors`` with I mapped through the id column on the device (-1 stays -1)."""
        import torch
        self._need_ids("search_ids")
        D, I = self.search_tensors(q, k, allowed=allowed)
        if not self.ntotal:
            return D, I
        return D, torch.where(I >= 0, self.ids[I.clamp(min=0)], torch.full_like(I, -1))

    def rows_tensors(self, ids):
        """The corpus rows `ids` (integers, any shape [..]) as a device fp32 tensor [.., d_in]: the fp32 store returns the fp32
        block's rows bit for bit, the half store its stored halves un-scaled and widened (exact); the zero columns of a
        padded width are cut off.  An id outside [0, ntotal) raises IndexError (ids in a device tensor cost one host read)."""
        import torch
        t = torch.as_tensor(ids)
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise IndexError("reconstruct: row ids must be integers (got %s)" % t.dtype)
        t = t.to(torch.int64)
        if t.numel():
            lo, hi = (int(v) for v in torch.stack([t.min(), t.max()]).cpu())
            if lo < 0 or hi >= self.ntotal:
                raise IndexError("reconstruct: row ids %d..%d outside [0, ntotal = %d)" % (lo, hi, self.ntotal))
        t = t.to(self.device)
        if self._rows is None:
            return torch.empty(tuple(t.shape) + (self.d_in,), dtype=torch.float32, device=self.device)
        r = self._rows[t.reshape(-1)][:, :self.d_in]
        if self._half:
            r = r.float() * (1.0 / float(self._scale))     # (a power of two: exact)
        return r.reshape(tuple(t.shape) + (self.d_in,)).contiguous()

    def reconstruct(self, i):
        """FAISS ``reconstruct``: row i as float32 numpy [d_in] (see rows_tensors)."""
        return self.rows_tensors(int(i)).cpu().numpy()

    def reconstruct_n(self, i0, ni):
        """FAISS ``reconstruct_n``: rows [i0, i0 + ni) as float32 numpy [ni, d_in]."""
        i0, ni = int(i0), int(ni)
        if ni < 0 or i0 < 0 or i0 + ni > self.ntotal:
            raise IndexError("reconstruct_n: rows [%d, %d) outside [0, ntotal = %d)" % (i0, i0 + ni, self.ntotal))
        return self.rows_tensors(np.arange(i0, i0 + ni, dtype=np.int64)).cpu().numpy()

    def reconstruct_batch(self, ids):
        """FAISS ``reconstruct_batch``: the rows `ids` (int64 vector) as float32 numpy [len(ids), d_in]."""
        return self.rows_tensors(ids).cpu().numpy()

    def _search_call(self, q, nq, p32, p16, plo, n, k, tau_in, cap, rank_target, ws, D, I, status, tau_retry, split=False,
                     deep=False, allowed=None):
        """One call of convdr_ip_search[_deep][_f16 | _h16]: the entry of this index's scan copy and of the depth; with a
        RowFilter, convdr_ip_search_filtered with the same operands."""
        ptr = _lib.ptr
        store, r32, r16, scale, _ = self._operands((p32, p16))
        rlo, split = None if self._half else ptr(plo), int(bool(split)) if self._half else 0
        if allowed is not None:
            _lib.check(_lib.lib().convdr_ip_search_filtered(
                store, int(bool(deep)), ptr(q), nq, r32, r16, rlo, scale, split, n, self.d, k, ptr(self._max_norm),
                ptr(tau_in), cap, rank_target, ptr(ws), ws.numel(), ptr(allowed.bits), allowed.bits.numel(), allowed.n_allowed,
                ptr(D), ptr(I), ptr(status), ptr(tau_retry), _lib.stream_ptr()), "convdr_ip_search_filtered")
            return
        # the direct entry of the store code, each with the operands it declares
        name, rows = (("", (r32, r16, rlo)), ("_f16", (r32, r16, rlo, scale)), ("_h16", (r16, scale, split)))[store]
        name = "convdr_ip_search" + ("_deep" if deep else "") + name
        _lib.check(getattr(_lib.lib(), name)(ptr(q), nq, *rows, n, self.d, k, ptr(self._max_norm), ptr(tau_in), cap, rank_target,
                                             ptr(ws), ws.numel(), ptr(D), ptr(I), ptr(status), ptr(tau_retry),
                                             _lib.stream_ptr()), name)

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
        while cap < 2 * k and cap < 8192:      # the candidate list holds at least 2k entries (csrc/ip_topk.hip: k <= cap / 2)
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
        allowed rows, I in the index's row numbers, padding where fewer than k rows are allowed."""
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
        x3 = self.precision in _SPLIT or (self.precision == "auto" and getattr(self, "_x3_first", False) and self.ntotal > 0)
        # 4096 < k <= 65536: the same pipeline with the lists in global memory (convdr_ip_search_deep*)
        depth, cap = (self._DEEP, self._deep_cap(k)) if k > self.MAX_K else (self._SHALLOW, self.cap)
        if (depth is self._DEEP and not self.ntotal) or (f is not None and f.n_allowed == 0):
            return _Pending(qt, k, depth, x3, cap, None, f)     # (the shallow kernels pad an empty index's result themselves)
        return _Pending(qt, k, depth, x3, cap, getattr(self, depth.enqueue)(qt, k, cap=cap, x3=x3, **kw), f)

    def search_finish(self, handle):
        """The ladder, at either depth: fp16 (or pinned) first pass -> rebuild on RANGE -> retries with tau_retry / a doubled
        list -> split scan -> whatever is still open takes the depth's last rung."""
        import torch
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
        if self.kind == "f16" and n_range:
            self._rebuild_scaled()
            self.stats["rescaled"] = 1
            D, I, status, tau_retry = enqueue(qt, k, cap=cap, x3=x3)
            n_bad = int((status != 0).sum().item())
        self.stats["retried"] = int(n_bad)
        second = self.precision == "auto" and not x3        # the split scan is still ahead
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
        """``search_distinct`` with a row filter (``search_docs``).  allowed: a RowFilter or a mask as for ``search``, packed
        once for all passes, or None.  With a filter the result is the walk over the ALLOWED rows, the filter's ``n_allowed``
        takes ntotal's place in the depth defaults, and a query is certified iff it found k keys, or the list ran out of rows,
        or m >= n_allowed.  None: search_distinct as it was."""
        import torch
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
        todo = None                                     # indices of the queries still open (None: all)
        self.distinct_stats = {"depths": [], "searched": []}
        while True:
            qs = qt if todo is None else qt[todo].contiguous()
            Dm, Im = self.search_tensors(qs, m, **kw)
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
            m = min(2 * m, limit)

    @property
    def _split_key(self):
        """stats key that counts the queries of the second rung: the three-pass split scan, or the half store's two passes"""
        return "x2_queries" if self._half else "x3_queries"

    MAX_K = 4096         # convdr_ip_search: k <= cap / 2, cap <= 8192
    DEEP_MAX_K = 65536   # convdr_ip_search_deep: k <= cap / 2, cap <= 131072
    DEEP_MIN_CAP, DEEP_MAX_CAP = 16384, 131072
    DEEP_WS_BYTES = 4 << 30      # most workspace one deep call may ask for; search_deep_device splits the queries to stay under it
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
        return self._range(q, radius, allowed, False)

    def range_count(self, q, radius, allowed=None):
        """int64 numpy [nq]: how many rows ``range_search`` would return per query, without ordering or packing them
        (1 + range_count(q, score of a known positive) is that positive's exact rank in the whole index)."""
        return self._range(q, radius, allowed, True)

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
                if self.kind != "f16" or self.stats["rescaled"]:
                    raise _lib.ConvdrError("%s: CONVDR_IP_RANGE %s" % (who, "after the scan copy was rebuilt"
                                           if self.stats["rescaled"] else "from a bf16 scan"))
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
            store, r32, r16, scale, _ = self._operands(None if n else (None, None))     # (an empty index passes no rows)
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().convdr_ip_score_rows(store, _lib.ptr(qt), nq, r32, r16, scale, n, self.d, _lib.ptr(rt), m, m,
                                                           _lib.ptr(X), _lib.ptr(D), _lib.stream_ptr()), "convdr_ip_score_rows")
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
        of its score, which are re-scored exactly.  The host loop reads ONE tensor per pass: the first pass runs at
        ``self.cap``; a pair whose band overflowed is re-run once at the smallest power of two that holds the reported band
        count, up to RANGE_MAX_CAP; CONVDR_IP_RANGE rebuilds the scan copy once (as search_finish).  A pair whose band holds
        more than RANGE_MAX_CAP rows -- more duplicates or near-duplicates of the target than that -- takes the fallback: a
        ``range_search`` just below the target's score (which has its own row-slice rung) and the canonical fp64 scores of
        the rows it returns, compared on the device.  Correct, not fast.
        ``stats``: rank_rounds (passes), rank_cap (the longest band list used), rank_band_rows (band entries re-scored, all
        passes), rank_above (rows counted without a re-score, final passes), rank_fallback_pairs, rescaled."""
        import torch
        qt, rt, shape = self._rows_arg("rank_rows", q, rows)
        f = self._filter(allowed)
        nq, m = int(rt.shape[0]), int(rt.shape[1])
        npairs = nq * m
        self.stats = {"rank_rounds": 0, "rank_cap": 0, "rank_band_rows": 0, "rank_above": 0, "rank_fallback_pairs": 0, "rescaled": 0}
        out = torch.full((npairs,), -1, dtype=torch.int64, device=self.device)
        if not npairs or not self.ntotal:
            return out.reshape(shape)
        qp = qt if m == 1 else qt.repeat_interleave(m, dim=0)
        tp = rt.reshape(-1).contiguous()
        X = torch.empty(npairs, dtype=torch.float64, device=self.device)

        def one_pass(idx, sub, cap):
            rank, cnt, above, st, Xs = self._rank_pass(qp if sub is None else qp[sub].contiguous(),
                                                       tp if sub is None else tp[sub].contiguous(), cap, f)
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
        rounds, longest, fallback = self._count_ladder("convdr_ip_rank_rows", npairs, one_pass, accept)
        self.stats.update(rank_rounds=rounds, rank_cap=longest)
        if fallback:
            stats = self.stats
            stats["rank_fallback_pairs"] = len(fallback)
            xs = X[torch.as_tensor(np.asarray(fallback, dtype=np.int64), device=self.device)].cpu().numpy()
            for j, x in zip(fallback, xs):
                t = tp[j]
                r = np.float32(x)               # the largest fp32 strictly below the target's score: every row that ties
                if not np.float64(r) < x:       # with it, or beats it, exceeds this radius
                    r = np.nextafter(r, np.float32(-np.inf))
                qj = qp[j:j + 1].contiguous()
                _, _, I = self.range_search_tensors(qj, r, allowed=f)
                Xr = self.score_rows_tensors(qj, I[None, :])[1][0]
                out[j] = ((Xr > float(x)) | ((Xr == float(x)) & (I < t))).sum()
            self.stats = stats
        return out.reshape(shape)

    def _rows_arg(self, who, q, rows):
        """(queries device fp32 [nq, d], rows device int64 [nq, m], the shape of `rows`); the checks that need no device"""
        import torch
        qt = torch.as_tensor(q)
        if qt.dim() != 2 or qt.shape[1] not in (self.d, self.d_in):
            raise ValueError("%s: queries must be [nq, %d] (got shape %s)" % (who, self.d_in, tuple(qt.shape)))
        nq = int(qt.shape[0])
        rt = torch.as_tensor(rows)
        if rt.dim() not in (1, 2) or int(rt.shape[0]) != nq:
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
        document left out.  The host ladder is that of ``rank_rows_tensors`` (one tensor read per pass, one jump to the
        reported band count, one rebuild on CONVDR_IP_RANGE).  A pair whose band holds more than RANGE_MAX_CAP rows takes the
        fallback: ``range_search`` just below the target's score, the canonical scores of the rows it returns, the ids of
        those that precede the target, the target's own id dropped, a distinct count.  Correct, not fast.
        ``stats``: rank_rounds, rank_cap, rank_band_rows (band entries re-scored, all passes), rank_above (ROWS marked without
        a re-score, final passes), rank_fallback_pairs, rescaled, ndocs."""
        import torch
        self._need_ids("rank_ids")
        qt, it, shape = self._ids_arg("rank_ids", q, ids)
        f = self._filter(allowed)
        o = self._ordinals(ordinals)
        D, R = self.score_ids_tensors(qt, it)
        if o is None:
            o = self.doc_ordinals()
        nq, m = int(qt.shape[0]), (shape[1] if len(shape) == 2 else 1)
        npairs = nq * m
        self.stats = {"rank_rounds": 0, "rank_cap": 0, "rank_band_rows": 0, "rank_above": 0, "rank_fallback_pairs": 0, "rescaled": 0,
                      "ndocs": o.ndocs}
        out = torch.full((npairs,), -1, dtype=torch.int64, device=self.device)
        if not npairs or not self.ntotal:
            return out.reshape(shape), D, R
        qt = self._queries(qt, padded_ok=True)
        qp = qt if m == 1 else qt.repeat_interleave(m, dim=0)
        tp = R.reshape(-1).contiguous()                     # (an id on no row has best row -1: the entry's padding, rank -1)
        X = torch.empty(npairs, dtype=torch.float64, device=self.device)

        def one_pass(idx, sub, cap):
            rank, cnt, above, st, Xs = self._rank_docs_pass(qp if sub is None else qp[sub].contiguous(),
                                                            tp if sub is None else tp[sub].contiguous(), cap, o, f)
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
        rounds, longest, fallback = self._count_ladder("convdr_ip_rank_docs", npairs, one_pass, accept)
        self.stats.update(rank_rounds=rounds, rank_cap=longest)
        if fallback:
            stats = self.stats
            stats["rank_fallback_pairs"] = len(fallback)
            xs = X[torch.as_tensor(np.asarray(fallback, dtype=np.int64), device=self.device)].cpu().numpy()
            col = self.ids
            for j, x in zip(fallback, xs):
                t = tp[j]
                r = np.float32(x)               # the largest fp32 strictly below the target's score (as rank_rows_tensors)
                if not np.float64(r) < x:
                    r = np.nextafter(r, np.float32(-np.inf))
                qj = qp[j:j + 1].contiguous()
                _, _, I = self.range_search_tensors(qj, r, allowed=f)
                Xr = self.score_rows_tensors(qj, I[None, :])[1][0]
                ahead = col[I[(Xr > float(x)) | ((Xr == float(x)) & (I < t))]]
                out[j] = torch.unique(ahead[ahead != col[t]]).numel()
            self.stats = stats
        return out.reshape(shape), D, R


# Pinned staging buffers and the copy thread pool are process-wide: pinning 64 MB costs ~20 ms (hipHostMalloc), i.e. a
# fresh set per index would cost as much as loading a 3 GB block through them.
_STAGING = {}
_STAGING_THREADS = {}
_POOLS = {}
import threading as _threading
_STAGING_LOCK = _threading.Lock()        # guards the dictionaries
_STAGING_BUILD = _threading.Lock()       # held while buffers are allocated and pinned
_NUMA = {}


def gpu_numa_cpus(device):
    """CPUs of the NUMA node the GPU hangs off (None when the topology cannot be read, or on a one-node host).
    A pinned buffer is placed where its allocating thread runs; across the socket link the same H2D copy runs at 29 GB/s
    instead of 57 (measured on a 2-socket MI355X host, tools/dbg/loader_probe.py) -- which is why the loader's rate, and the
    'pinned H2D ceiling' beside it, used to differ by a factor of two between boxes of one pool."""
    import torch
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx in _NUMA:
        return _NUMA[idx]
    cpus = None
    try:
        import ctypes
        buf = ctypes.create_string_buffer(64)
        # (through libconvdr_hip.so, which is bound to the HIP runtime torch loaded: dlopen-ing "libamdhip64.so" by name
        #  brings a SECOND runtime into the process, which slowed every later launch -- the training step went host-bound)
        if _lib.lib().convdr_device_pci_bus_id(int(idx), buf, 64) == 0:
            bdf = buf.value.decode().lower()
            node = int(open("/sys/bus/pci/devices/%s/numa_node" % bdf).read().strip())
            import glob
            if node >= 0 and len(glob.glob("/sys/devices/system/node/node[0-9]*")) > 1:
                got = set()
                for part in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
                    lo, _, hi = part.partition("-")
                    got.update(range(int(lo), int(hi or lo) + 1))
                got &= os.sched_getaffinity(0)
                cpus = got or None
    except Exception:
        cpus = None
    _NUMA[idx] = cpus
    return cpus


class _on_cpus:
    """Confine the calling thread to `cpus` for the duration of the block (no-op for None)."""

    def __init__(self, cpus):
        self.cpus, self.old = cpus, None

    def __enter__(self):
        if self.cpus:
            try:
                self.old = os.sched_getaffinity(0)
                os.sched_setaffinity(0, self.cpus)
            except OSError:
                self.old = None

    def __exit__(self, *exc):
        if self.old is not None:
            os.sched_setaffinity(0, self.old)


def pinned_near(device, shape, dtype):
    """A pinned host tensor allocated (first-touched and locked) on the GPU's NUMA node."""
    import torch
    with _on_cpus(gpu_numa_cpus(device)):
        t = torch.empty(shape, dtype=dtype).pin_memory()
    return t


def _staging_key(device, d, nbuf):
    return (str(device), int(d), int(nbuf))


def _staging(device, rows, d, nbuf):
    """([nbuf pinned [rows, d] fp32 buffers], [their last H2D-copy events]) of `device`: process-wide, grown on demand.
    Serialised by _STAGING_BUILD (a background pre-pin -- FlatIPIndex.prepin_staging -- and the first add() may race)."""
    import torch
    key = _staging_key(device, d, nbuf)
    with _STAGING_BUILD:
        ent = _STAGING.get(key)
        if ent is None or ent[0][0].shape[0] < rows:
            ent = ([pinned_near(device, (rows, d), torch.float32) for _ in range(nbuf)], [None] * nbuf)
            with _STAGING_LOCK:
                _STAGING[key] = ent
    return ent


def _copy_pool(threads, device=None):
    """Reader threads of the block loader; confined to the GPU's NUMA node (their destination is the pinned staging there)."""
    cpus = gpu_numa_cpus(device) if device is not None else None
    key = (threads, None if cpus is None else min(cpus))
    pool = _POOLS.get(key)
    if pool is None:
        from concurrent.futures import ThreadPoolExecutor

        def init():
            if cpus:
                try:
                    os.sched_setaffinity(0, cpus)
                except OSError:
                    pass
        pool = _POOLS[key] = ThreadPoolExecutor(max_workers=threads, initializer=init)
    return pool


def load_block(path):
    """pickle.load, as run_convdr_inference.py:164-175 does."""
    with open(path, "rb") as h:
        return pickle.load(h)


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
DISTINCT_DEEP_WS_BYTES = None   # most workspace one convdr_topk_distinct_deep call may ask for (None: FlatIPIndex.DEEP_WS_BYTES)


def distinct_topk_device(D, I, k, key_map=None):
    """``distinct_topk`` on the device, no sync: D fp32 / I int64 [nq, n <= 65536] torch tensors with unit column stride,
    key_map None or a device int64 vector.  Returns device (D, I, K [nq, k], counts [nq, 2]).
    n, k <= 4096: convdr_topk_distinct, one launch.  Beyond: convdr_topk_distinct_deep, whose keys and table live in a
    workspace allocated per call (n * 8 + at most 4n * 4 bytes per query: 1 MB at n = 65,536); the queries are split so that
    one call never asks for more than FlatIPIndex.DEEP_WS_BYTES (the calls run back to back on the stream and share it)."""
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
        budget = FlatIPIndex.DEEP_WS_BYTES if DISTINCT_DEEP_WS_BYTES is None else int(DISTINCT_DEEP_WS_BYTES)
        step, need = split_under(lambda c: L.convdr_topk_distinct_deep_workspace_bytes(c, n), max(nq, 1), budget)
        if n > FlatIPIndex.DEEP_MAX_K or k > FlatIPIndex.DEEP_MAX_K or not need:
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
        return FlatIPIndex.MAX_K
    md = int(max_depth)
    if md < 1 or md > FlatIPIndex.DEEP_MAX_K:
        raise ValueError("%s: max_depth = %d is outside 1..%d (FlatIPIndex.DEEP_MAX_K)" % (who, md, FlatIPIndex.DEEP_MAX_K))
    return md


def _distinct_row_depth(who, topN, rows_per_key, limit, limit_name):
    """m = topN * rows_per_key, the row depth at which a walk over block files holds topN keys for every query."""
    m = topN * rows_per_key
    if topN < 1 or rows_per_key < 1 or m > limit:
        raise ValueError("%s: topN * rows_per_key = %d * %d = %d is outside 1..%d (%s)" % (who, topN, rows_per_key, m, limit, limit_name))
    return m


def _check_distinct_certificate(who, counts, topN, m, rows_per_key, ann_data_dir, max_blocks, key_map):
    """The certificate of the ONE distinct step after a block walk at row depth m: a query with fewer than topN keys in m rows
    of a corpus that has more rows means rows_per_key was understated."""
    from . import blocks
    if (counts[:, 0] < 0).any():
        raise _lib.ConvdrError("%s: a record offset lies outside key_map (%d entries)" % (who, len(key_map)))
    open_ = np.nonzero((counts[:, 0] < topN) & (counts[:, 1] >= m))[0]
    if len(open_):
        most, total = blocks.key_row_stats(ann_data_dir, max_blocks, key_map)
        if total > m:
            raise _lib.ConvdrError("%s: %d queries hold fewer than %d keys in their top %d rows: "
                                   "rows_per_key = %d is understated (the id files give %d)"
                                   % (who, len(open_), topN, m, rows_per_key, most))


def search_distinct_one_by_one(ann_data_dir, gpu_index, query_embedding, topN, rows_per_key=None, key_map=None, max_blocks=8,
                               timings=None, max_depth=None):
    """``search_one_by_one`` at DOCUMENT level: per query the topN best distinct keys over all block files, each with the
    score and record offset of its best row -- what the reference gets from search_one_by_one + the `seen_pid` walk of
    EvalDevQuery (run_convdr_inference.py:58-69) only while the top-topN ROWS still hold topN documents.
    key: the record offset itself (key_map=None: MaxP blocks, where encode.py repeats the offset for every chunk row) or
    key_map[offset] (e.g. offset2pid, for a corpus with duplicate pids; numpy or torch int64).
    rows_per_key: the most rows any key owns (None: counted from the id files, blocks.max_rows_per_key).  The block walk
    runs ONCE, at row depth m = topN * rows_per_key <= FlatIPIndex.MAX_K -- deep enough for every query when rows_per_key
    is right -- the running merge is cut to m columns and ONE distinct step (device: convdr_topk_distinct) follows.  The
    certificate is checked: a query with fewer than topN keys in m rows of a corpus that has more rows means rows_per_key
    was understated -> ConvdrError; the walk is never silently repeated.
    Returns (D float64 [nq, topN], record offsets int64 [nq, topN]), the shapes EvalDevQuery reads; a corpus with fewer
    than topN keys leaves (-3.4028235e38, -1) in the tail.  Host path (an index without search_begin): every block needs
    at least m rows, as the reference's own id lookup does.
    max_depth (default FlatIPIndex.MAX_K, at most DEEP_MAX_K): the bound of m.  Beyond 4,096 the block searches are the deep
    ones, the running merge is merge_topk_sorted and the distinct step convdr_topk_distinct_deep."""
    from . import blocks
    max_depth = _check_max_depth("search_distinct_one_by_one", max_depth)
    topN = int(topN)
    if rows_per_key is None:
        rows_per_key = blocks.max_rows_per_key(ann_data_dir, max_blocks, key_map)
    rows_per_key = int(rows_per_key)
    m = _distinct_row_depth("search_distinct_one_by_one", topN, rows_per_key, max_depth,
                            "FlatIPIndex.MAX_K" if max_depth == FlatIPIndex.MAX_K else "max_depth")
    merged = _search_block_list(ann_data_dir, gpu_index, query_embedding, m, range(max_blocks), True, timings)
    if merged is None:
        raise FileNotFoundError("no passage blocks under %s" % ann_data_dir)
    if hasattr(gpu_index, "search_begin"):
        import torch
        Dm, Im = merged[0][:, :m], merged[1][:, :m]
        km = key_map
        if km is not None:
            km = (km if torch.is_tensor(km) else torch.from_numpy(np.asarray(km, dtype=np.int64))).to(Dm.device, torch.int64)
        D, I, _, counts = distinct_topk_device(Dm, Im, topN, km)
        D, I, counts = D.double().cpu().numpy(), I.cpu().numpy(), counts.cpu().numpy()
    else:
        km = key_map.cpu().numpy() if hasattr(key_map, "cpu") else key_map
        D, I, _, counts = distinct_topk(merged[0][:, :m], merged[1][:, :m], topN, km)
    _check_distinct_certificate("search_distinct_one_by_one", counts, topN, m, rows_per_key, ann_data_dir, max_blocks, key_map)
    return D, I


def search_one_by_one(ann_data_dir, gpu_index, query_embedding, topN, max_blocks=8, timings=None):
    """Block-by-block search + merge; same contract as the reference function (float64 scores, int64 offsets,
    2 * topN columns once two blocks have been merged).  With a FlatIPIndex the embedding block is memory-mapped
    (blocks.BlockView: no pickle.load copy) and streamed to HBM in pinned chunks (FlatIPIndex.add), and the per-block
    results, the offset lookup ``embid[I]`` and the running merge stay on the device; any other index object
    (``.add/.search/.reset``) takes the reference's host path.
    Device path, pipelined: TWO blocks are in flight -- the first scan pass of block i is enqueued (search_begin, no host
    round trip), then the host reads block i + 1 into the twin index (file -> pinned staging -> HBM on the copy stream)
    while the GPU searches block i; block i's certificates are read (search_finish), its result merged and its storage
    dropped only after that.  The reference's load -> add -> search -> merge -> reset is strictly serial (:157-242).
    HBM residency: with two blocks in flight TWO fp32 blocks and their 16-bit scan copies are resident at once (2 x 1.5 x the
    block: 44 GB for CAsT's 14.6 GB blocks, of 288 GB) -- pass an index that is not a FlatIPIndex-with-twin, or search block
    files one at a time with index.add(BlockView) / search / reset yourself, where that does not fit.
    timings (optional dict): filled with the wall seconds spent per stage."""
    merged = _search_block_list(ann_data_dir, gpu_index, query_embedding, topN, range(max_blocks), True, timings)
    if merged is None:
        raise FileNotFoundError("no passage blocks under %s" % ann_data_dir)
    if hasattr(gpu_index, "search_begin"):
        return merged[0].double().cpu().numpy(), merged[1].cpu().numpy()
    return merged


def _search_block_list(ann_data_dir, gpu_index, query_embedding, topN, block_ids, stop_at_missing, timings=None):
    """The loop of ``search_one_by_one`` over the block files `block_ids`, in that order.  stop_at_missing: the first
    block whose embedding or id file cannot be read ends the walk (the reference's discovery, run_convdr_inference.py:
    159-177); otherwise (parallel.search_blocks_sharded: the ids of blocks that were found) such a block is an error.
    Returns the running merge as it stands -- device tensors (fp32, int64) on the device path, numpy (float64, int64) on
    the host path -- or None when no block was searched."""
    import time
    from . import blocks
    on_device = hasattr(gpu_index, "search_begin")
    merged = None
    tm = {"load_add_s": 0.0, "search_finish_merge_s": 0.0, "blocks": 0, "bytes": 0}

    def paths(block_id):
        return (os.path.join(ann_data_dir, "passage__emb_p__data_obj_%d.pb" % block_id),
                os.path.join(ann_data_dir, "passage__embid_p__data_obj_%d.pb" % block_id))
    if on_device:
        import torch
        twins = [gpu_index, None]
        pending = None                       # (handle, index, embid) of the block whose first pass is in flight

        def finish(p):
            nonlocal merged
            handle, idx, ids = p
            D, I = idx.search_finish(handle)
            embid = torch.as_tensor(np.asarray(ids, dtype=np.int64), device=D.device)
            found = torch.where(I >= 0, embid[I.clamp_min(0)], I) if embid.numel() else I   # -1 padding when n < topN
            cand = (D, found)
            merged = cand if merged is None else merge_topk_device(merged, cand, topN)
            idx.reset()
        for pos, block_id in enumerate(block_ids):
            emb_path, id_path = paths(block_id)
            try:
                view = blocks.BlockView(emb_path)
            except Exception:
                if stop_at_missing:
                    break
                raise
            try:
                try:
                    ids = load_block(id_path)
                except Exception:
                    if stop_at_missing:
                        break
                    raise
                idx = twins[pos & 1]
                if idx is None:
                    idx = twins[pos & 1] = gpu_index.twin()
                t0 = time.perf_counter()
                idx.add(view)                # the host reads; the GPU meanwhile searches the previous block
                t1 = time.perf_counter()
                tm["load_add_s"] += t1 - t0
                tm["bytes"] += int(view.array.nbytes)
                tm["blocks"] += 1
                if pending is not None:
                    finish(pending)
                pending = (idx.search_begin(query_embedding, topN), idx, ids)
                tm["search_finish_merge_s"] += time.perf_counter() - t1
            finally:
                view.close()                 # (streamed blocks: read by host threads that add() has joined; small blocks:
                                             #  copied synchronously by add() -- nothing reads the mapping any more)
        if pending is not None:
            t1 = time.perf_counter()
            finish(pending)
            tm["search_finish_merge_s"] += time.perf_counter() - t1
        if timings is not None:
            timings.update(tm)
        return merged
    for block_id in block_ids:
        emb_path, id_path = paths(block_id)
        try:
            passage_embedding = load_block(emb_path)
            passage_embedding2id = load_block(id_path)
        except Exception:
            if stop_at_missing:
                break
            raise
        gpu_index.add(passage_embedding)
        D, I = gpu_index.search(query_embedding, topN)
        cand = (D.astype(np.float64), np.asarray(passage_embedding2id)[I])
        merged = cand if merged is None else merge_topk(merged, cand, topN)
        gpu_index.reset()
    return merged


def EvalDevQuery(query_embedding2id, merged_D, dev_query_positive_id, I_nearest_neighbor, topN, output_file,
                 output_trec_file, offset2pid, raw_data_dir, output_query_type, raw_sequences=None,
                 load_collection=None):
    """Result writer with the reference's exact text output (run_convdr_inference.py:21-113).
    The offset -> pid mapping and the first-occurrence de-duplication (:56-69) run as array operations per query (one
    gather + one np.unique over the topN candidates) instead of the reference's Python loop over nq x topN entries."""
    ranked = {}
    raw = {}
    o2p = np.asarray(offset2pid)
    I_top = np.asarray(I_nearest_neighbor)[:, :topN]
    D_top = np.asarray(merged_D)[:, :topN]
    pids_all = o2p[I_top]                                   # offset -> pid for every candidate at once
    for query_idx in range(len(I_top)):
        query_id = query_embedding2id[query_idx]
        if query_id not in ranked:
            ranked[query_id] = [(0, 0)] * topN
        raw[query_id] = raw_sequences[query_idx]
        row = pids_all[query_idx]
        _, first = np.unique(row, return_index=True)        # first occurrence of every pid ...
        first.sort()                                        # ... in rank order
        scores = D_top[query_idx][first].tolist()
        for rank, (pid, score) in enumerate(zip(row[first].tolist(), scores)):
            ranked[query_id][rank] = (pid, score)
    queries = {}
    with open(os.path.join(raw_data_dir, "queries." + output_query_type + ".tsv")) as f:
        for line in f:
            qid, query = line.strip().split("\t")
            queries[qid] = query
    collection = os.path.join(raw_data_dir, "collection.jsonl")
    if not os.path.exists(collection):
        collection = os.path.join(raw_data_dir, "collection.tsv")
        if not os.path.exists(collection):
            raise FileNotFoundError("Neither collection.tsv nor collection.jsonl found in {}".format(raw_data_dir))
    all_passages = (load_collection or _load_collection)(collection)
    with open(output_file, "w") as f, open(output_trec_file, "w") as g:
        for qid, passages in ranked.items():
            for i in range(topN):
                pid, score = passages[i]
                label = 0 if qid not in dev_query_positive_id else dev_query_positive_id[qid].get(pid, 0)
                f.write(json.dumps({"query": queries[qid], "doc": all_passages[pid], "label": label,
                                    "query_id": str(qid), "doc_id": str(pid), "retrieval_score": score,
                                    "input": raw[qid]}) + "\n")
                g.write(str(qid) + " Q0 " + str(pid) + " " + str(i + 1) + " " + str(-i - 1 + 200) + " ance\n")


class _Passages(dict):
    def __missing__(self, key):
        return "[INVALID DOC ID]"


def _load_collection(collection_file):
    """utils/util.py:327-352 without the 50M-entry list: a dict with the same default."""
    all_passages = _Passages()
    ext = collection_file[collection_file.rfind(".") + 1:]
    if ext not in ["jsonl", "tsv"]:
        raise TypeError("Unrecognized file type")
    with open(collection_file) as f:
        for line in f:
            line = line.strip()
            if ext == "jsonl":
                obj = json.loads(line)
                all_passages[int(obj["id"])] = obj["title"] + "[SEP]" + obj["text"]
            else:
                try:
                    arr = line.split("\t")
                    all_passages[int(arr[0])] = arr[1].rstrip()
                except IndexError:
                    print("bad passage")
                except ValueError:
                    print("bad pid")
    return all_passages
