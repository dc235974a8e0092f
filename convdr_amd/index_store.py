"""The rows a FlatIPIndex holds: the resident buffers (fp32 block, scan copy, remainder copy, id column) and everything that writes
them or speaks only about rows and ids -- add / update / remove, row filters, the id operations, reading rows back.  The questions
asked of the rows (search, range, score, rank) are ``search.FlatIPIndex(_IndexStore)``; nothing here calls into it."""
import functools
import os

import numpy as np

from . import _lib
from .staging import _STAGING, _STAGING_LOCK, _STAGING_THREADS, _copy_pool, _staging, _staging_key
from .stores import _HALF_PRECISIONS, _KINDS, HALF_NORM_LIMIT, SQ8_MAX_D, SQ8_REFUSED, STORES

RESERVED_ID = -(1 << 63)    # INT64_MIN: the free-slot marker of the key set (csrc/ip_keys.hpp), no legal row id
KEY_ST_LIST, KEY_ST_PROBE, KEY_ST_COLUMN, KEY_ST_NOSET = 1, 2, 4, 8      # status bits of convdr_keyset_build / the row passes
ROW_FILTER_TILE = 256       # the bitmap covers whole scan tiles of this many rows (csrc/ip_scan.hpp: Tile256::TR)


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


EXCLUDE_MAX = 16384         # entries per query of an exclusion list, before de-duplication (csrc/ip_exclude.hpp: EXCL_MAX_ENTRIES)
EXCL_ST_ROW, EXCL_ST_LONG = 1, 2     # status bits of convdr_excl_build_*: a row >= ntotal; more than EXCLUDE_MAX entries


def pack_exclusions(rows, nq):
    """The per-query exclusion lists of `nq` queries as ONE padded int64 array [nq, e] (negative = padding): the checks that
    need no device.  rows: an integer array [nq, e] (numpy, or a torch tensor on any device: returned as int64 where it lives),
    or a host sequence of nq integer sequences of different lengths (padded with -1 to the longest).  Any order, repeats
    allowed.  ValueError for another shape, a non-integer dtype (bool included), or more than EXCLUDE_MAX = 16,384 entries per
    query -- of an array, the width e (padding included: it is what the build sorts); of a sequence, its length."""
    import torch
    nq = int(nq)

    def width_ok(e):
        if e > EXCLUDE_MAX:
            raise ValueError("exclude: %d entries per query, at most %d" % (e, EXCLUDE_MAX))
    if isinstance(rows, torch.Tensor):
        if rows.dim() != 2 or int(rows.shape[0]) != nq:
            raise ValueError("exclude: rows must be [nq, e] with nq = %d (got shape %s)" % (nq, tuple(rows.shape)))
        if rows.is_floating_point() or rows.is_complex() or rows.dtype == torch.bool:
            raise ValueError("exclude: rows must be integers (got %s)" % rows.dtype)
        width_ok(int(rows.shape[1]))
        return rows.to(torch.int64)
    if isinstance(rows, np.ndarray) and rows.dtype != object:
        if rows.ndim != 2 or rows.shape[0] != nq:
            raise ValueError("exclude: rows must be [nq, e] with nq = %d (got shape %s)" % (nq, rows.shape))
        if rows.dtype.kind not in "iu":
            raise ValueError("exclude: rows must be integers (got %s)" % rows.dtype)
        width_ok(rows.shape[1])
        return rows.astype(np.int64)
    try:
        lists = list(rows)
    except TypeError:
        raise ValueError("exclude: rows must be an integer array [nq, e] or a sequence of nq integer sequences") from None
    if len(lists) != nq:
        raise ValueError("exclude: %d lists for nq = %d queries" % (len(lists), nq))
    cols = []
    for j, one in enumerate(lists):
        if isinstance(one, torch.Tensor):
            one = one.cpu().numpy()
        a = np.asarray(one)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError("exclude: the list of query %d must be a sequence of integers (got %s, shape %s)" % (j, a.dtype, a.shape))
        width_ok(a.size)
        cols.append(a.astype(np.int64))
    out = np.full((nq, max([c.size for c in cols], default=0)), -1, dtype=np.int64)
    for j, c in enumerate(cols):
        out[j, :c.size] = c
    return out


class QueryExclusions:
    """Per-query excluded rows of an index (FlatIPIndex.exclude_rows / exclude_ids), the operand of ``FlatIPIndex.excluding`` (the exact entries with per-query exclusions):
    `rows` the device lists [nq, ld] (int32 words, the bytes of uint32: each query's excluded rows ascending and distinct, then
    0xffffffff; ld a multiple of 4), `count` device int32 [nq]; on the host `nq`, `n` (the ntotal it was built for) and `e_max`
    (the longest list), all from the build's one host read.  Reusable across calls; ``select(idx)`` takes a subset of the queries.
    Stale under RowFilter's rule: another ntotal or device raises ValueError -- and, as for a RowFilter, ``upsert_docs`` may move
    rows without changing ntotal: rebuild after it."""

    def __init__(self, rows, count, counts_host, n):
        self.rows, self.count, self.n = rows, count, int(n)
        self._host = np.asarray(counts_host, dtype=np.int64).reshape(-1)
        self.nq = int(self._host.size)
        self.e_max = int(self._host.max()) if self.nq else 0

    def select(self, idx):
        """the exclusions of the queries `idx` (integer indices: a sequence, numpy or torch), in that order; no device read
        unless `idx` lives on a device"""
        import torch
        i = (idx.cpu().numpy() if isinstance(idx, torch.Tensor) else np.asarray(idx)).astype(np.int64).reshape(-1)
        t = torch.as_tensor(i, device=self.rows.device)
        return QueryExclusions(self.rows[t].contiguous(), self.count[t].contiguous(), self._host[i], self.n)


class DocOrdinals:
    """Dense document numbers of an index's id column (FlatIPIndex.doc_ordinals): `ord` the device vector [ntotal] (int32
    words, the bytes of uint32: ord[r] = the number of distinct ids whose first row lies below the first row of ids[r]),
    `ndocs` the distinct ids, `n` the ntotal it was built for -- ranking with it on an index of another size raises ValueError.
    Query independent: build once, pass as ``ordinals=`` to rank_ids / rank_ids_tensors."""

    def __init__(self, ord, ndocs, n):
        self.ord, self.ndocs, self.n = ord, int(ndocs), int(n)


class _IndexStore:
    """The storage half of FlatIPIndex (see there for the constructor's arguments)."""

    # state an index has from birth, whatever constructed it: the id column and its ping-pong partner (keep_rows), the id
    # operations' workspace, the H2D stream of the streamed add; a reservation; "auto" starts on the split scan
    _sid = _sid_spare = _key_ws = _copy_stream = None
    _reserved = _x3_first = False
    _store = STORES["fp32"]     # (the default storage's, for an index built without the constructor; the constructor sets its own)

    def __init__(self, d, device=None, cap=4096, rank_target=0, precision="auto", center=None, prepin=True, storage="fp32"):
        if storage not in STORES:
            raise ValueError("FlatIPIndex: storage must be 'fp32', 'fp16' or 'sq8' (got %r)" % (storage,))
        self.storage, self._store = storage, STORES[storage]
        center = self._store.admit(precision, center, d)
        import torch
        if not torch.cuda.is_available():
            raise _lib.ConvdrError("FlatIPIndex needs a GPU (no CPU fallback)")
        assert precision in self._store.precisions, precision
        _lib.lib()
        # the scan contracts in 64-wide K steps (128 for the 8-bit store: one K step is 128 bytes): other widths get zero
        # columns, which add exact zeros to every score
        self.d_in, kstep = int(d), self._store.kstep
        self.d = (self.d_in + kstep - 1) // kstep * kstep
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.cap, self.rank_target = int(cap), int(rank_target)
        self.precision, self.center = precision, center
        self.kind = self._store.kind or _KINDS[precision]
        self._scan_dtype = {"f16": torch.float16, "bf16": torch.bfloat16, "i8": torch.int8}[self.kind]
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
            if not ((ent is not None and ent[0][0].shape[0] >= rows) or (th is not None and th.is_alive())):
                th = threading.Thread(target=_staging, args=(self.device, rows, self.d, key[2]), daemon=True, name="convdr-prepin")
                _STAGING_THREADS[key] = th
                th.start()
        if wait and th is not None:
            th.join()

    def twin(self):
        """An empty index with this one's parameters (search_one_by_one keeps two blocks in flight: one being searched, one
        being loaded)."""
        t = type(self)(self.d_in, device=self.device, cap=self.cap, rank_target=self.rank_target, precision=self.precision,
                         center=None if self._store.centred is not None else self.center, prepin=False, storage=self.storage)
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
        """The rows the canonical re-score reads: the fp32 block, or the half / 8-bit store itself."""
        return self._pbf if self._s32 is None else self._p32

    @property
    def store(self):
        """storage="fp16": the resident halves [ntotal, d] = 2^s x the stored passages (s: ``_scale``)."""
        return getattr(self, self._store.store_view) if self._store.store_view else None

    def _row_pair(self, sel):
        """(re-score rows, scan copy) of a slice or an index vector of the resident rows, contiguous"""
        r = self._rows[sel].contiguous()
        return (r, r) if self._s32 is None else (r, self._pbf[sel].contiguous())

    def _operands(self, rows=None):
        """What a block looks like to the C ABI: (store code 0 bf16 / 1 fp16 / 2 half store / 3 8-bit store, fp32 rows or NULL,
        scan operand, scale of that operand -- the 8-bit store: its step vector --, centre or NULL) of the resident block, or of
        `rows` = (re-score rows, scan copy) of a slice.  The half store has no fp32 rows and no centre, the bf16 copy no scale;
        the 8-bit store's largest row L1 norm of the codes travels in the max norm's place."""
        p32, p16 = (self._rows, self._pbf) if rows is None else rows
        return self._store.block(self, p32, p16)

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
        if not self._reserved:
            self._s32 = self._s16 = self._slo = None
        self._sid = self._sid_spare = None      # the id column and its ping-pong partner (keep_rows): an index has ids or not,
                                                # from its first add on; a reset forgets that too
        self._centre = None
        self._scale = 1.0                       # power of two applied to the fp16 scan copy (1 for bf16)
        self._max_norm = torch.zeros(1, dtype=torch.float32, device=self.device)
        if self._store.words:
            # the max norm (the 8-bit store: the largest row L1 norm of the codes, in its role) and the store's words side by
            # side: ONE host read at the end of an add()
            self._mf = torch.zeros(3, dtype=torch.float32, device=self.device)
            self._max_norm = self._mf[:1]
            for j, name in enumerate(self._store.words, 1):
                setattr(self, name, self._mf[j:j + 1].view(torch.int32))
        for name, value in self._store.fields:
            setattr(self, name, value)
        self._ws = None
        self._x3_first = False

    def release(self):
        self._reserved = False
        self.reset()

    def reserve(self, n, lo=None):
        """Backing storage for n passages (fp32 block + 16-bit scan copy, + the remainder copy of the split scan when
        `lo`, default: only if the precision pins it; + the id column of an index that carries ids).  Existing rows are kept."""
        import torch
        # the buffers this index holds: a half or 8-bit store keeps its one buffer and nothing else
        held = {name: torch.float32 if name == "_s32" else self._scan_dtype for name in self._store.buffers}
        if "_slo" in held and self._slo is None and not ((self.precision in ("bf16x3", "fp16x3")) if lo is None else bool(lo)):
            del held["_slo"]
        rows = max(int(n), 0 if self._s16 is None else self._s16.shape[0])      # (all of them keep one row count)
        with torch.cuda.device(self.device):
            for name, dtype in held.items():
                old = getattr(self, name)
                if old is None or old.shape[0] < rows:
                    t = torch.empty((rows, self.d), dtype=dtype, device=self.device)
                    if old is not None and self._n:
                        t[:self._n].copy_(old[:self._n])
                    setattr(self, name, t)
            if self._sid is not None:
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
        ptr = _lib.ptr
        name, scale = ("convdr_ip_prepare_block_f16", (float(self._scale),)) if self.kind == "f16" else ("convdr_ip_prepare_block", ())
        _lib.check(getattr(_lib.lib(), name)(ptr(src32), src32.shape[0], self.d, ptr(self._centre), *scale, ptr(dst16), ptr(dstlo),
                                             ptr(self._max_norm), _lib.stream_ptr()), name)

    def _first_rows(self, t):
        """The first rows an empty index sees (of a streamed add: the first chunk, >= 40 k passages) fix its centring vector --
        any centre keeps the search exact, it only has to be close to the mean to shrink the rounding-error band -- and, for the
        fp16 scan, the power-of-two scale of the scan copy (from these rows' largest centred norm: one extra pass over them and one
        host read per index lifetime; later rows may be up to 7x longer before the copy has to be rebuilt, see _rebuild_scaled)."""
        if self.center:
            self._set_centre(t)
        if self.kind == "f16":
            L = _lib.lib()
            _lib.check(L.convdr_ip_prepare_block_f16(_lib.ptr(t), t.shape[0], self.d, _lib.ptr(self._centre), 1.0, None, None,
                                                     _lib.ptr(self._max_norm), _lib.stream_ptr()), "convdr_ip_prepare_block_f16")
            self._scale = float(L.convdr_ip_f16_scale(float(self._max_norm.item())))
        return t

    def _rebuild_scaled(self):
        """CONVDR_IP_RANGE: rows added after the scale was fixed are more than 7x longer than the first block's longest: the scale
        is re-derived from the block's max norm and the scan copy rebuilt, or the half store's rows rescaled in place."""
        import torch
        with torch.cuda.device(self.device):
            self._store.rescale(self)

    def _grow_for(self, m, want_lo=False):
        """rows [n, n + m) of the backing storage (fp32 block, scan copy, remainder copy; None for a buffer the index does not
        hold), growing it when needed (exact fit unless reserved larger)"""
        need = self._n + m
        if self._s16 is None or self._s16.shape[0] < need or (want_lo and self._slo is None):
            keep = self._reserved
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
            if self._n and self._sid is not None:
                raise ValueError("FlatIPIndex.add: this index carries row ids (%d rows), an add without ids= would leave rows "
                                 "without one; the index is unchanged" % self._n)
            return self._add_rows(x, chunk_bytes)
        if self._n and self._sid is None:
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
        """add() without the id column, for every store.  The description supplies what differs (stores.py): the dtypes a source may
        keep, the room for the new rows (the fp32 store adopts the caller's device tensor as its first block), what the first rows of
        an empty index fix, where streamed chunks land (in the store itself; later adds of the 8-bit store: one window of the staging
        ring at a time), how rows are written, and the verdict after the add's ONE host read -- keep, refuse and restore, or, for
        the half store only, lower the scale and write once more."""
        import time
        import torch
        s = self._store
        chunk_bytes = int(chunk_bytes or self.host_chunk_bytes)
        have = str(getattr(x.array if hasattr(x, "array") else x, "dtype", "")).replace("torch.", "")
        t, reader = self._source(x, chunk_bytes, np.dtype(have if have in s.streams and self.d == self.d_in else s.streams[-1]),
                                 tuple(getattr(torch, name) for name in s.keeps))
        m, n0 = int(t.shape[0]), self._n
        if m == 0:
            return
        with torch.cuda.device(self.device):
            t0 = time.perf_counter() if s.clock_growth else None
            state0 = ({a: getattr(self, a) for a in s.fixes}, self._mf.clone()) if s.words else None
            host = isinstance(t, np.ndarray)
            bounce = functools.partial(torch.empty, dtype=getattr(torch, t.dtype.name), device=self.device) if host else None
            if host and n0 == 0 and s.first_needs_all:
                # a host array goes whole into a transient buffer of the add's size (the 8-bit store: 4 d bytes per row for fp32
                # input, 2 d for fp16 -- build a large index from a first block it can afford)
                tmp = bounce((m, self.d))
                self._stream_rows(t, tmp, reader, chunk_bytes, lambda ci, lo, hi: None)
                t, host = tmp, False
            dst = s.room(self, t, m)

            def resident(rows, lo, hi):         # landed rows -> rows [lo, hi) of the new resident ones
                p32, p16, plo = (None if b is None else b[lo:hi] for b in dst)
                if p32 is not None and rows.data_ptr() != p32.data_ptr():       # (streamed chunks landed in the block, an adopted
                    p32.copy_(rows)                                             #  tensor is the block)
                s.write(self, rows if p32 is None else p32, p16, plo)
            for attempt in (0, 1):
                fresh = n0 == 0 and not attempt
                if host:
                    land, win = s.landing(self, t, dst, chunk_bytes)
                    land = bounce((min(win, m), self.d)) if land is None else land
                    for a in range(0, m, win):
                        def each(ci, lo, hi, a=a):
                            if fresh and a == 0 and ci == 0:
                                s.first(self, land[lo:hi])
                            resident(land[lo:hi], a + lo, a + hi)
                        rd = None if reader is None else (lambda buf, lo, hi, a=a, **kw: reader(buf, a + lo, a + hi, **kw))
                        self._stream_rows(t[a:a + win], land[:min(m, a + win) - a], rd, chunk_bytes, each, t0)
                else:
                    resident(s.first(self, t) if fresh else t, 0, m)
                if s.verdict(self, n0, state0, attempt):
                    break
            self._n = n0 + m

    def _restore(self, state0):
        """what a refused add puts back: what the first rows fixed, and the max norm with its words"""
        for name, value in state0[0].items():
            setattr(self, name, value)
        self._mf.copy_(state0[1])

    def _add_half(self, x, chunk_bytes):
        return self._add_rows(x, chunk_bytes)

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
        return src

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
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        stage, freed = _staging(self.device, min(per32, (n * dst.element_size() + 3) // 4), d, nbuf)
        stage = [b.view(dst.dtype).view(-1, d) for b in stage]
        cs = self._copy_stream
        cs.wait_stream(main)                    # (allocation order / the copy of the old rows in _grow_for)
        threads = self._copy_threads()
        pool = _copy_pool(threads * (nbuf - 1), self.device)
        chunks = [(s, min(n, s + rows_per)) for s in range(0, n, rows_per)]

        def fill(ci):
            """start filling staging buffer ci % nbuf with chunk ci: `threads` positioned reads / memcpy slices"""
            s, e = chunks[ci]
            bi = ci % nbuf
            # staging buffer bi may be refilled once its previous H2D copy has completed.  The events live with the
            # buffers (module-level, shared by every index of the process): the last copies of one add() are still in
            # flight when the next add() starts filling (1 run in ~500 put rows of a second block into the first
            # before they did, tests/test_ip_search_gpu.py::test_back_to_back_streamed_adds_keep_their_rows).
            # The rule, for every user of the buffers (this loop, _load_bytes, and save's _save_bytes, which runs them the
            # other way): freed[bi] is the event of the LAST device copy that read or wrote buffer bi, recorded on the
            # stream that ran it; whoever touches the buffer next waits for it first (the host with synchronize(), a copy
            # stream with wait_event()); and nobody returns to its caller while a host thread still reads or writes a
            # buffer.  A save therefore leaves every freed[bi] recorded and its file writes returned.
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
        self._centre = self._max_norm.new_empty(self.d)         # (fp32, on the index's device)
        self._column_pass("convdr_ip_column_mean", t, (), self._centre)

    def _column_pass(self, name, t, given, out):
        """convdr_ip_column_mean / _absdev over the fp32 rows `t` into out [d]; given: the vector arguments before the scratch"""
        import torch
        scratch = torch.empty(1024 * self.d, dtype=torch.float32, device=self.device)
        _lib.check(getattr(_lib.lib(), name)(_lib.ptr(t), t.shape[0], self.d, *given, _lib.ptr(scratch), _lib.ptr(out),
                                             _lib.stream_ptr()), name)

    def _ensure_lo(self):
        """Remainder copy for the split scan, built on first use."""
        import torch
        if self._slo is None and self._s32 is not None:      # (a store without an fp32 block has no remainder copy)
            with torch.cuda.device(self.device):
                self._slo = torch.empty((self._s32.shape[0], self.d), dtype=self._scan_dtype, device=self.device)
                if self._n:
                    self._prepare_into(self._p32, self._pbf, self._plo)

    def update_rows(self, row0, emb):
        """Overwrite rows [row0, row0 + len(emb)) of the resident block with freshly encoded embeddings
        (device fp32 [m, d]) and refresh their scan copy / the block's max norm.  No sync."""
        import torch
        self._store.refuse(self, "update_rows")
        m = int(emb.shape[0])
        assert emb.dtype == torch.float32 and emb.is_contiguous() and row0 + m <= self.ntotal
        dst16, dstlo = self._pbf[row0:row0 + m], None if self._slo is None else self._plo[row0:row0 + m]
        if self._s32 is None:
            # the half store: the new rows are rounded to half and scaled; a row the store cannot hold is an error AFTER the write
            # (the caller owns the rows it overwrites), a scale the rows outgrow is CONVDR_IP_RANGE at the next search, as for add()
            src = (emb if self.d == self.d_in else torch.nn.functional.pad(emb, (0, self.d - self.d_in))).contiguous()
        else:
            src = self._p32[row0:row0 + m]
            src[:, :self.d_in].copy_(emb)        # (zero columns of a padded width stay zero)
        with torch.cuda.device(self.device):
            self._store.write(self, src, dst16, dstlo, update=True)

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
            if self._sid is not None:
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
        return None if self._sid is None else self._sid[:self._n]

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
        ws = self._key_workspace(need)
        status = torch.empty(1, dtype=torch.int32, device=self.device)
        _lib.check(L.convdr_keyset_build(ptr(t), m, ptr(ws), ws.numel(), ptr(status), _lib.stream_ptr()), "convdr_keyset_build")
        return ws, status

    def _key_workspace(self, need, keep=0):
        """the workspace of the id operations, at least `need` bytes; one that has to grow takes the first `keep` bytes over"""
        import torch
        ws = self._key_ws
        if ws is None or ws.numel() < need:
            self._key_ws = torch.empty(int(need), dtype=torch.uint8, device=self.device)
            if keep:
                self._key_ws[:keep].copy_(ws[:keep])
        return self._key_ws

    @staticmethod
    def _key_codes(ws, status):
        """the two status words (the build's, the row pass's) as device int64 [2], to ride along with the caller's host read"""
        import torch
        return torch.cat([status, ws[:4].view(torch.int32)]).to(torch.int64)

    def _key_read(self, who, parts, ws, status=None, reserved_ok=False):
        """THE host read of an id operation: the caller's device int64 vectors `parts` and the status words (`status`, the build's,
        where a set was built; the row pass's, in the workspace's head) in one copy.  The words go through _key_status
        (reserved_ok: INT64_MIN in the list is padding, not an error); `parts` come back joined, as numpy int64."""
        import torch
        codes = ws[:4].view(torch.int32).to(torch.int64) if status is None else self._key_codes(ws, status)
        got, words = np.split(torch.cat([*parts, codes]).cpu().numpy(), [-int(codes.numel())])
        self._key_status(who, int(np.bitwise_or.reduce(words)) & ~(KEY_ST_LIST if reserved_ok else 0))
        return got

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
            got = self._key_read(who, [counts], ws, status)
        return bits, int(got[0]), int(got[1])

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
        return self._locate("rows_of", ids)[1:3]

    def reconstruct_ids(self, ids):
        """FAISS ``IndexIDMap2.reconstruct`` for a list: float32 numpy [m, d_in], the first row of every id (rows_tensors of
        rows_of).  An id that is on no row raises IndexError."""
        first, _ = self.rows_of(ids)
        if first.numel():
            absent = int((first < 0).sum().item())
            if absent:
                raise IndexError("reconstruct_ids: %d of the %d ids are on no row" % (absent, int(first.numel())))
        return self.rows_tensors(first).cpu().numpy()

    def _emb_arg(self, who, emb, rows):
        import torch
        if not (isinstance(emb, torch.Tensor) and emb.dtype == torch.float32 and emb.device == self.device
                and tuple(emb.shape) == (rows, self.d_in)):
            raise ValueError("%s: emb must be a float32 tensor [%d, %d] on %s" % (who, rows, self.d_in, self.device))

    @staticmethod
    def _no_repeats(who, dup):
        rep = np.nonzero(dup != np.arange(len(dup)))[0]
        if rep.size:
            raise ValueError("%s: the list repeats an id (position %d repeats position %d); nothing was written"
                             % (who, int(rep[0]), int(dup[rep[0]])))

    def upsert(self, ids, emb):
        """Re-encoded passages: `emb` (device fp32 [m, d_in]) replaces the rows of `ids` (int64 [m]).  An id that is on exactly
        one row gets that row overwritten in place (the scan copies and the max norm refreshed as by update_rows; the half
        store's update_flags() rule applies); an id on no row is appended, in list order, with its id.  Returns
        (n_updated, n_added).  A list that repeats an id, or an id that sits on more than one row (chunk rows: which one?),
        raises ValueError BEFORE anything is written -- one host read, the one that also splits the list."""
        import torch
        self._store.refuse(self, "upsert")
        t, first, count, dup, ws, status = self._locate("upsert", ids, want_dup=True)
        m = int(t.numel())
        self._emb_arg("upsert", emb, m)
        fr, cnt, dp = self._key_read("upsert", [first, count.to(torch.int64), dup.to(torch.int64)], ws, status).reshape(3, m)
        self._no_repeats("upsert", dp)
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
        t16 = torch.empty((m, self.d), dtype=self._scan_dtype, device=self.device)
        tlo = None if self._slo is None else torch.empty_like(t16)
        self._store.write(self, src, t16, tlo, update=True)
        for buf, new in ((self._s32, src), (self._s16, t16), (self._slo, tlo)):
            if buf is not None:
                buf.index_copy_(0, rows, new)

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
            got = self._key_read(who, [total] + ([start, count.to(torch.int64), dup.to(torch.int64)] if host else []), ws, status,
                                 reserved_ok)
            tot = int(got[0])
            # the two lists of the fill lie behind what the count wrote: a larger buffer takes that part over
            ws = self._key_workspace(int(L.convdr_keys_rows_workspace_bytes(m, tot)), keep=need0)
            rows = torch.empty(tot, dtype=torch.int64, device=self.device)
            _lib.check(L.convdr_keys_rows_fill(ptr(self.ids), n, ptr(ws), ws.numel(), m, ptr(rows), tot, _lib.stream_ptr()),
                       "convdr_keys_rows_fill")
        return start, count, rows, (got[1:].reshape(3, m) if host else None)

    def rows_all(self, ids):
        """ALL rows of the listed ids (int64 vector, numpy or torch, host or device; repeats allowed): device (start int64 [m],
        count int32 [m], rows int64 [total]).  The rows that carry ids[j] are rows[start[j] : start[j] + count[j]], ascending;
        an id on no row has count 0; a repeated id shares the segment of its first occurrence, so total = the rows of the
        DISTINCT listed ids.  The same bits in every run.  One host read (total, to size `rows`, and the status words; a
        device list that holds the reserved id INT64_MIN raises ValueError there, as for remove_ids)."""
        self._need_ids("rows_all")
        return self._rows_csr("rows_all", self._id_list("rows_all", ids))[:3]

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
            ws = self._key_workspace(need)
            ord_ = torch.empty(n, dtype=torch.int32, device=self.device)
            nd = torch.empty(1, dtype=torch.int64, device=self.device)
            _lib.check(L.convdr_doc_ordinals(ptr(self.ids), n, ptr(ws), ws.numel(), ptr(ord_), ptr(nd), _lib.stream_ptr()),
                       "convdr_doc_ordinals")
            ndocs = int(self._key_read("doc_ordinals", [nd], ws)[0])
        return DocOrdinals(ord_, ndocs, n)

    # -- per-query exclusions: the rows each query of a call leaves out (include/convdr_hip.h, "Per-query exclusions") ----------
    def exclude_rows(self, rows):
        """A QueryExclusions from row numbers: rows int64 [nq, e] (numpy or torch, host or device; any order, repeats allowed,
        negative = padding) or a host list of nq integer sequences of different lengths (``pack_exclusions``).  At most 16,384
        entries per query.  Sorted and de-duplicated per query on the device (convdr_excl_build_rows); ONE host read (the
        counts and the status word).  A host row id >= ntotal raises ValueError before anything is launched, a device one
        after that read.  Pass it to ``excluding``; valid while ntotal stays what it was."""
        return self._exclusions(rows, int(rows.shape[0]) if hasattr(rows, "shape") else len(rows))

    def exclude_ids(self, ids):
        """A QueryExclusions from document ids: ids int64 [nq, m] (numpy or torch, host or device; INT64_MIN = padding); query j
        excludes EVERY row of every document it lists -- resolved on the device through the CSR of ``rows_all`` and
        convdr_excl_build_docs --, an id on no row excludes nothing.  Needs an id column.  Two host reads: the CSR's size, then
        the counts and the status word -- more than 16,384 rows for one query raise ValueError there."""
        import torch
        self._need_ids("exclude_ids")
        it = torch.as_tensor(np.array(ids) if isinstance(ids, np.ndarray) and not ids.flags.writeable else ids)
        if it.dim() != 2 or it.dtype != torch.int64:
            raise ValueError("exclude_ids: ids must be int64 [nq, m] (got %s, shape %s)" % (it.dtype, tuple(it.shape)))
        nq, m = int(it.shape[0]), int(it.shape[1])
        if m > EXCLUDE_MAX:
            raise ValueError("exclude_ids: %d ids per query, at most %d entries" % (m, EXCLUDE_MAX))
        if not nq or not m:
            return self._exclude_build("exclude_ids", nq, 4, None)
        start, count, rows, _ = self._rows_csr("exclude_ids", it.to(self.device).reshape(-1).contiguous(), reserved_ok=True)
        tot, L, ptr = int(rows.numel()), _lib.lib(), _lib.ptr
        return self._exclude_build("exclude_ids", nq, min(EXCLUDE_MAX, tot), lambda ex, ld, cnt, st: _lib.check(
            L.convdr_excl_build_docs(ptr(rows), tot, ptr(start), ptr(count), nq, m, m, self.ntotal, ptr(ex), ld, ptr(cnt), ptr(st),
                                     _lib.stream_ptr()), "convdr_excl_build_docs"))

    def _exclude_build(self, who, nq, width, launch):
        """The build's outputs, its launch (None: every list is empty) and its ONE host read -> QueryExclusions"""
        import torch
        ld = max(4, (int(width) + 3) // 4 * 4)
        ex = torch.full((nq, ld), -1, dtype=torch.int32, device=self.device)          # (0xffffffff: the padding)
        out = torch.zeros(nq + 1, dtype=torch.int32, device=self.device)             # counts | status
        if launch is None or not nq:
            return QueryExclusions(ex, out[:nq], np.zeros(nq, np.int64), self.ntotal)
        with torch.cuda.device(self.device):
            launch(ex, ld, out[:nq], out[nq:])
        host = out.cpu().numpy()
        if host[nq] & EXCL_ST_LONG:
            raise ValueError("%s: a query excludes more than %d rows (repeats counted)" % (who, EXCLUDE_MAX))
        if host[nq] & EXCL_ST_ROW:
            raise ValueError("%s: a row id >= ntotal = %d" % (who, self.ntotal))
        used = max(4, (int(host[:nq].max()) + 3) // 4 * 4)
        return QueryExclusions(ex if used == ld else ex[:, :used].contiguous(), out[:nq], host[:nq], self.ntotal)

    def _exclusions(self, exclude, nq):
        """the exclusions of a call with nq queries -> None or a QueryExclusions that fits this index and those queries; a raw
        [nq, e] array or a list of lists is built for the call"""
        import torch
        if exclude is None:
            return None
        if isinstance(exclude, QueryExclusions):
            if exclude.n != self.ntotal or exclude.rows.device != self.device:
                raise ValueError("stale QueryExclusions: built for ntotal = %d on %s, the index holds %d rows on %s"
                                 % (exclude.n, exclude.rows.device, self.ntotal, self.device))
            if exclude.nq != nq:
                raise ValueError("exclude: built for %d queries, the call has %d" % (exclude.nq, nq))
            return exclude
        arr = pack_exclusions(exclude, nq)
        if isinstance(arr, np.ndarray):
            if arr.size and int(arr.max()) >= self.ntotal:
                raise ValueError("exclude: row id %d >= ntotal = %d" % (int(arr.max()), self.ntotal))
            arr = torch.as_tensor(arr)
        elif arr.device.type == "cpu" and arr.numel() and int(arr.max()) >= self.ntotal:
            raise ValueError("exclude: row id %d >= ntotal = %d" % (int(arr.max()), self.ntotal))
        t, e = arr.to(self.device).contiguous(), int(arr.shape[1])
        if not e:
            return self._exclude_build("exclude_rows", nq, 4, None)
        L, ptr = _lib.lib(), _lib.ptr
        return self._exclude_build("exclude_rows", nq, e, lambda ex, ld, cnt, st: _lib.check(
            L.convdr_excl_build_rows(ptr(t), nq, e, e, self.ntotal, ptr(ex), ld, ptr(cnt), ptr(st), _lib.stream_ptr()),
            "convdr_excl_build_rows"))

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
        self._store.refuse(self, "upsert_docs")
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
        self._emb_arg("upsert_docs", emb, int(cn.sum()))
        if not m:
            return 0, 0, 0
        _, _, rows, (st, cur, dp) = self._rows_csr("upsert_docs", t, host=True)
        self._no_repeats("upsert_docs", dp)

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
        r = self._store.widen(self, r)
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

    # -- snapshots (FAISS write_index / read_index): one verified file, snapshot.py; the digest is convdr_digest_rows --------
    # What is written: the re-score rows at the resident width, the id column, the centre, and in the header the scale, the max
    # norm's bits and the x3_first flag.  The scan copy and the remainder copy are a pure function of (row, centre, scale) and
    # are rebuilt by load as add builds them; RowFilter / DocOrdinals are derived and stale across a save / load.
    def _sections(self):
        """[(name, device tensor of the used rows or None, rows, row_bytes)] of what a snapshot holds, in file order"""
        secs = [("rows", self._rows, self._n, self.d * self._store.esize)]
        if self._sid is not None:
            secs.append(("ids", self.ids, self._n, 8))
        secs += [(name, getattr(self, "_" + name), 1, self.d * 4) for name in self._store.vectors if getattr(self, "_" + name) is not None]
        return secs

    def _digest_into(self, t, rows, row_bytes, word0, window_rows, out):
        """convdr_digest_rows of the first `rows` rows of `t` into out int64 [windows, 2] (the bytes of uint64); enqueued"""
        if rows:
            _lib.check(_lib.lib().convdr_digest_rows(_lib.ptr(t), int(rows), int(row_bytes), int(word0), int(window_rows), _lib.ptr(out),
                                                     _lib.stream_ptr()), "convdr_digest_rows")

    def _digest_sections(self, secs, window_rows, word0_rows=0):
        """One launch per section, every section's windows in ONE device tensor int64 [total + 1, 2] whose last row holds the
        max norm's bits, so that one host read fetches everything: -> (tensor, {name: (first window, end window)})"""
        import torch
        spans, at = {}, 0
        for name, _t, rows, _rb in secs:
            c = (rows + window_rows - 1) // window_rows
            spans[name] = (at, at + c)
            at += c
        dg = torch.zeros((at + 1, 2), dtype=torch.int64, device=self.device)
        for name, t, rows, rb in secs:
            w0 = 0 if name in ("centre", "step") else word0_rows * (rb // 8)
            self._digest_into(t, rows, rb, w0, window_rows, dg[spans[name][0]:spans[name][1]])
        dg[at, :1].copy_(self._max_norm.view(torch.int32))
        return dg, spans

    @staticmethod
    def _digest_read(dg, spans):
        """THE host read: ({name: [(A, B)]}, max-norm bits)"""
        host = dg.cpu().numpy().astype(np.uint64)
        return ({name: [(int(host[j, 0]), int(host[j, 1])) for j in range(a, b)] for name, (a, b) in spans.items()},
                int(host[-1, 0]) & 0xffffffff)

    def fingerprint(self):
        """What this index holds, as a small dict that is equal for equal content whatever sequence of add / reserve / removal
        produced it: d_in, storage, precision, center, n, the scale's and the max norm's fp32 bits (hex), and ONE digest
        (A, B) each of the re-score rows, the id column and the centre (None where the index has none) -- convdr_digest_rows
        over the resident buffers, word0 = 0, one window; no host copy of the rows, one host read.  Not cryptographic."""
        import struct
        import torch
        with torch.cuda.device(self.device):
            dg, spans = self._digest_sections(self._sections(), max(1, self._n))
            got, mn = self._digest_read(dg, spans)
        fp = {"d_in": self.d_in, "storage": self.storage, "precision": self.precision, "center": self.center, "n": self._n,
              "scale": "%08x" % struct.unpack("<I", struct.pack("<f", float(self._scale)))[0], "max_norm": "%08x" % mn}
        for name in ("rows", "ids") + self._store.vectors:
            fp[name] = None if name not in got else (got[name][0] if got[name] else (0, 0))
        fp.update({key: getattr(self, attr) for key, attr in self._store.counters})
        return fp

    def _stage_bytes(self, total):
        """the pinned staging buffers as flat byte views (torch, numpy), their events, the chunk size in bytes, the copy stream"""
        import torch
        per32 = max(1, int(self.host_chunk_bytes) // (4 * self.d))
        nbuf = max(2, int(self.host_stage_buffers))
        stage, freed = _staging(self.device, min(per32, (int(total) + 4 * self.d - 1) // (4 * self.d)), self.d, nbuf)
        flat = [b.view(torch.uint8).view(-1) for b in stage]
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        return flat, [f.numpy() for f in flat], freed, per32 * self.d * 4, self._copy_stream

    def _copy_threads(self):
        avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        return max(1, min(int(self.host_copy_threads), avail))

    def _save_bytes(self, t, fd, offset):
        """Device tensor `t` (contiguous) -> the file, bytes [offset, offset + t.nbytes): the mirror image of _stream_rows.  D2H
        copies of host_chunk_bytes on the copy stream into the pinned staging buffers, host_stage_buffers - 1 of them in flight;
        the pool's threads os.pwrite slices of a landed chunk while the next chunks cross PCIe.  A buffer is reused only after
        its D2H has completed AND its file writes have returned; on return every write has returned and every freed[bi] is a
        recorded event (the rule beside the events in _stream_rows)."""
        import torch
        from .snapshot import _pwrite_all
        if t is None or not t.numel():
            return
        src = t.reshape(-1).view(torch.uint8)
        total = int(src.numel())
        flat, flat_np, freed, cap, cs = self._stage_bytes(total)
        nbuf, threads = len(flat), self._copy_threads()
        pool = _copy_pool(threads * (nbuf - 1), self.device)
        cs.wait_stream(torch.cuda.current_stream())         # (the rows are what the main stream has made of them so far)
        chunks = [(s, min(total, s + cap)) for s in range(0, total, cap)]
        events, writes = {}, {}

        def land(ci):
            """chunk ci has crossed PCIe: its file writes, `threads` slices on the pool"""
            s, e = chunks[ci]
            events.pop(ci).synchronize()
            buf = flat_np[ci % nbuf]
            step = ((e - s + threads - 1) // threads + 4095) // 4096 * 4096
            writes[ci] = [pool.submit(_pwrite_all, fd, buf[a:min(e - s, a + step)], offset + s + a) for a in range(0, e - s, step)]

        def written(ci):
            for f in writes.pop(ci):
                f.result()
        try:
            for ci, (s, e) in enumerate(chunks):
                bi = ci % nbuf
                if ci >= nbuf:
                    written(ci - nbuf)                      # (the buffer's last file writes have returned)
                elif freed[bi] is not None:
                    cs.wait_event(freed[bi])                # (an earlier add's H2D copy may still be reading the buffer)
                with torch.cuda.stream(cs):
                    flat[bi][:e - s].copy_(src[s:e], non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(cs)
                freed[bi] = events[ci] = ev
                if ci >= nbuf - 1:
                    land(ci - (nbuf - 1))
            for ci in range(max(0, len(chunks) - (nbuf - 1)), len(chunks)):
                land(ci)
        finally:
            for ev in events.values():                      # (after an error, too: no copy in flight, no thread in a buffer)
                ev.synchronize()
            err = None
            for ci in sorted(writes):
                for f in writes[ci]:
                    try:
                        f.result()
                    except BaseException as e:              # noqa: PERF203
                        err = err or e
            writes.clear()
        if err is not None:
            raise err

    def _load_bytes(self, fd, offset, dst):
        """the file's bytes [offset, offset + dst.nbytes) -> the device tensor `dst` (contiguous) through the staging buffers,
        one chunk after the other (the id column: 8 bytes per row beside the rows' 1.5 - 3 KB)"""
        import torch
        from .snapshot import pread_into
        flat_dst = dst.reshape(-1).view(torch.uint8)
        total = int(flat_dst.numel())
        if not total:
            return
        flat, flat_np, freed, cap, cs = self._stage_bytes(total)
        main = torch.cuda.current_stream()
        cs.wait_stream(main)
        for ci, s in enumerate(range(0, total, cap)):
            e, bi = min(total, s + cap), ci % len(flat)
            if freed[bi] is not None:
                freed[bi].synchronize()
            pread_into(fd, memoryview(flat_np[bi][:e - s]), offset + s)
            with torch.cuda.stream(cs):
                flat_dst[s:e].copy_(flat[bi][:e - s], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(cs)
            freed[bi] = ev
            main.wait_event(ev)

    def save(self, path, window_rows=65536):
        """FAISS ``write_index``: the index as ONE verified snapshot file (snapshot.py; layout in include/convdr_hip.h).  Per
        section -- rows, ids, centre -- one convdr_digest_rows launch over the used rows gives the per-window digests the
        header stores (windows of `window_rows` rows), then the bytes go D2H through the process-wide pinned staging buffers
        and to the file with positioned writes (_save_bytes).  One host read (the digests and the max norm's bits).  The file
        is written to path + ".tmp" and renamed: a failed save leaves an existing snapshot untouched.  Returns when the file
        is in place.  ``stats``: save_bytes (the file's size), save_s, save_fsync_s (the share of save_s spent in fsync)."""
        import struct
        import time
        import torch
        from . import snapshot
        t0 = time.perf_counter()
        w = int(window_rows)
        if w < 1:
            raise ValueError("save: window_rows must be >= 1 (got %d)" % w)
        secs = self._sections()
        meta = {"d_in": self.d_in, "d": self.d, "storage": self.storage, "precision": self.precision, "center": self.center,
                "n": self._n, "scale": "%08x" % struct.unpack("<I", struct.pack("<f", float(self._scale)))[0], "max_norm": "0" * 8,
                "x3_first": bool(self._x3_first), "has_ids": self._sid is not None, "window_rows": w}
        # (the 8-bit store: max_norm holds the largest row L1 norm of the codes, and the saturation count rides along)
        meta.update({key: int(getattr(self, attr)) for key, attr in self._store.counters})
        timings = {}
        with torch.cuda.device(self.device):
            dg, spans = self._digest_sections(secs, w)

            def finish():
                got, mn = self._digest_read(dg, spans)
                meta["max_norm"] = "%08x" % mn              # (fixed width: the JSON's length was known before)
                return got
            size = snapshot.write_snapshot(path, meta, [(name, rows * rb, rb, functools.partial(self._save_section, t))
                                                        for name, t, rows, rb in secs], finish, timings)
        self.stats["save_bytes"], self.stats["save_s"], self.stats["save_fsync_s"] = size, time.perf_counter() - t0, timings["fsync_s"]

    def _save_section(self, t, fd, offset):
        self._save_bytes(t, fd, offset)
        return None                                         # (the digests come with finish(): one host read for all sections)

    @classmethod
    def load(cls, path, device=None, rows=None, reserve=None, verify=True, precision=None, cap=4096, rank_target=0, prepin=True,
             chunk_bytes=None):
        """FAISS ``read_index``: the index a snapshot file holds (``save``).  Constructed from the header; the centre, the scale,
        the max norm's bits and the x3_first flag are the saved ones (never re-derived from the rows); storage for
        max(n, reserve) rows (``reserve`` given: kept as a reservation, as by reserve()); the rows stream from the file with
        positioned reads through the staging buffers exactly as add(BlockView) streams a block -- the fp32 store makes its scan
        copy per chunk (convdr_ip_prepare_block*), the half store's halves land in the store and no kernel runs --, then the ids.
        verify: one convdr_digest_rows launch per section over what landed in HBM, compared with the header's per-window digests
        in ONE host read at the end; a mismatch raises ConvdrError naming the section and the window, and no index is returned.
        precision: overrides the saved one (the fp32 store: any of its precisions, the scale re-derived from the saved max norm
        when the scan kind changes, as _rebuild_scaled does; the half store: its own three).
        rows=(r0, r1): that slice only -- one rank's share of a shared snapshot; r0 a multiple of the file's window_rows, r1 a
        multiple of it or n (else ValueError); only the covered windows are verified; centre, scale and max norm stay the whole
        snapshot's (an upper bound is all the certificate needs, as after remove_rows).
        chunk_bytes: the staging chunk (default host_chunk_bytes).  ``stats``: load_bytes, load_s."""
        import struct
        import time
        import torch
        from . import snapshot
        t0 = time.perf_counter()
        h = snapshot.read_header(path)
        n_file, w, secs = int(h["n"]), int(h["window_rows"]), h["sections"]
        r0, r1 = (0, n_file) if rows is None else (int(rows[0]), int(rows[1]))
        if not (0 <= r0 <= r1 <= n_file) or r0 % w or (r1 % w and r1 != n_file):
            raise ValueError("load: rows=(%d, %d) must lie in [0, n = %d], r0 a multiple of the file's window_rows = %d and r1 a "
                             "multiple of it or n" % (r0, r1, n_file, w))
        store = STORES[h["storage"]]
        precision = h["precision"] if precision is None else precision
        if precision not in store.precisions:
            raise ValueError("load: precision %r is none of the %s store's" % (precision, h["storage"]))
        idx = cls(int(h["d_in"]), device=device, cap=cap, rank_target=rank_target, precision=precision,
                  center=None if store.centred is not None else bool(h["center"]), prepin=prepin, storage=h["storage"])
        n, rb = r1 - r0, idx.d * store.esize
        want = {"rows": (n_file * rb, rb)}
        if h["has_ids"]:
            want["ids"] = (n_file * 8, 8)
        for name in store.vectors:      # (the centre of an index that has one; the vectors behind it whenever there are rows)
            if name in secs if name == "centre" else n_file:
                want[name] = (idx.d * 4, idx.d * 4)
        for name, (nbytes, rbytes) in want.items():
            if name not in secs or (secs[name]["bytes"], secs[name]["row_bytes"]) != (nbytes, rbytes) or int(h["d"]) != idx.d:
                raise _lib.ConvdrError("load %s: section %r does not have the %d bytes of %d-byte rows the header's n, d and storage "
                                       "imply" % (path, name, nbytes, rbytes))
        if chunk_bytes is not None:
            idx.host_chunk_bytes = int(chunk_bytes)
        L = _lib.lib()
        mn_bits = int(h["max_norm"], 16)
        scale = struct.unpack("<f", struct.pack("<I", int(h["scale"], 16)))[0]
        if idx.kind != (store.kind or _KINDS[h["precision"]]):
            # another scan kind: the scale that fits the saved max norm, as _rebuild_scaled derives it (bf16 has none)
            scale = float(L.convdr_ip_f16_scale(struct.unpack("<f", struct.pack("<I", mn_bits))[0])) if idx.kind == "f16" else 1.0
        fd = os.open(path, os.O_RDONLY)
        try:
            with torch.cuda.device(idx.device):
                for name in store.vectors:
                    if name in secs:
                        c = np.empty(idx.d, dtype=np.float32)
                        snapshot.pread_into(fd, memoryview(c).cast("B"), secs[name]["offset"])
                        setattr(idx, "_" + name, torch.from_numpy(c).to(idx.device))
                for key, attr in (store.counters if store.vectors[-1] in secs else ()):     # (they travel with the last vector)
                    setattr(idx, attr, int(h.get(key, 0)))
                    idx.stats[key] = getattr(idx, attr)
                idx._scale, idx._x3_first = scale, bool(h["x3_first"])
                # (copy_ INTO the tensor: the half store's max norm is a view of its (norm, flags) triple and must stay one)
                idx._max_norm.copy_(torch.tensor([mn_bits - (1 << 32) if mn_bits >> 31 else mn_bits], dtype=torch.int32).view(torch.float32))
                room = max(n, int(reserve or 0))
                if room:
                    idx.reserve(room)
                    idx._reserved = reserve is not None
                if n:
                    src = snapshot.FileRows(fd, secs["rows"]["offset"], rb, r0, n, idx.d)
                    # (never the store's `first`: centre and scale are the saved ones; rows that are the store land in it and no
                    #  kernel runs)
                    dst = tuple(None if b is None else b[:n] for b in (idx._s32, idx._s16, idx._slo))
                    each = (lambda ci, s, e: None) if dst[0] is None else (
                        lambda ci, s, e: idx._prepare_into(*(None if b is None else b[s:e] for b in dst)))
                    idx._stream_rows(src, dst[1] if dst[0] is None else dst[0], src.read_rows_into, idx.host_chunk_bytes, each, t0)
                idx._n = n
                if h["has_ids"]:
                    idx._sid, idx._sid_spare = torch.empty(max(room, 0), dtype=torch.int64, device=idx.device), None
                    idx._load_bytes(fd, secs["ids"]["offset"] + r0 * 8, idx._sid[:n])
                if verify:
                    dg, spans = idx._digest_sections(idx._sections(), w, word0_rows=r0)
                    got, _ = idx._digest_read(dg, spans)
                    for name in sorted(got):
                        first = 0 if name in ("centre", "step") else r0 // w
                        for j, pair in enumerate(got[name]):
                            if pair != secs[name]["digests"][first + j]:
                                raise _lib.ConvdrError("load %s: section %r, window %d: what landed on the device has digest %016x %016x, "
                                                       "the header says %016x %016x; no index is returned"
                                                       % ((path, name, first + j) + pair + secs[name]["digests"][first + j]))
                else:
                    torch.cuda.current_stream().synchronize()       # (the call returns when the index is in place)
        finally:
            os.close(fd)
        idx.stats["load_bytes"] = sum(secs[name]["bytes"] if name in ("centre", "step") else n * want[name][1] for name in want)
        idx.stats["load_s"] = time.perf_counter() - t0
        return idx
