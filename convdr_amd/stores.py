"""What FlatIPIndex asks about its storage: one description per ``storage`` string, looked up in STORES.  A description is
data plus a few functions that take the index as their first argument; it has no state and no back-pointer -- every per-index
field stays on the index (index_store.py), which keeps ``self._store = STORES[storage]`` and asks it instead of testing flags."""
import numpy as np

from . import _lib

_KINDS = {"auto": "f16", "fp16": "f16", "fp16x3": "f16", "bf16": "bf16", "bf16x3": "bf16", "fp16x2": "f16", "i8": "i8"}
_HALF_PRECISIONS = ("auto", "fp16", "fp16x2")    # the rungs of a half store (storage="fp16")
SQ8_MAX_D = 1024                                 # csrc/ip_topk.hip: IP_Q8_MAX_D (the int32 range of the integer scan)
HALF_NORM_LIMIT = 60000.0                        # csrc/ip_topk.hip: IP_F16_NORM_LIMIT
# CONVDR_IP_RANGE from a scan that has no scale to rebuild: no threshold and no retry changes the verdict, every entry ends with this
_BF16_RANGE = ("CONVDR_IP_RANGE from the bf16 scan: a query or the block has a non-zero norm below 2^-60, where bf16 operands "
               "and their products are subnormal and the scan's error bound does not hold; use precision=\"auto\" or "
               "\"fp16\", whose scan rescales both operands")
_SQ8_RANGE = ("CONVDR_IP_RANGE from the 8-bit store's scan: a query holds a value that is not finite, or its largest |q_j step_j| "
              "is non-zero and below 2^-100, where the integer query operand has no relative precision")


class Store:
    """One storage: data, and functions that take the index first.  Constructor rules: `precisions`, `centred` (True / False:
    forced, None: the caller's choice, default on), `max_d`, `kstep` the width is padded to, `kind` of the scan (None: the
    precision's), `esize` bytes per element of the re-score rows.  State: `buffers` reserve() holds (`one_buffer`: corpus and scan
    operand at once), `words` beside the max norm in the (norm, word, word) triple ONE host read fetches, further `fields` reset()
    creates.  One add (_IndexStore._add_rows): the dtypes a host source may be streamed in (`streams`, the last one otherwise) and a device
    source may keep (`keeps`, fp32 otherwise), room, landing, first, write (rows -> scan copy / stored rows; update: by
    update_rows), verdict; `fixes`: what the first rows fix and a refused add puts back; `first_needs_all`: they fix it from ALL rows
    of the first add; `clock_growth`: add_host_s includes growing the storage.  Afterwards: rescale (None: never asked for), widen
    (stored rows -> fp32), `store_view`.  The C
    ABI: block, call.  The ladder: `split_key`, `second_rung`, `range_message`, search_stats.  Snapshots: the fp32 [d] `vectors`
    behind the ids, the (header key, attribute) `counters` that travel with the last of them.  `refused`: entries not offered."""

    def __init__(self, name, **kw):
        self.name, self.refused, self.max_d, self.kind, self.kstep, self.words, self.fields = name, frozenset(), None, None, 64, (), ()
        self.first_needs_all = self.clock_growth = False
        self.store_view, self.vectors, self.counters, self.range_message = None, ("centre",), (), _BF16_RANGE
        self.split_key, self.second_rung, self.search_stats = "x3_queries", True, (lambda ix, nq, n_bad: {})
        # (a streamed add: the storage grows, the rows land in the buffer of the re-score rows, nothing refuses them)
        self.room, self.verdict = (lambda ix, t, m: ix._grow_for(m)), (lambda ix, n0, state0, attempt: True)
        self.landing = lambda ix, t, dst, cb: (dst[1] if dst[0] is None else dst[0], int(t.shape[0]))
        self.__dict__.update(kw)
        self.one_buffer = "_s32" not in self.buffers

    def admit(self, precision, center, d):
        """The constructor's rules that need no device -> the centring flag; ValueError with the storage's text."""
        who = "FlatIPIndex(storage=%r)" % self.name
        if precision == "i8" and "i8" not in self.precisions:
            raise ValueError("%s: precision 'i8' belongs to storage='sq8'" % who)
        if self.one_buffer and precision not in self.precisions:       # (the fp32 store asserts, once it knows there is a GPU)
            raise ValueError("%s: precision must be one of %s (got %r)" % (who, self.precisions, precision))
        if self.centred is not None and center is not None and bool(center) != self.centred:
            raise ValueError("%s: the %s (center=%s)" % (who, "8-bit store is always centred" if self.centred else
                                                         "half store is not centred", bool(center)))
        if self.max_d and (int(d) + self.kstep - 1) // self.kstep * self.kstep > self.max_d:
            raise ValueError("%s: d = %d, at most %d" % (who, int(d), self.max_d))
        return bool(self.centred if self.centred is not None else (True if center is None else center))

    def refuse(self, ix, who):
        """ValueError for an entry this storage does not offer, before anything is launched (or any other attribute read)"""
        if who in self.refused:
            raise ValueError("FlatIPIndex(storage='sq8').%s: not offered by the 8-bit store (storage='sq8'); use storage='fp32' or "
                             "'fp16'" % who)

    def final_range(self, ix):
        """None where CONVDR_IP_RANGE is rebuilt away (a scan copy with a scale), else the message the entry ends with"""
        return None if ix.kind == "f16" else self.range_message

    @staticmethod
    def call(what, ops, plo=None, split=False):
        """(entry suffix, leading arguments, block arguments) of the C entry that scans ("search", "filtered") or re-scores
        ("score") the block `ops` (_IndexStore._operands), each store code with the operands its entry declares"""
        code, r32, r16, scale, centre = ops
        if code == 3:
            return "_q8", (), (r16, centre, scale)
        if what == "score":
            return "", (code,), (r32, r16, scale)
        rlo, split = (None, int(bool(split))) if code == 2 else (_lib.ptr(plo), 0)
        if what == "filtered":
            return "", (code,), (r32, r16, rlo, scale, split)
        return (("", (), (r32, r16, rlo)), ("_f16", (), (r32, r16, rlo, scale)), ("_h16", (), (r16, scale, split)))[code]


# -- storage="fp32": fp32 block, 16-bit scan copy, optional remainder copy ------------------------------------------------------
def _fp32_room(ix, t, m):
    want_lo = ix.precision in ("bf16x3", "fp16x3") or ix._slo is not None
    if ix._s32 is None and not want_lo and not isinstance(t, np.ndarray):
        # first block of an unreserved index: adopt the caller's device tensor instead of copying it
        ix._s32, ix._s16 = t, t.new_empty((m, ix.d), dtype=ix._scan_dtype)
        return ix._s32, ix._s16, None
    return ix._grow_for(m, want_lo)


def _fp32_rescale(ix):
    """re-derive the scale from the block's max norm and rebuild the fp16 copies from the resident fp32 rows"""
    ix._scale = float(_lib.lib().convdr_ip_f16_scale(float(ix._max_norm.item())))
    if ix._n:
        ix._prepare_into(ix._p32, ix._pbf, ix._plo)


# -- storage="fp16": the half store -----------------------------------------------------------------------------------------------
def _half_verdict(ix, n0, state0, attempt):
    """keep, refuse, or -- a scaled value overflowed -- lower the scale and have the new rows written once more"""
    got = ix._mf[:2].cpu()                                          # the one host read of this add()
    mn, fl = float(got[0]), int(got.view(ix._flags.dtype)[1])
    ix._flags.zero_()
    if (fl & 1) or not mn <= HALF_NORM_LIMIT:
        ix._restore(state0)
        raise _lib.ConvdrError("FlatIPIndex(storage='fp16').add: %s; the index is unchanged (%d rows)"
                               % ("a value is not finite as a half" if fl & 1 else "a row's norm %g exceeds %g" % (mn, HALF_NORM_LIMIT), n0))
    if fl & 2:
        if attempt:
            raise _lib.ConvdrError("half store: scaled values overflow at scale %g, max norm %g" % (ix._scale, mn))
        ix._rebuild_scaled()                # the scale that fits the new max norm; rows [0, n0) rescaled in place
    return not (fl & 2)


def _half_rescale(ix):
    """the half store is rescaled IN PLACE by 2^(s_new - s_old) <= 1, s_new >= 0: exact (convdr_ip_store_rows_f16)"""
    new = max(1.0, float(_lib.lib().convdr_ip_f16_scale(float(ix._max_norm.item()))))
    if ix._n and new != ix._scale:
        ix._store_rows(ix._pbf, ix._pbf, new / ix._scale, fold_norm=False)
        if int(ix._flags.item()):
            raise _lib.ConvdrError("half store: the in-place rescale %g -> %g was not exact" % (ix._scale, new))
    ix._scale = new


# -- storage="sq8": the 8-bit store --------------------------------------------------------------------------------------------------
def _sq8_landing(ix, t, dst, chunk_bytes):
    # (None: a bounce buffer) of the staging ring's size: the copy stream waits for the main stream at the start of every window
    # (_stream_rows), i.e. for the quantisation of the window before, so ONE bounce buffer serves them all
    return None, max(1, int(chunk_bytes) // (4 * ix.d)) * 4 // t.dtype.itemsize * max(2, int(ix.host_stage_buffers))


def _sq8_first(ix, rows):
    """centre = the column mean, step = the largest column deviation / 127, of ALL rows of the first add (widened, exactly)"""
    rows = rows.float()
    ix._set_centre(rows)
    ix._step = ix._centre.new_empty(ix.d)
    ix._column_pass("convdr_ip_column_absdev", rows, (_lib.ptr(ix._centre),), ix._step)
    return rows


def _sq8_write(ix, rows, codes, tlo, update=False):
    ptr, rows = _lib.ptr, rows.float()
    _lib.check(_lib.lib().convdr_ip_store_rows_q8(ptr(rows), int(rows.shape[0]), ix.d, ptr(ix._centre), ptr(ix._step), ptr(codes),
                                                  ptr(ix._max_norm), ptr(ix._flags), ptr(ix._sat), _lib.stream_ptr()),
               "convdr_ip_store_rows_q8")


def _sq8_verdict(ix, n0, state0, attempt):
    """a value that is not finite refuses the add and leaves the index exactly as it was (the codes it wrote lie behind ntotal)"""
    got = ix._mf[1:].view(ix._flags.dtype).cpu()                     # the one host read of this add()
    fl, sat = int(got[0]), int(got[1]) & 0xffffffff
    ix._mf[1:].zero_()
    if fl & 1:
        ix._restore(state0)
        raise _lib.ConvdrError("FlatIPIndex(storage='sq8').add: a value is not finite; the index is unchanged (%d rows)" % n0)
    ix._saturated += sat
    ix.stats["sq8_saturated"] = ix._saturated
    return True


STORES = {s.name: s for s in (
    Store("fp32", precisions=("auto", "fp16", "fp16x3", "bf16", "bf16x3"), centred=None, esize=4, buffers=("_s32", "_s16", "_slo"),
          fixes=("_centre", "_scale"), clock_growth=True, streams=("float32",), keeps=("float32",), room=_fp32_room,
          first=lambda ix, rows: ix._first_rows(rows), write=lambda ix, src, t16, tlo, update=False: ix._prepare_into(src, t16, tlo),
          rescale=_fp32_rescale, widen=lambda ix, r: r,
          block=lambda ix, p32, p16: (int(ix.kind == "f16"), _lib.ptr(p32), _lib.ptr(p16), float(ix._scale) if ix.kind == "f16" else 1.0,
                                      _lib.ptr(ix._centre))),       # (the bf16 copy has no scale)
    Store("fp16", precisions=_HALF_PRECISIONS, centred=False, esize=2, buffers=("_s16",), fixes=("_scale",),
          # max norm, the flag word of convdr_ip_store_rows_f16 and update_rows' own flag word (update_flags()) side by side
          words=("_flags", "_uflags"), store_view="_pbf", split_key="x2_queries", streams=("float16",), keeps=("float16", "float32"),
          first=lambda ix, rows: ix._half_first_scale(rows), verdict=_half_verdict, rescale=_half_rescale,
          write=lambda ix, src, t16, tlo, update=False: ix._store_rows(src, t16, ix._scale, flags=ix._uflags if update else None),
          block=lambda ix, p32, p16: (2, None, _lib.ptr(p16), float(ix._scale), None),
          widen=lambda ix, r: r.float() * (1.0 / float(ix._scale))),        # (a power of two: exact)
    Store("sq8", precisions=("auto", "i8"), centred=True, max_d=SQ8_MAX_D, kstep=128, kind="i8", esize=1, buffers=("_s16",),
          # the largest row L1 norm of the codes (in the max norm's role), the flag word and the saturation count of
          # convdr_ip_store_rows_q8 side by side
          words=("_flags", "_sat"), fields=(("_step", None), ("_saturated", 0)), fixes=("_centre", "_step"), first_needs_all=True,
          second_rung=False, range_message=_SQ8_RANGE, vectors=("centre", "step"), counters=(("sq8_saturated", "_saturated"),),
          refused=frozenset(("range_search", "range_search_tensors", "range_count", "rank_rows", "rank_rows_tensors", "rank_ids",
                             "rank_ids_tensors", "excluding", "score_ids", "score_ids_tensors", "search_docs", "search_distinct",
                             "update_rows", "upsert", "upsert_docs")),      # (README, "8-bit passage store")
          streams=("float16", "float32"), keeps=("float32", "float16"),     # (fp16 rows are widened, exactly)
          landing=_sq8_landing, first=_sq8_first, write=_sq8_write, verdict=_sq8_verdict,
          rescale=None,     # (its CONVDR_IP_RANGE is final: final_range)
          block=lambda ix, p32, p16: (3, None, _lib.ptr(p16), _lib.ptr(ix._step), _lib.ptr(ix._centre)),
          # v = fl(centre + fl(step c)): two torch ops, each rounded to fp32 (nothing fuses them)
          widen=lambda ix, r: ix._centre[:ix.d_in] + ix._step[:ix.d_in] * r.float(),
          # queries the first integer pass certified; the values later adds saturated
          search_stats=lambda ix, nq, n_bad: {"sq8_first_pass": nq - int(n_bad), "sq8_saturated": ix._saturated}))}
SQ8_REFUSED = tuple(sorted(STORES["sq8"].refused))      # entries the 8-bit store does not offer
