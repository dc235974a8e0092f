"""The snapshot file of a FlatIPIndex (FlatIPIndex.save / load): ONE file, little-endian, every byte of it covered by a digest
stored in its header, so that what lands -- on disk after a save, in HBM after a load -- can be checked where it lands.
Pure host code; reading a header needs neither torch nor the library (layout: include/convdr_hip.h, "Digest and snapshot file").

  bytes 0-63   magic "CONVDRIX" | u32 version = 1 | u32 0 | u64 JSON length | u64 A, u64 B: the digest of the JSON bytes zero
               padded to a multiple of 8, word0 = 0 | zero fill
  from 64      the JSON: d_in, d, storage, precision, center, n, scale and max_norm (fp32 bit patterns, 8 hex digits), x3_first,
               has_ids, window_rows, and "sections": {name: {offset, bytes, row_bytes, digests}} -- digests one [A, B] per window
               of window_rows rows, 16 hex digits each, the window's first word at word0 = (its first row) x row_bytes / 8
  sections     each at a 4,096-byte aligned offset: "rows" n x d of the re-score rows at the resident width, "ids" n x 8,
               "centre" ONE row of d x 4 bytes (one window)

The digest (csrc/ip_digest.hpp) is position-dependent and additive; it is NOT cryptographic."""
import json
import os
import struct
import time

import numpy as np

from ._lib import ConvdrError

MAGIC = b"CONVDRIX"
VERSION = 1
HEADER_BYTES = 64
SECTION_ALIGN = 4096
_HEAD = struct.Struct("<8sIIQQQ")             # magic, version, zero, JSON length, A, B: 40 bytes, the rest of the 64 is zero
K1, K2 = 0x9e3779b97f4a7c15, 0xd6e8feb86659fd93
_M64 = (1 << 64) - 1


def _mix(x):
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xbf58476d1ce4e5b9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def digest_bytes(data, word0=0):
    """(A, B) of `data` (bytes, zero padded to a multiple of 8 here) in numpy: the header's own digest, so that a header can be
    read without the library.  Sections go through convdr_digest_host (digest_host)."""
    data = bytes(data)
    data += b"\0" * (-len(data) % 8)
    w = np.frombuffer(data, dtype="<u8").astype(np.uint64)
    if not w.size:
        return 0, 0
    with np.errstate(over="ignore"):
        g = np.arange(1, w.size + 1, dtype=np.uint64) + np.uint64(word0 & _M64)
        a = _mix(w ^ (g * np.uint64(K1))).sum(dtype=np.uint64)
        b = _mix(((w << np.uint64(29)) | (w >> np.uint64(35))) ^ (g * np.uint64(K2))).sum(dtype=np.uint64)
    return int(a), int(b)


def digest_host(buf, word0=0):
    """(A, B) of a C-contiguous buffer (numpy array, bytes, memoryview) of a multiple of 8 bytes: convdr_digest_host.  ctypes
    releases the GIL for the call, so a thread pool spreads a file over cores."""
    import ctypes
    from . import _lib
    a = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf
    out = (ctypes.c_uint64 * 2)()
    _lib.check(_lib.lib().convdr_digest_host(ctypes.c_void_p(a.ctypes.data if a.size else 0), a.nbytes, word0 & _M64, out),
               "convdr_digest_host")
    return int(out[0]), int(out[1])


def _windows(sec, window_rows):
    """[(first byte, end byte, word0)] of the windows of a section"""
    rb, total = int(sec["row_bytes"]), int(sec["bytes"])
    step = int(window_rows) * rb
    return [(a, min(total, a + step), a // 8) for a in range(0, total, step)]


def _render(meta, table):
    return json.dumps(dict(meta, sections=table), sort_keys=True).encode()


def _layout(meta, sections, window_rows):
    """The section table with zero digests and every offset fixed: the JSON's length does not depend on the digests (fixed-width
    hex), so the offsets are known before a byte is produced."""
    table = {}
    for name, nbytes, row_bytes in sections:
        table[name] = {"offset": 0, "bytes": int(nbytes), "row_bytes": int(row_bytes), "digests": []}
        table[name]["digests"] = [["0" * 16] * 2 for _ in _windows(table[name], window_rows)]
    for _ in range(8):                         # (an offset's digit count feeds back into the JSON's length: a fixed point)
        at = HEADER_BYTES + len(_render(meta, table))
        moved = False
        for name, nbytes, _rb in sections:
            at = (at + SECTION_ALIGN - 1) // SECTION_ALIGN * SECTION_ALIGN
            moved |= table[name]["offset"] != at
            table[name]["offset"] = at
            at += int(nbytes)
        if not moved:
            return table
    raise ConvdrError("snapshot: the section offsets did not settle")


def write_snapshot(path, meta, sections, finish=None, timings=None):
    """Write the snapshot `path` ATOMICALLY: everything goes to path + ".tmp", the header last, then fsync and os.replace -- a
    failed or interrupted save leaves an existing file at `path` untouched.
    meta: the JSON's scalar fields (with window_rows).  sections: [(name, bytes, row_bytes, produce)]; produce(fd, offset) writes
    the section's bytes at that file offset (positioned writes, any order) and returns its per-window digests [(A, B)] or None.
    finish(): called once after every producer has returned, {name: [(A, B)]} for the sections whose producer returned None (a
    device-side producer reads all its digests back in one copy there).  timings: a dict that gets "fsync_s", the seconds the
    fsync took (the page cache -> disk share of a save).  Returns the file's size."""
    w = int(meta["window_rows"])
    if w < 1:
        raise ValueError("snapshot: window_rows must be >= 1 (got %d)" % w)
    table = _layout(meta, [s[:3] for s in sections], w)
    json_len = len(_render(meta, table))
    tmp = path + ".tmp"
    fd = os.open(tmp, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        got = {}
        end = HEADER_BYTES + json_len
        for name, nbytes, _rb, produce in sections:
            got[name] = produce(fd, table[name]["offset"])
            end = max(end, table[name]["offset"] + int(nbytes))
        late = finish() if finish is not None else {}
        for name in table:
            dg = got[name] if got[name] is not None else late[name]
            if len(dg) != len(table[name]["digests"]):
                raise ConvdrError("snapshot: section %r has %d windows, %d digests were produced" % (name, len(table[name]["digests"]), len(dg)))
            table[name]["digests"] = [["%016x" % (int(a) & _M64), "%016x" % (int(b) & _M64)] for a, b in dg]
        js = _render(meta, table)
        assert len(js) == json_len
        os.ftruncate(fd, end)                  # (an empty last section still ends the file where the table says)
        _pwrite_all(fd, js, HEADER_BYTES)
        _pwrite_all(fd, _HEAD.pack(MAGIC, VERSION, 0, json_len, *digest_bytes(js)).ljust(HEADER_BYTES, b"\0"), 0)
        t0 = time.perf_counter()
        os.fsync(fd)
        if timings is not None:
            timings["fsync_s"] = time.perf_counter() - t0
    except BaseException:
        os.close(fd)
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    os.close(fd)
    os.replace(tmp, path)
    return end


def _pwrite_all(fd, data, offset):
    mv = memoryview(data).cast("B")
    pos = 0
    while pos < mv.nbytes:
        pos += os.pwrite(fd, mv[pos:], offset + pos)


def pread_into(fd, mv, offset):
    """fill the byte view `mv` from file offset `offset` (os.preadv releases the GIL)"""
    pos = 0
    while pos < mv.nbytes:
        got = os.preadv(fd, [mv[pos:]], offset + pos)
        if got <= 0:
            raise ConvdrError("snapshot: short read at byte %d (the file is truncated)" % (offset + pos))
        pos += got


def read_header(path):
    """The header of a snapshot as a dict: the JSON's fields, "sections" with "digests" as (A, B) integer pairs, "file_bytes".
    Refuses (ConvdrError, with the reason; never a partial result): a bad magic, an unknown version, a truncated file, a header
    digest mismatch, a section that runs past the end of the file."""
    with open(path, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        head = f.read(HEADER_BYTES)
        if len(head) < HEADER_BYTES:
            raise ConvdrError("snapshot %s: truncated file: %d bytes, the header alone has %d" % (path, len(head), HEADER_BYTES))
        magic, version, _zero, json_len, a, b = _HEAD.unpack_from(head)
        if magic != MAGIC:
            raise ConvdrError("snapshot %s: bad magic %r (not a snapshot file)" % (path, magic))
        if version != VERSION:
            raise ConvdrError("snapshot %s: unknown version %d (this reader knows version %d)" % (path, version, VERSION))
        if HEADER_BYTES + json_len > size:
            raise ConvdrError("snapshot %s: truncated file: %d bytes, the header's JSON ends at byte %d" % (path, size, HEADER_BYTES + json_len))
        js = f.read(json_len)
    if digest_bytes(js) != (a, b):
        raise ConvdrError("snapshot %s: header digest mismatch: the JSON does not hash to what bytes 24-39 say" % path)
    h = json.loads(js.decode())
    w = int(h["window_rows"])
    for name, sec in sorted(h["sections"].items(), key=lambda kv: kv[1]["offset"]):      # (file order: the first cut is named)
        sec["digests"] = [(int(x, 16), int(y, 16)) for x, y in sec["digests"]]
        wins = _windows(sec, w)
        if len(wins) != len(sec["digests"]) or sec["bytes"] % sec["row_bytes"] or sec["offset"] % SECTION_ALIGN:
            raise ConvdrError("snapshot %s: section %r: %d bytes of %d-byte rows at offset %d with %d digests is no layout of this format"
                              % (path, name, sec["bytes"], sec["row_bytes"], sec["offset"], len(sec["digests"])))
        if sec["offset"] + sec["bytes"] > size:
            cut = next(j for j, (_a, e, _w0) in enumerate(wins) if sec["offset"] + e > size)
            raise ConvdrError("snapshot %s: truncated file: section %r (bytes %d to %d) runs past the end of the file (%d bytes), "
                              "from window %d on" % (path, name, sec["offset"], sec["offset"] + sec["bytes"], size, cut))
    h["file_bytes"] = size
    return h


def verify_file(path, threads=None):
    """Check every byte of the snapshot on the host, without a GPU: the header's own digest (read_header) and the digest of every
    window of every section (convdr_digest_host on `threads` threads, default the CPUs this process may use, at most 16).
    Raises ConvdrError naming the first section and window that differ; returns the header."""
    from concurrent.futures import ThreadPoolExecutor
    h = read_header(path)
    w = int(h["window_rows"])
    if threads is None:
        threads = min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
    piece = 8 << 20                           # (a window is read in pieces: the digest is additive)
    fd = os.open(path, os.O_RDONLY)
    try:
        def one(job):
            name, j, off, a, e, w0 = job
            buf = np.empty(min(piece, e - a), dtype=np.uint8)
            A = B = 0
            for s in range(a, e, piece):
                part = buf[:min(piece, e - s)]
                pread_into(fd, memoryview(part), off + s)
                x, y = digest_host(part, w0 + (s - a) // 8)
                A, B = (A + x) & _M64, (B + y) & _M64
            return name, j, (A, B)
        jobs = [(name, j, sec["offset"], a, e, w0) for name, sec in sorted(h["sections"].items())
                for j, (a, e, w0) in enumerate(_windows(sec, w))]
        with ThreadPoolExecutor(max_workers=max(1, int(threads))) as pool:
            for name, j, got in pool.map(one, jobs):
                want = h["sections"][name]["digests"][j]
                if got != want:
                    raise ConvdrError("snapshot %s: section %r, window %d: digest mismatch (file %016x %016x, header %016x %016x)"
                                      % (path, name, j, got[0], got[1], want[0], want[1]))
    finally:
        os.close(fd)
    return h


class FileRows:
    """Rows [row0, row0 + n) of a section as FlatIPIndex._stream_rows reads a host source: `.shape` and the positioned reads
    of a blocks.BlockView."""

    def __init__(self, fd, offset, row_bytes, row0, n, cols):
        self.fd, self.base, self.row_bytes, self.shape = fd, int(offset) + int(row0) * int(row_bytes), int(row_bytes), (int(n), int(cols))

    def read_rows_into(self, out, row0, row1, pool=None, parts=8, wait=True):
        mv = memoryview(out).cast("B")
        total = (row1 - row0) * self.row_bytes
        assert mv.nbytes >= total
        base = self.base + row0 * self.row_bytes
        if pool is None or parts <= 1 or total < (8 << 20):
            pread_into(self.fd, mv[:total], base)
            return []
        step = (total // parts + 4095) // 4096 * 4096
        futs = [pool.submit(pread_into, self.fd, mv[a:min(total, a + step)], base + a) for a in range(0, total, step)]
        if not wait:
            return futs
        for f in futs:
            f.result()
        return []
