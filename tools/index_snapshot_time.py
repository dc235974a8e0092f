#!/usr/bin/env python
"""Cost of FlatIPIndex.save / load (one verified snapshot file, convdr_amd/snapshot.py) and of the digest they rest on
(convdr_digest_rows), on one GPU: `--rows` x 768, both stores, with ids, medians of `--rounds`.

(0) equality first: load(save(A)) has A's fingerprint, verify_snapshot accepts the file.  A mismatch ends the run with status 1.
(a) save, load(verify=True) and load(verify=False) in GB/s of the file's bytes (wall clock around the call: each returns when
    the file / the index is in place), and beside them add(BlockView) of the same rows from a blocks.dump_block file -- the only
    disk -> index route there was before snapshots, and so the yardstick for load.  It is run twice, A/A, for the spread.
    Whether the files were in the page cache is recorded (mincore over the whole file, before the loads).
(b) convdr_digest_rows over each resident buffer (device events, one window and 65,536-row windows) in GB/s, beside a
    device-to-device copy of the same buffer (read + write: its GB/s counts the bytes once, as the digest's does); the shader
    clock while the digest runs back to back.

  python tools/index_snapshot_time.py [--out profiles/index_snapshot_time.txt] [--rows 1000000] [--dir /tmp]

No threshold is fixed in advance: the figures are written down."""
import argparse
import ctypes
import mmap
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

D = 768


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def resident_fraction(path):
    """fraction of the file's pages in the page cache (mincore); None when it cannot be asked"""
    try:
        size = os.path.getsize(path)
        if not size:
            return 1.0
        libc = ctypes.CDLL(None, use_errno=True)
        with open(path, "rb") as f:
            mm = mmap.mmap(f.fileno(), size, access=mmap.ACCESS_READ)
        pages = (size + mmap.PAGESIZE - 1) // mmap.PAGESIZE
        vec = (ctypes.c_ubyte * pages)()
        buf = np.frombuffer(mm, dtype=np.uint8)
        rc = libc.mincore(ctypes.c_void_p(buf.ctypes.data), ctypes.c_size_t(size), vec)
        frac = sum(v & 1 for v in vec) / pages if rc == 0 else None
        del buf
        mm.close()
        return frac
    except Exception:
        return None


def clock_under_load(fn, seconds=1.5):
    """median shader clock in MHz while fn() runs back to back (rocm-smi --showclocks read from a thread); None when it cannot
    be read"""
    import json
    import re
    import subprocess
    import threading
    samples, stop = [], threading.Event()

    def poll():
        while not stop.is_set():
            try:
                r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--json"], capture_output=True, text=True, timeout=10)
                c = json.loads(r.stdout).get("card0", {})
                samples.extend(int(re.sub(r"\D", "", v)) for k, v in c.items() if k.lower().startswith("sclk clock speed"))
            except Exception:
                return
            stop.wait(0.05)
    th = threading.Thread(target=poll, daemon=True)
    t0 = time.perf_counter()
    th.start()
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()
    stop.set()
    th.join(timeout=12)
    return statistics.median(samples) if samples else None


def rate(nbytes, ts):
    med = statistics.median(ts)
    return "%8.3f s (%.3f..%.3f)  %6.2f GB/s" % (med, min(ts), max(ts), nbytes / med / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "index_snapshot_time.py measures on a GPU; there is no CPU fallback"
    from convdr_amd import _lib, blocks
    from convdr_amd.search import FlatIPIndex, verify_snapshot
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    n = args.rows
    work = tempfile.mkdtemp(prefix="convdr_snapshot_", dir=args.dir)
    say("# index_snapshot_time: %s; %d x %d rows with ids; files under %s; medians of %d"
        % (torch.cuda.get_device_name(0), n, D, args.dir or "the default temporary directory", args.rounds))
    rs = np.random.RandomState(5)
    P = rs.randn(n, D).astype(np.float32)
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    files = []
    try:
        for storage in ("fp32", "fp16"):
            host = P.astype(np.float16) if storage == "fp16" else P
            block = os.path.join(work, "block_%s.pb" % storage)
            snap = os.path.join(work, "index_%s.convdr" % storage)
            files += [block, snap, snap + ".tmp"]
            blocks.dump_block(block, host)
            idx = FlatIPIndex(D, storage=storage, precision="auto")
            idx.prepin_staging(wait=True)
            idx.reserve(n)
            with blocks.BlockView(block) as v:
                idx.add(v, ids=ids)
            torch.cuda.synchronize()
            fp = idx.fingerprint()
            # ---- (0) equality ----------------------------------------------------------------------------------------------
            idx.save(snap)
            size = os.path.getsize(snap)
            verify_snapshot(snap)
            back = FlatIPIndex.load(snap)
            if back.fingerprint() != fp:
                say("(0) %s store: load(save(A)).fingerprint() DIFFERS from A's: nothing timed" % storage)
                return 1
            del back
            say("(0) %s store: %d rows, file %.3f GB: verify_snapshot accepts it, load(save(A)).fingerprint() == A.fingerprint()"
                % (storage, n, size / 1e9))
            # ---- (a) save / load / add(BlockView) ------------------------------------------------------------------------------
            say("# (a) %s store: wall clock per call, median (min..max), GB/s = file bytes / median" % storage)
            ts, fs = [], []
            for _ in range(args.rounds):
                ts.append(wall(lambda: idx.save(snap))[0])
                fs.append(idx.stats["save_fsync_s"])
            say("    save                      %s   (of it fsync: median %.3f s)" % (rate(size, ts), statistics.median(fs)))
            say("    page cache before the loads: snapshot %s, block file %s resident"
                % tuple("%.0f %%" % (100 * f) if f is not None else "unknown" for f in (resident_fraction(snap), resident_fraction(block))))
            for verify in (True, False):
                ts = []
                for _ in range(args.rounds):
                    t, back = wall(lambda: FlatIPIndex.load(snap, verify=verify, reserve=n))
                    ts.append(t)
                    del back
                say("    load(verify=%-5s)        %s" % (verify, rate(size, ts)))
            bsize = os.path.getsize(block)
            for tag in ("A", "A'"):
                ts = []
                for _ in range(args.rounds):
                    twin = FlatIPIndex(D, storage=storage, precision="auto", prepin=False)
                    twin.reserve(n)

                    def add():
                        with blocks.BlockView(block) as v:
                            twin.add(v, ids=ids)
                    ts.append(wall(add)[0])
                    del twin
                say("    add(BlockView) run %-2s     %s   (block file %.3f GB + ids from memory)" % (tag, rate(bsize, ts), bsize / 1e9))
            # ---- (b) the digest -----------------------------------------------------------------------------------------
            say("# (b) %s store: convdr_digest_rows per resident buffer, device events, median (min..max) of %d" % (storage, args.rounds))
            L = _lib.lib()
            for name, t, rb in (("rows", idx._rows, idx.d * (2 if storage == "fp16" else 4)), ("ids", idx.ids, 8)):
                nbytes = n * rb
                for w in (n, 65536):
                    out = torch.empty(((n + w - 1) // w, 2), dtype=torch.int64, device="cuda")

                    def dig():
                        _lib.check(L.convdr_digest_rows(_lib.ptr(t), n, rb, 0, w, _lib.ptr(out), _lib.stream_ptr()), "convdr_digest_rows")
                    ts = [timed(dig) for _ in range(args.rounds + 1)][1:]
                    med = statistics.median(ts)
                    say("    digest %-5s window %8d  %9.3f ms (%.3f..%.3f)  %8.1f GB/s" % (name, w, med, min(ts), max(ts), nbytes / med / 1e6))
                dst = torch.empty_like(t)
                ts = [timed(lambda: dst.copy_(t)) for _ in range(args.rounds + 1)][1:]
                med = statistics.median(ts)
                say("    copy   %-5s device-to-device %9.3f ms (%.3f..%.3f)  %8.1f GB/s" % (name, med, min(ts), max(ts), nbytes / med / 1e6))
                del dst
                if name == "rows":
                    mhz = clock_under_load(dig)
                    say("    shader clock while the digest of the rows runs back to back: %s" % ("%d MHz (rocm-smi)" % mhz if mhz else "not readable"))
            del idx
            torch.cuda.empty_cache()
            for f in (block, snap):
                os.unlink(f)
    finally:
        for f in files:
            try:
                os.unlink(f)
            except OSError:
                pass
        try:
            os.rmdir(work)
        except OSError:
            pass
    return 0


if __name__ == "__main__":
    sys.exit(main())
