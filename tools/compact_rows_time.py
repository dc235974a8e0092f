#!/usr/bin/env python
"""Cost of removing rows in place (FlatIPIndex.keep_rows: convdr_ip_compact_plan + convdr_ip_compact_rows per resident buffer)
on one GPU, beside the out-of-place torch gather of the same rows and a plain device-to-device copy of the same bytes.

(0) equality first.  At the full shape, both storages, one removal of a random half per window size: every resident buffer
    must equal clone_before[keep] bit for bit.  A mismatch ends the run with exit status 1; nothing is timed.
(a) `--rows` x 768 resident, both storages; removed: a random 1 %, a random 50 %, and the contiguous last 10 % (nothing moves:
    every window skips -- the cost of the launches alone).  For every window size of `--windows` the median and min..max of
    `--rounds` device-event windows around keep_rows(filter) -- the filter is built before (its one host read is the caller's
    in any flow), so the window holds the plan and the moves of every buffer and no host read.  Between rounds the row count
    is put back; the rows' contents do not matter to the time.
    bytes moved = (kept rows that change place) x (row bytes of every resident buffer); GB/s = bytes moved / time -- payload,
    i.e. one read and one write per byte for the direct form and two of each for windows that go through the bounce buffer.
    Beside it, in the same process: `gather` = [buf[keep] for every buffer] (out of place: a second copy of the kept rows), and
    `copy` = one device-to-device copy of as many bytes as were moved (the ceiling).

  python tools/compact_rows_time.py [--out profiles/compact_rows_time.txt] [--rows 1000000]

No ratio is fixed in advance: the figures are written down, and the last line names the window size that did best."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch            # noqa: E402

D = 768


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def index(storage, P):
    from convdr_amd.search import FlatIPIndex
    idx = FlatIPIndex(D, storage=storage, precision="auto", prepin=False)
    idx.reserve(P.shape[0])
    idx.add(P.half() if storage == "fp16" else P)
    return idx


def buffers(idx):
    return [t for t in (idx._s32, idx._s16, idx._slo) if t is not None]


def masks(n, g):
    tail = torch.ones(n, dtype=torch.bool, device="cuda")
    tail[n - n // 10:] = False
    return (("random 1 % removed", torch.rand(n, generator=g, device="cuda") >= 0.01),
            ("random 50 % removed", torch.rand(n, generator=g, device="cuda") >= 0.5),
            ("last 10 % removed", tail))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--windows", type=int, nargs="+", default=[1024, 4096, 16384, 65536, 262144])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "compact_rows_time.py measures on a GPU; there is no CPU fallback"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    n = args.rows
    g = torch.Generator(device="cuda").manual_seed(17)
    P = torch.randn((n, D), generator=g, device="cuda")
    say("# compact_rows_time: %s; %d x %d rows" % (torch.cuda.get_device_name(0), n, D))

    # ---- (0) equality at the full shape ------------------------------------------------------------------------------------
    keep = masks(n, g)[1][1]
    for storage in ("fp32", "fp16"):
        for w in args.windows:
            idx = index(storage, P)
            idx.compact_window_rows = w
            before = [t[:n].clone() for t in buffers(idx)]
            idx.keep_rows(keep)
            for t, b in zip(buffers(idx), before):
                if not torch.equal(t[:idx.ntotal].view(torch.int16), b[keep].view(torch.int16)):
                    say("(0) %s store window %d: a buffer DIFFERS from clone[keep]: nothing timed" % (storage, w))
                    return 1
            del idx, before
    say("(0) %d rows, a random half removed, both stores, windows %s: every buffer == clone[keep] bit for bit" % (n, args.windows))

    # ---- (a) times -------------------------------------------------------------------------------------------------------------
    say("# (a) ms per call: median (min..max) of %d device-event windows; GB/s = bytes moved / median" % args.rounds)
    best = {}
    for storage in ("fp32", "fp16"):
        idx = index(storage, P)
        bufs = buffers(idx)
        row_bytes = sum(int(t.shape[1]) * t.element_size() for t in bufs)
        for name, keep in masks(n, g):
            f = idx.row_filter(keep)
            dest = torch.cumsum(keep, 0) - 1
            moved = int((keep & (dest != torch.arange(n, device="cuda"))).sum()) * row_bytes
            say("%s store (%d buffers, %d bytes per row), %s: %d kept, %.3f GB moved" % (storage, len(bufs), row_bytes, name, f.n_allowed,
                                                                                          moved / 1e9))
            for w in args.windows:
                idx.compact_window_rows = w
                series = []
                for _ in range(args.rounds + 1):
                    series.append(timed(lambda: idx.keep_rows(f))[0])
                    idx._n = n                                  # (put the row count back: the contents do not matter to the time)
                series = series[1:]                              # (the first call may allocate the workspace)
                med = statistics.median(series)
                say("    keep_rows window %7d  %9.3f ms (%.3f..%.3f)  %8.1f GB/s  %d launches"
                    % (w, med, min(series), max(series), moved / med / 1e6, 2 + 2 * len(bufs) * ((n + w - 1) // w)))
                if moved:
                    best.setdefault(w, []).append(med)
            idx._ws = None
            series = []
            for _ in range(args.rounds + 1):
                series.append(timed(lambda: [t[:n][keep] for t in bufs])[0])
            med = statistics.median(series[1:])
            say("    gather  buf[keep] (out of place, all kept rows)  %9.3f ms (%.3f..%.3f)" % (med, min(series[1:]), max(series[1:])))
            if moved:
                src = torch.empty(moved, dtype=torch.uint8, device="cuda")
                dst = torch.empty_like(src)
                series = [timed(lambda: dst.copy_(src))[0] for _ in range(args.rounds + 1)][1:]
                med = statistics.median(series)
                say("    copy    device-to-device, the bytes moved        %9.3f ms (%.3f..%.3f)  %8.1f GB/s"
                    % (med, min(series), max(series), moved / med / 1e6))
                del src, dst
        del idx, bufs
        torch.cuda.empty_cache()
    total = {w: sum(v) for w, v in best.items()}
    w_best = min(total, key=total.get)
    say("# sum of the medians over the cases that move rows, per window: %s" % ", ".join("%d: %.3f ms" % (w, total[w]) for w in sorted(total)))
    say("# best window_rows: %d (bounce buffer %.0f MB at 3,072-byte rows)" % (w_best, w_best * 3072 / 2 ** 20))
    return 0


if __name__ == "__main__":
    sys.exit(main())
