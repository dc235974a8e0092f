#!/usr/bin/env python
"""Cost of the row filter (FlatIPIndex.search(..., allowed=)) on one GPU: what a filtered search costs, and whether the
unfiltered search pays anything for the feature's existence.

(0) equality first.  On a 20,000-row sub-sample a 50 % filter is compared with the oracle over the allowed rows
    (oracle.search.flat_ip_search(Q, P[rows], k), I mapped back).  At the full shape the all-rows filter must return the
    unfiltered search's bytes, and every other filter the bytes of an exact search over a COMPACT index built from P[rows] alone,
    mapped back through rows (two exact searches of one corpus).  A mismatch ends the run with exit status 1; nothing is timed.
(a) `--rows` x 768 resident, `--queries` (default 100 and 1,000) queries, top-100, both storages.  Per round one window each of:
    unfiltered, all rows allowed, random 50 %, random 1 %, a contiguous half, unfiltered again -- "spread" is the distance between
    the two unfiltered medians.  Device events around the whole search (certificates read); the filters are built before the
    clock starts (row_filter is a build-time cost, reported on its own line).  A second, profiled pass reports the
    `ip_scan_emit` span (convdr_prof_collect).
(b) `--parent-lib PATH`: the unfiltered search of this build against another build of the library (the parent commit's), each
    in FRESH child processes that alternate, `--ab-runs` of each: per library the medians of every run and their spread.

  python tools/row_filter_time.py [--out profiles/row_filter_time.txt] [--rows 1000000] [--parent-lib gpu_jobs/parent/libconvdr_hip.so]

No verdict is fixed in advance: the figures are written down."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

D, K = 768, 100
MASKS = ("all", "random 50 %", "random 1 %", "contiguous half")


def corpus(n, nq, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    P = torch.randn((n, D), generator=g, device="cuda").half().float()      # both stores hold the same corpus
    Q = torch.randn((nq, D), generator=g, device="cuda")
    return P, Q


def mask_of(name, n):
    g = torch.Generator(device="cuda").manual_seed(5)
    if name == "all":
        return torch.ones(n, dtype=torch.bool, device="cuda")
    if name == "contiguous half":
        m = torch.zeros(n, dtype=torch.bool, device="cuda")
        m[n // 4:n // 4 + n // 2] = True
        return m
    return torch.rand(n, generator=g, device="cuda") < (0.5 if "50" in name else 0.01)


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
    idx.add(P.half() if storage == "fp16" else P.clone())
    return idx


def load_lib():
    """the library CONVDR_HIP_LIB names; a build from before the filter lacks its entry, which the unfiltered search never calls"""
    from convdr_amd import _lib
    try:
        return _lib.lib()
    except AttributeError:
        # lib() cached the handle and stopped binding signatures at the missing entry: drop both and bind again from the start
        _lib._SIGNATURES.pop("convdr_ip_search_filtered")
        _lib._lib = None
        return _lib.lib()


def child(args):
    """--child: unfiltered searches only, medians as one JSON line"""
    load_lib()
    out = {}
    for storage in ("fp32", "fp16"):
        P, _ = corpus(args.rows, 1, 23)
        idx = index(storage, P)
        del P
        for nq in args.queries:
            Q = corpus(1, nq, 29)[1]
            idx.search_tensors(Q, K)
            out["%s nq=%d" % (storage, nq)] = statistics.median(timed(lambda: idx.search_tensors(Q, K))[0] for _ in range(args.reps))
        del idx
        torch.cuda.empty_cache()
    print("CHILD " + json.dumps(out), flush=True)
    return 0


def same(a, b):
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "row_filter_time.py measures on a GPU; there is no CPU fallback"
    if args.child:
        return child(args)
    from convdr_amd import _lib
    from oracle import search as OS
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    n = args.rows
    say("# row_filter_time: %s; %d x %d rows, top-%d" % (torch.cuda.get_device_name(0), n, D, K))

    # ---- (0) equality on a sub-sample, against the oracle ----------------------------------------------------------------
    P, Q = corpus(20000, 16, 11)
    m = mask_of("random 50 %", 20000)
    rows = np.flatnonzero(m.cpu().numpy())
    Dr, Ir = OS.flat_ip_search(Q.cpu().numpy(), P.cpu().numpy()[rows], K)
    for storage in ("fp32", "fp16"):
        Df, If = index(storage, P).search(Q.cpu().numpy(), K, allowed=m)
        if not (np.array_equal(If, rows[Ir]) and np.array_equal(Df, Dr)):
            say("(0) %s store, 20000 x 16, 50 %% filter: DIFFERS FROM THE ORACLE over the allowed rows: nothing timed" % storage)
            return 1
    say("(0) sub-sample 20000 rows x 16 queries, 50 % filter, both stores: == oracle over the allowed rows (D and I, bit for bit)")
    del P, Q

    # ---- (a) the filters at the full shape ---------------------------------------------------------------------------------
    say("# (a) ms per search, medians of %d windows; rounds of (unfiltered, %s, unfiltered again); emit = ip_scan_emit span of one "
        "profiled search (launches)" % (args.rounds, ", ".join(MASKS)))
    for storage in ("fp32", "fp16"):
        P, _ = corpus(n, 1, 23)
        idx = index(storage, P)
        build_ms, filters = {}, {}
        for name in MASKS:
            mk = mask_of(name, n)
            build_ms[name], filters[name] = timed(lambda: idx.row_filter(mk))
        say("%s store: row_filter(mask on the device) %s ms; allowed rows %s"
            % (storage, ", ".join("%.2f" % build_ms[x] for x in MASKS), ", ".join(str(filters[x].n_allowed) for x in MASKS)))
        for nq in args.queries:
            Q = corpus(1, nq, 29)[1]
            base = idx.search_tensors(Q, K)
            for name in MASKS:
                got = idx.search_tensors(Q, K, allowed=filters[name])
                if name == "all":
                    want = base
                else:
                    r = filters[name].rows()
                    Dc, Ic = index(storage, P[r]).search_tensors(Q, K)
                    want = (Dc, torch.where(Ic >= 0, r[Ic.clamp_min(0)], Ic))
                torch.cuda.synchronize()
                if not same(got, want):
                    say("(a) %s store nq=%d filter '%s': DIFFERS from the %s: not timed"
                        % (storage, nq, name, "unfiltered search" if name == "all" else "search of the compact index"))
                    return 1
            kinds = ("unfiltered",) + MASKS + ("unfiltered again",)
            series = {x: [] for x in kinds}
            stats = {}
            for _ in range(args.rounds):
                for x in kinds:
                    f = filters.get(x)
                    series[x].append(timed(lambda: idx.search_tensors(Q, K, allowed=f))[0])
                    stats[x] = dict(idx.stats)
            emit = {}
            for x in kinds[:-1]:
                _lib.lib().convdr_prof_enable(1)
                idx.search_tensors(Q, K, allowed=filters.get(x))
                torch.cuda.synchronize()
                emit[x] = _lib.prof_collect("ip_scan_emit")
                _lib.lib().convdr_prof_enable(0)
            med = {x: statistics.median(v) for x, v in series.items()}
            say("%s store nq=%d: results equal; unfiltered %.3f  again %.3f  spread %.3f" % (storage, nq, med["unfiltered"],
                med["unfiltered again"], abs(med["unfiltered"] - med["unfiltered again"])))
            for x in kinds[:-1]:
                st = stats[x]
                say("    %-16s %8.3f ms (%.2fx unfiltered; min..max %.3f..%.3f)  emit %.3f ms (%d)  rounds %d retried %d x2/x3 %d"
                    % (x, med[x], med[x] / med["unfiltered"], min(series[x]), max(series[x]), emit[x][0], emit[x][1],
                       st["rounds"], st["retried"], st.get("x2_queries", 0) + st["x3_queries"]))
            del Q
        del idx, P, filters
        torch.cuda.empty_cache()

    # ---- (b) the unfiltered search: this build against another build of the library, fresh processes --------------------
    if args.parent_lib:
        here = os.path.join(ROOT, "convdr_amd", "libconvdr_hip.so")
        libs = {"parent": os.path.abspath(args.parent_lib), "this": os.environ.get("CONVDR_HIP_LIB") or here}
        say("# (b) unfiltered search, ms (median of %d searches per process); fresh child processes alternate (parent, this) x %d"
            % (args.reps, args.ab_runs))
        runs = {"parent": [], "this": []}
        for _ in range(args.ab_runs):
            for who in ("parent", "this"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rows", str(n), "--reps", str(args.reps), "--queries"] + \
                      [str(q) for q in args.queries]
                res = subprocess.run(cmd, env=dict(os.environ, CONVDR_HIP_LIB=libs[who]), capture_output=True, text=True, timeout=300)
                got = [ln for ln in res.stdout.splitlines() if ln.startswith("CHILD ")]
                if res.returncode != 0 or not got:
                    say("(b) child process with the %s library failed (exit status %d): %s" % (who, res.returncode, res.stderr[-400:]))
                    return 1
                runs[who].append(json.loads(got[-1][6:]))
        for key in runs["this"][0]:
            a, b = [r[key] for r in runs["parent"]], [r[key] for r in runs["this"]]
            spread = max(max(a) - min(a), max(b) - min(b))
            say("%-14s parent %s (median %.3f, spread %.3f)  this %s (median %.3f, spread %.3f)  this - parent %+.3f ms; inside the "
                "spread of repeated runs (%.3f): %s"
                % (key, " ".join("%.3f" % v for v in a), statistics.median(a), max(a) - min(a), " ".join("%.3f" % v for v in b),
                   statistics.median(b), max(b) - min(b), statistics.median(b) - statistics.median(a), spread,
                   "yes" if abs(statistics.median(b) - statistics.median(a)) <= spread else "NO"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
