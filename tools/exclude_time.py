#!/usr/bin/env python
"""Cost of per-query exclusions (FlatIPIndex.excluding(ex).search_tensors / rank_rows_tensors) on one GPU.

`--rows` x 768 resident (default 1 M), both stores, `--queries` queries (default 1,000), k = 100, e in {1, 10, 100, 1,000, 5,000}
excluded rows per query: each query's own top e ranks, so every excluded row bites and the result is ranks e .. e + k - 1.

(0) equality first, at the full shape: excluding(ex).search_tensors(Q, k) must return columns e .. e + k - 1 of the plain search at
    depth k + e, bit for bit, and excluding(ex).rank_rows_tensors of the row at residual rank k / 2 must be k / 2.  A mismatch ends
    the run with exit status 1; nothing is timed.
(a) this build, ms per call (hipEvent, median of `--reps` = 5): exclude_rows (the build), search_tensors(Q, k),
    search_tensors(Q, k + e), excluding(ex).search_tensors(Q, k), rank_rows_tensors(Q, t), excluding(ex).rank_rows_tensors(Q, t);
    the shader clock while the excluded search runs back to back.
(b) `--parent-lib PATH`: search_tensors(Q, k), search_tensors(Q, k + e) and rank_rows_tensors(Q, t) with another build of the
    library (the parent commit's) beside this build's, in FRESH child processes that alternate, `--ab-runs` of each.

  python tools/exclude_time.py [--out profiles/exclude_time.txt] [--rows 1000000] [--parent-lib gpu_jobs/parent/libconvdr_hip.so]

No verdict is fixed in advance: the figures are written down."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch            # noqa: E402

from tools.doc_ops_time import clock_under_load          # noqa: E402
from tools.row_filter_time import corpus, index, timed  # noqa: E402

K = 100
ES = (1, 10, 100, 1000, 5000)
NEW = ("convdr_excl_build_rows", "convdr_excl_build_docs", "convdr_excl_drop_topk", "convdr_excl_count_ragged", "convdr_excl_pack_ragged",
       "convdr_ip_excl_count_ahead")


def load_lib():
    """the library CONVDR_HIP_LIB names; a build from before the exclusions lacks their entries, which the plain calls never use"""
    from convdr_amd import _lib
    try:
        return _lib.lib()
    except AttributeError:
        for name in NEW:
            _lib._SIGNATURES.pop(name, None)
        _lib._lib = None
        return _lib.lib()


def med(fn, reps):
    fn()
    return statistics.median(timed(fn)[0] for _ in range(reps))


def child(args):
    """--child: the plain calls only, medians as one JSON line"""
    load_lib()
    out = {}
    for storage in ("fp32", "fp16"):
        P, _ = corpus(args.rows, 1, 23)
        idx = index(storage, P)
        del P
        Q = corpus(1, args.queries, 29)[1]
        t = idx.search_tensors(Q, K)[1][:, K // 2].contiguous()
        out["%s search k" % storage] = med(lambda: idx.search_tensors(Q, K), args.reps)
        for e in ES:
            out["%s search k+%d" % (storage, e)] = med(lambda: idx.search_tensors(Q, K + e), args.reps)
        out["%s rank" % storage] = med(lambda: idx.rank_rows_tensors(Q, t), args.reps)
        del idx
        torch.cuda.empty_cache()
    print("CHILD " + json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ab-runs", type=int, default=2)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "exclude_time.py measures on a GPU; there is no CPU fallback"
    if args.child:
        return child(args)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    n, nq = args.rows, args.queries
    say("# exclude_time: %s; %d x 768 rows, %d queries, k = %d; each query excludes its own top e ranks; ms, hipEvent medians of %d"
        % (torch.cuda.get_device_name(0), n, nq, K, args.reps))
    for storage in ("fp32", "fp16"):
        P, _ = corpus(n, 1, 23)
        idx = index(storage, P)
        del P
        Q = corpus(1, nq, 29)[1]
        plain_ms = med(lambda: idx.search_tensors(Q, K), args.reps)
        say("%s store: search_tensors(Q, k) %.3f ms" % (storage, plain_ms))
        for e in ES:
            Dw, Iw = idx.search_tensors(Q, K + e)
            lists = Iw[:, :e].contiguous()
            t = Iw[:, e + K // 2].contiguous()
            build_ms, ex = timed(lambda: idx.exclude_rows(lists))
            got = idx.excluding(ex).search_tensors(Q, K)
            depth, dropped = idx.stats["exclude_depth"], idx.stats["excluded_dropped"]
            rk = idx.excluding(ex).rank_rows_tensors(Q, t)
            if not (torch.equal(got[1], Iw[:, e:]) and torch.equal(got[0].view(torch.int32), Dw[:, e:].contiguous().view(torch.int32))
                    and bool((rk == K // 2).all())):
                say("(0) %s store e=%d: the excluded search or rank DIFFERS from the plain search at depth k + e: nothing timed" % (storage, e))
                return 1
            deep_ms = med(lambda: idx.search_tensors(Q, K + e), args.reps)
            ex_ms = med(lambda: idx.excluding(ex).search_tensors(Q, K), args.reps)
            rank_ms = med(lambda: idx.rank_rows_tensors(Q, t), args.reps)
            rank_ex_ms = med(lambda: idx.excluding(ex).rank_rows_tensors(Q, t), args.reps)
            mhz = clock_under_load(lambda: idx.excluding(ex).search_tensors(Q, K), seconds=1.0)
            say("    e=%-5d equal; exclude_rows %.3f | search k+e %.3f  excluding %.3f (%+.3f: the drop and its host read; depth %d, "
                "dropped %d) | rank_rows %.3f  excluding %.3f (%+.3f) | shader clock %s"
                % (e, build_ms, deep_ms, ex_ms, ex_ms - deep_ms, depth, dropped, rank_ms, rank_ex_ms, rank_ex_ms - rank_ms,
                   "%d MHz" % mhz if mhz else "not readable"))
        del idx, Q
        torch.cuda.empty_cache()
    if args.parent_lib:
        here = os.path.join(ROOT, "convdr_amd", "libconvdr_hip.so")
        libs = {"parent": os.path.abspath(args.parent_lib), "this": os.environ.get("CONVDR_HIP_LIB") or here}
        say("# (b) the plain calls, ms (median of %d per process); fresh child processes alternate (parent, this) x %d" % (args.reps, args.ab_runs))
        runs = {"parent": [], "this": []}
        for _ in range(args.ab_runs):
            for who in ("parent", "this"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rows", str(n), "--queries", str(nq), "--reps", str(args.reps)]
                res = subprocess.run(cmd, env=dict(os.environ, CONVDR_HIP_LIB=libs[who]), capture_output=True, text=True, timeout=400)
                got = [ln for ln in res.stdout.splitlines() if ln.startswith("CHILD ")]
                if res.returncode != 0 or not got:
                    say("(b) child process with the %s library failed (exit status %d): %s" % (who, res.returncode, res.stderr[-400:]))
                    return 1
                runs[who].append(json.loads(got[-1][6:]))
        for key in runs["this"][0]:
            a, b = [r[key] for r in runs["parent"]], [r[key] for r in runs["this"]]
            say("%-22s parent %s  this %s  this - parent %+.3f ms (spread of repeated runs %.3f)"
                % (key, " ".join("%.3f" % v for v in a), " ".join("%.3f" % v for v in b), statistics.median(b) - statistics.median(a),
                   max(max(a) - min(a), max(b) - min(b))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
