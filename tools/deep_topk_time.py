#!/usr/bin/env python
"""Cost of exact top-k beyond 4,096 on one GPU: the deep kernel pipeline (convdr_ip_search_deep*, FlatIPIndex's route for
4096 < k <= 65536) against the chunked host-side route it replaces (FlatIPIndex._search_large_k), in one process on one index.

(a) A/B at shapes the chunked route finishes in seconds: results compared for equality first, then `--rounds` rounds of three
    windows -- chunked, deep, chunked again -- each window one search between two device events.  "spread" is the distance
    between the medians of the two chunked series: what the same code differs from itself by in this run.
(b) the deep route alone at 1 M rows: device-event time of the whole search, the per-launch split from the library's own
    spans (convdr_prof_*: sample scan, threshold select, emit scan, cut, re-score, select), and the shallow search at k = 4096
    on the same index and queries as the yardstick.

  python tools/deep_topk_time.py [--out profiles/deep_topk_time.txt] [--skip-b]

No verdict is fixed in advance; the exit status is 1 only when the two routes disagree."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch            # noqa: E402

#            n,    d,  nq,     k
AB_SHAPES = [(200_000, 768, 8, 5_000),
             (200_000, 768, 8, 16_384)]
DEEP_SHAPES = [(1_000_000, 768, 100, 10_000),
               (1_000_000, 768, 1_000, 4_097)]
SPANS = ("ip_scan_sample", "ip_tau_deep", "ip_scan_emit", "ip_cut_deep", "ip_rescore_deep", "ip_select_deep")


def corpus(n, d, nq, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    P = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32)
    Q = torch.randn((nq, d), generator=g, device="cuda", dtype=torch.float32)
    return P, Q


def timed(fn):
    """milliseconds of one call between two device events (the call's host work included: both routes read certificates)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--skip-b", action="store_true", help="only the A/B of the two routes")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "deep_topk_time.py measures on a GPU; there is no CPU fallback"
    from convdr_amd import _lib
    from convdr_amd.search import FlatIPIndex
    L = _lib.lib()
    lines, ok = [], True

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                     # written as it grows: a run that is cut short leaves what it had
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    say("# deep_topk_time: %s; ms per search (device events around the whole call)" % torch.cuda.get_device_name(0))
    say("# (a) chunked route (FlatIPIndex._search_large_k) vs deep route, %d rounds of (chunked, deep, chunked)" % args.rounds)
    for n, d, nq, k in AB_SHAPES:
        P, Q = corpus(n, d, nq, 1000 + k)
        idx = FlatIPIndex(d, prepin=False)
        idx.add(P)

        def chunked():
            return idx._search_large_k(Q, k)

        def deep():
            return idx.search_tensors(Q, k)
        (Dc, Ic), (Dd, Id) = chunked(), deep()
        torch.cuda.synchronize()
        st = dict(idx.stats)
        same = torch.equal(Dc.view(torch.int32), Dd.view(torch.int32)) and torch.equal(Ic, Id)
        if not same or st.get("deep") != nq:
            ok = False
            say("n=%d d=%d nq=%d k=%d  ROUTES DISAGREE (equal=%s, stats=%s): not timed" % (n, d, nq, k, same, st))
            continue
        series = {"chunked": [], "deep": [], "chunked2": []}
        for _ in range(args.rounds):
            for name, fn in (("chunked", chunked), ("deep", deep), ("chunked2", chunked)):
                series[name].append(timed(fn)[0])
        med = {m: statistics.median(v) for m, v in series.items()}
        say("n=%d d=%d nq=%d k=%d  chunked %.1f  chunked-again %.1f  spread %.1f  deep %.2f  (chunked/deep %.0fx; min..max "
            "chunked %.1f..%.1f, deep %.2f..%.2f; deep cap %d, retried %d)"
            % (n, d, nq, k, med["chunked"], med["chunked2"], abs(med["chunked"] - med["chunked2"]), med["deep"],
               med["chunked"] / med["deep"], min(series["chunked"] + series["chunked2"]),
               max(series["chunked"] + series["chunked2"]), min(series["deep"]), max(series["deep"]), st["deep_cap"],
               st["retried"]))
        del idx, P, Q
        torch.cuda.empty_cache()
    if not args.skip_b:
        say("# (b) deep route alone; spans are summed kernel time of one search (convdr_prof_collect), ms")
        P = idx = None
        for n, d, nq, k in DEEP_SHAPES:
            if idx is None or idx.ntotal != n:
                P, _ = corpus(n, d, 1, 7)
                idx = FlatIPIndex(d, prepin=False)
                idx.add(P)
            Q = corpus(1, d, nq, 2000 + k)[1]

            def deep():
                return idx.search_tensors(Q, k)

            def shallow():
                return idx.search_tensors(Q, FlatIPIndex.MAX_K)
            deep(), shallow()                            # warm-up (workspace, one-time attributes)
            td, ts = [], []
            for _ in range(args.rounds):
                td.append(timed(deep)[0])
                st = dict(idx.stats)
                ts.append(timed(shallow)[0])
            L.convdr_prof_enable(1)
            deep()
            torch.cuda.synchronize()
            spans = ["%s %.3f (%d)" % ((name,) + _lib.prof_collect(name)) for name in SPANS]
            L.convdr_prof_enable(0)
            say("n=%d d=%d nq=%d k=%d  deep %.2f (min..max %.2f..%.2f; cap %d, retried %d of %d, rounds %d, chunked %d)  "
                "shallow k=%d on the same inputs %.2f (min..max %.2f..%.2f)"
                % (n, d, nq, k, statistics.median(td), min(td), max(td), st["deep_cap"], st["retried"], nq, st["rounds"],
                   st["chunked_queries"], FlatIPIndex.MAX_K, statistics.median(ts), min(ts), max(ts)))
            say("    spans, ms (launches): " + "; ".join(spans))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
