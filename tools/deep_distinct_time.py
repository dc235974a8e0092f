#!/usr/bin/env python
"""Cost of the two deep list kernels on one GPU, each beside the route the same job took before them.

(a) convdr_topk_distinct_deep (toplists.distinct_topk_device for n > 4096) against the device-to-host copy of the ranked lists +
    toplists.distinct_topk (the numpy walk), the only route lists of that length had.
(b) convdr_topk_merge_deep (parallel.merge_rank_topk for k > 4096) against the stable descending torch.sort of the
    rank-ordered concatenation on the device + two gathers.

Results are compared for bit equality first; then `--rounds` rounds of three windows -- old, new, old again -- each window one
call between two device events (host work inside the window included).  "spread" is the distance between the medians of the
two old-route series: what the same code differs from itself by in this run.

  python tools/deep_distinct_time.py [--out profiles/deep_distinct_time.txt] [--rounds 5]

No verdict is fixed in advance; the exit status is 1 only when two routes disagree."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

#                   nq,      n, n_out, keys
DISTINCT_SHAPES = [(100, 10_000, 1_000, "1..4 rows per key"),
                   (1_000, 5_000, 1_000, "1..4 rows per key"),
                   (100, 65_536, 6_553, "distinct keys"),
                   (100, 65_536, 6_553, "one key")]
#                W,      k,  nq
MERGE_SHAPES = [(8, 10_000, 100),
                (2, 65_536, 100)]


def timed(fn):
    """milliseconds of one call between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def ranked_lists(nq, n, keys, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    D = torch.sort(torch.randn((nq, n), generator=g, device="cuda"), dim=1, descending=True).values
    if keys == "one key":
        I = torch.full((nq, n), 2 ** 40 + 17, dtype=torch.int64, device="cuda")
    elif keys == "distinct keys":
        I = torch.argsort(torch.rand((nq, n), generator=g, device="cuda"), dim=1) * 3 + 2 ** 33
    else:
        I = torch.randint(0, max(1, int(n / 2.5)), (nq, n), generator=g, device="cuda", dtype=torch.int64) + 2 ** 35
    return D.contiguous(), I.contiguous()


def abx(old, new, rounds):
    series = {"old": [], "new": [], "old2": []}
    for _ in range(rounds):
        for name, fn in (("old", old), ("new", new), ("old2", old)):
            series[name].append(timed(fn)[0])
    med = {m: statistics.median(v) for m, v in series.items()}
    return med, series


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "deep_distinct_time.txt"), help="the report is also written here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "deep_distinct_time.py measures on a GPU; there is no CPU fallback"
    from convdr_amd import parallel
    from convdr_amd import search as S
    lines, ok = [], True

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                     # written as it grows: a run that is cut short leaves what it had
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    say("# deep_distinct_time: %s; ms per call (device events around the whole call), %d rounds of (old, new, old)"
        % (torch.cuda.get_device_name(0), args.rounds))
    say("# (a) first entry per key: copy to the host + toplists.distinct_topk (numpy)  vs  convdr_topk_distinct_deep")
    for nq, n, n_out, keys in DISTINCT_SHAPES:
        D, I = ranked_lists(nq, n, keys, 1000 + n + nq)

        def host():
            return S.distinct_topk(D.cpu().numpy(), I.cpu().numpy(), n_out)

        def deep():
            return S.distinct_topk_device(D, I, n_out)
        h, g = host(), deep()
        torch.cuda.synchronize()
        same = all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), b.cpu().numpy().view(np.uint8)) for a, b in zip(h, g))
        if not same:
            ok = False
            say("nq=%d n=%d n_out=%d %s  ROUTES DISAGREE: not timed" % (nq, n, n_out, keys))
            continue
        med, s = abx(host, deep, args.rounds)
        say("nq=%d n=%d n_out=%d %s  host %.1f  host-again %.1f  spread %.1f  deep %.3f  (host/deep %.0fx; min..max host "
            "%.1f..%.1f, deep %.3f..%.3f)" % (nq, n, n_out, keys, med["old"], med["old2"], abs(med["old"] - med["old2"]), med["new"],
                                             med["old"] / med["new"], min(s["old"] + s["old2"]), max(s["old"] + s["old2"]),
                                             min(s["new"]), max(s["new"])))
    say("# (b) W-way merge: stable descending torch.sort of the concatenation + gathers  vs  convdr_topk_merge_deep")
    for W, k, nq in MERGE_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(2000 + k)
        # scores on a grid of 4,096 values: ties inside and across lists, as exact duplicates across blocks give
        D_all = torch.sort(torch.randint(0, 4096, (W, nq, k), generator=g, device="cuda").float() * 0.01, dim=2,
                           descending=True).values.contiguous()
        I_all = torch.randint(0, 2 ** 62, (W, nq, k), generator=g, device="cuda", dtype=torch.int64)

        def sort():
            d = D_all.permute(1, 0, 2).reshape(nq, W * k)
            i = I_all.permute(1, 0, 2).reshape(nq, W * k)
            order = torch.sort(d, dim=1, descending=True, stable=True).indices[:, :k]
            return torch.gather(d, 1, order), torch.gather(i, 1, order)

        def deep():
            return parallel.merge_rank_topk(D_all, I_all, k)
        (Ds, Is), (Dd, Id) = sort(), deep()
        torch.cuda.synchronize()
        if not (torch.equal(Ds.view(torch.int32), Dd.view(torch.int32)) and torch.equal(Is, Id)):
            ok = False
            say("W=%d k=%d nq=%d  ROUTES DISAGREE: not timed" % (W, k, nq))
            continue
        med, s = abx(sort, deep, args.rounds)
        say("W=%d k=%d nq=%d  sort %.3f  sort-again %.3f  spread %.3f  deep %.3f  (sort/deep %.2fx; min..max sort %.3f..%.3f, "
            "deep %.3f..%.3f)" % (W, k, nq, med["old"], med["old2"], abs(med["old"] - med["old2"]), med["new"],
                                  med["old"] / med["new"], min(s["old"] + s["old2"]), max(s["old"] + s["old2"]), min(s["new"]),
                                  max(s["new"])))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
