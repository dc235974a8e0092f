#!/usr/bin/env python
"""A/B of the cross-rank top-k merge on one GPU: the chain of W - 1 two-way convdr_topk_merge launches
(parallel._merge_rank_topk_chain) against parallel.merge_rank_topk (one convdr_topk_merge_multi launch), in one process.

Per shape: synthetic [W, nq, k] lists with ties, both paths asserted bit-identical, both warmed up, then `--rounds` rounds
of three windows each -- chain, new, chain again -- every window at least `--window` seconds of repeated merges between
two device synchronises.  The second chain series prices the noise: "spread" is the distance between the medians of the
two chain series, i.e. what the same code differs from itself by in this run.  Times are per merge (window / repeats).

  python tools/merge_ab.py [--out profiles/topk_merge_multi_ab.txt]

Verdict (exit status 1 when it fails): at nq = 1000, k = 100, W = 8 the new path's median is no longer than the chain's
median plus the spread.  The other shapes are for the record."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

#          W,   nq,    k, judged
SHAPES = [(2, 1000, 100, False),
          (4, 1000, 100, False),
          (8, 1000, 100, True),         # BASELINE configs[3]'s exchange
          (8, 1000, 1000, False),
          (8, 100, 4096, False)]


def make_lists(W, nq, k, seed):
    rs = np.random.RandomState(seed)
    D = np.sort(rs.randint(0, 4 * k, size=(W, nq, k)).astype(np.float32) * 0.25, axis=2)[:, :, ::-1].copy()
    I = rs.randint(0, 2 ** 40, size=(W, nq, k), dtype=np.int64)
    D[W - 1, :, k - k // 4:] = -3.4028234663852886e38        # the last rank's block was short: FAISS padding
    I[W - 1, :, k - k // 4:] = -1
    return torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda()


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def calibrate(fn, seconds):
    reps = 16
    while True:
        t = window(fn, reps)
        if t >= seconds:
            return reps
        reps = max(reps * 2, int(reps * 1.3 * seconds / max(t, 1e-6)) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="least seconds per timed window")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "merge_ab.py measures on a GPU; there is no CPU fallback"
    from convdr_amd import parallel
    lines, ok = [], True

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# merge_ab: %s, %d rounds of (chain, new, chain) windows >= %.2f s; us per merge"
        % (torch.cuda.get_device_name(0), args.rounds, args.window))
    for W, nq, k, judged in SHAPES:
        D, I = make_lists(W, nq, k, 100 + W)

        def chain():
            return parallel._merge_rank_topk_chain(D, I, k)

        def new():
            return parallel.merge_rank_topk(D, I, k)
        (Dc, Ic), (Dn, In) = chain(), new()
        torch.cuda.synchronize()
        assert torch.equal(Dc.contiguous().view(torch.int32), Dn.contiguous().view(torch.int32)) and torch.equal(Ic, In), \
            "chain and one-launch merge differ at W=%d nq=%d k=%d" % (W, nq, k)
        for fn in (chain, new):                          # warm-up of both
            window(fn, 50)
        reps = {"chain": calibrate(chain, args.window), "new": calibrate(new, args.window)}
        series = {"chain": [], "new": [], "chain2": []}
        shortest = 1e9
        for _ in range(args.rounds):
            for name, fn in (("chain", chain), ("new", new), ("chain2", chain)):
                r = reps["new" if name == "new" else "chain"]
                t = window(fn, r)
                while t < args.window:                   # a window that came out short is taken again, longer
                    r = reps["new" if name == "new" else "chain"] = int(r * 1.5) + 1
                    t = window(fn, r)
                shortest = min(shortest, t)
                series[name].append(1e6 * t / r)
        med = {n: statistics.median(v) for n, v in series.items()}
        spread = abs(med["chain"] - med["chain2"])
        verdict = ""
        if judged:
            good = med["new"] <= med["chain"] + spread
            ok = ok and good
            verdict = "  -> %s (new <= chain + spread)" % ("PASS" if good else "FAIL")
        say("W=%d nq=%d k=%d  chain %.2f  chain-again %.2f  spread %.2f  new %.2f  (new/chain %.3f; min..max chain %.2f..%.2f, "
            "new %.2f..%.2f; repeats %d / %d, shortest window %.3f s)%s"
            % (W, nq, k, med["chain"], med["chain2"], spread, med["new"], med["new"] / med["chain"],
               min(series["chain"] + series["chain2"]), max(series["chain"] + series["chain2"]), min(series["new"]),
               max(series["new"]), reps["chain"], reps["new"], shortest, verdict))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
