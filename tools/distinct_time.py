#!/usr/bin/env python
"""Time of convdr_topk_distinct (first entry per key of a ranked list) on one GPU, beside convdr_topk_merge of two lists of
the same length from the same process -- the two-way merge is the step search_one_by_one pays per block, the yardstick.

Per shape: synthetic ranked lists with ties and keys on 1..4 rows (through a key map), the kernel's result asserted equal to
toplists.distinct_topk (numpy), both calls warmed up, then `--rounds` rounds of three windows each -- merge, distinct, merge
again -- every window `reps` launches between two device events, at least `--window` seconds long.  The second merge
series prices the noise ("spread": distance between the medians of the two merge series).  Times are per launch.

  python tools/distinct_time.py [--out profiles/topk_distinct_time.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

#          nq,    n, n_out
SHAPES = [(1000, 400, 100),         # topN = 100 documents of <= 4 rows each
          (100, 4096, 1000)]        # the deepest row search


def make_lists(nq, n, seed):
    rs = np.random.RandomState(seed)
    D = np.sort(rs.randint(0, 4 * n, size=(nq, n)).astype(np.float32) * 0.25, axis=1)[:, ::-1].copy()
    nids = 1 << 20
    I = rs.randint(0, nids, size=(nq, n)).astype(np.int64)
    key_map = (np.arange(nids, dtype=np.int64) // 3) * 7 + (1 << 33)          # three consecutive ids share a key
    I[:, 1::5] = I[:, 0::5][:, :I[:, 1::5].shape[1]] // 3 * 3 + 1             # ... and every fifth entry repeats its neighbour's
    return D, I, key_map


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


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
    assert torch.cuda.is_available(), "distinct_time.py measures on a GPU; there is no CPU fallback"
    from convdr_amd import _lib
    from convdr_amd import search as S
    L = _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# distinct_time: %s, %d rounds of (merge, distinct, merge) windows >= %.2f s between device events; us per launch"
        % (torch.cuda.get_device_name(0), args.rounds, args.window))
    for nq, n, n_out in SHAPES:
        D, I, key_map = make_lists(nq, n, 7 + n)
        want = S.distinct_topk(D, I, n_out, key_map)
        Dt, It, km = torch.from_numpy(D).cuda(), torch.from_numpy(I).cuda(), torch.from_numpy(key_map).cuda()
        Do = torch.empty((nq, n_out), dtype=torch.float32, device="cuda")
        Io = torch.empty((nq, n_out), dtype=torch.int64, device="cuda")
        Ko = torch.empty((nq, n_out), dtype=torch.int64, device="cuda")
        counts = torch.empty((nq, 2), dtype=torch.int32, device="cuda")
        Dm = torch.empty((nq, 2 * n), dtype=torch.float32, device="cuda")
        Im = torch.empty((nq, 2 * n), dtype=torch.int64, device="cuda")
        st = _lib.stream_ptr()

        def distinct():
            _lib.check(L.convdr_topk_distinct(_lib.ptr(Dt), _lib.ptr(It), n, n, nq, _lib.ptr(km), km.numel(), n_out, _lib.ptr(Do),
                                              _lib.ptr(Io), _lib.ptr(Ko), n_out, _lib.ptr(counts), st), "convdr_topk_distinct")

        def merge():        # two lists of n entries -> the complete merge of 2n, as toplists.merge_topk_device runs it per block
            _lib.check(L.convdr_topk_merge(_lib.ptr(Dt), _lib.ptr(It), n, n, _lib.ptr(Dt), _lib.ptr(It), n, n, nq, 2 * n, _lib.ptr(Dm),
                                           _lib.ptr(Im), 2 * n, st), "convdr_topk_merge")
        distinct()
        torch.cuda.synchronize()
        got = (Do.cpu().numpy(), Io.cpu().numpy(), Ko.cpu().numpy(), counts.cpu().numpy())
        assert all(np.array_equal(g.view(np.int32) if g.dtype == np.float32 else g, w.view(np.int32) if w.dtype == np.float32 else w)
                   for g, w in zip(got, want)), "kernel and numpy walk differ at nq=%d n=%d" % (nq, n)
        for fn in (merge, distinct):
            window(fn, 50)
        reps = {"merge": calibrate(merge, args.window), "distinct": calibrate(distinct, args.window)}
        series = {"merge": [], "distinct": [], "merge2": []}
        for _ in range(args.rounds):
            for name, fn in (("merge", merge), ("distinct", distinct), ("merge2", merge)):
                key = "distinct" if name == "distinct" else "merge"
                t = window(fn, reps[key])
                while t < args.window:                   # a window that came out short is taken again, longer
                    reps[key] = int(reps[key] * 1.5) + 1
                    t = window(fn, reps[key])
                series[name].append(1e6 * t / reps[key])
        med = {k: statistics.median(v) for k, v in series.items()}
        say("nq=%d n=%d n_out=%d  distinct %.2f us (min..max %.2f..%.2f)  merge of two lists of %d %.2f us  merge-again %.2f us  "
            "spread %.2f  distinct/merge %.2f  (mean kept per query %.0f of %d valid; repeats %d / %d)"
            % (nq, n, n_out, med["distinct"], min(series["distinct"]), max(series["distinct"]), n, med["merge"], med["merge2"],
               abs(med["merge"] - med["merge2"]), med["distinct"] / med["merge"], want[3][:, 0].mean(), n, reps["merge"],
               reps["distinct"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
