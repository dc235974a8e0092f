#!/usr/bin/env python
"""Cost of judging a run on the device (convdr_amd.judge.judge_run: distinct keys -> labels -> measures, plus run_negatives)
beside the host route, on one GPU, in one process.

  shapes   `--nq` (1,000) queries with raw search output D / I [nq, n] for n = 100, 4,096 and 65,536: distinct rows of a
           200,000-row corpus whose keys sit on 1 to 3 rows each (key_map), scores descending; per query 50 judged keys of its own
           list and 10 others, grades -1..3.
  device   judge_run(D, I, qrels, key_map, cutoffs=(3, 10, 100)) and, separately, run_negatives on its K and labels: device
           events around the calls, medians and min..max of `--rounds` windows after a warm-up.  mean() (the one host read) apart.
  host     what a caller does without these kernels: D.cpu(), I.cpu(), convdr_amd.toplists.distinct_topk (numpy), then the oracle of
           the tests (tests/judge_cases.py: dict lookups, plain loops) for labels, measures and negatives.  The oracle is plain
           Python, so at the deeper shapes it is run on the first `--host-queries` queries only and the time for all of them is
           that figure scaled by nq / queries (marked "scaled").
  (0)      before anything is timed the two routes are compared on those queries: labels and negatives bit for bit, measures as
           in tests/test_judge_run_gpu.py.  A mismatch ends the run with exit status 1.

  python tools/judge_run_time.py [--out profiles/judge_run_time.txt]

No ratio is fixed in advance: the figures are written down."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

ROWS = 200_000
CUTOFFS = (3, 10, 100)
SHAPES = ((100, None), (4096, 100), (65536, 10))       # (n, host queries; None = all)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def search_output(nq, n, seed):
    """(D fp32 [nq, n] descending, I int64 [nq, n] distinct rows per query, key_map int64 [ROWS]) on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    I = torch.empty((nq, n), dtype=torch.int64, device="cuda")
    for a in range(0, nq, 100):
        b = min(nq, a + 100)
        I[a:b] = torch.argsort(torch.rand((b - a, ROWS), generator=g, device="cuda"), dim=1)[:, :n]
    D = torch.sort(torch.randn((nq, n), generator=g, device="cuda"), dim=1, descending=True)[0].contiguous()
    per_key = torch.randint(1, 4, (ROWS,), generator=g, device="cuda")
    key_map = torch.repeat_interleave(torch.arange(ROWS, device="cuda") + (1 << 33), per_key)[:ROWS]
    key_map = key_map[torch.randperm(ROWS, generator=g, device="cuda")].contiguous()
    return D, I, key_map


def judged_sets(I, key_map, seed):
    rs = np.random.RandomState(seed)
    Ih, km = I.cpu().numpy(), key_map.cpu().numpy()
    out = []
    for j in range(len(Ih)):
        own = km[Ih[j, rs.randint(0, Ih.shape[1], 50)]]
        keys = np.unique(np.concatenate([own, km[rs.randint(0, ROWS, 10)]]))
        out.append({int(k): int(g) for k, g in zip(keys, rs.randint(-1, 4, len(keys)))})
    return out


def host_route(D, I, key_map, judged, nh):
    """-> (seconds, labels, measures, negatives) of the first nh queries"""
    from convdr_amd.search import distinct_topk
    from tests import judge_cases as JC
    t0 = time.perf_counter()
    Dh, Ih, km = D[:nh].cpu().numpy(), I[:nh].cpu().numpy(), key_map.cpu().numpy()
    _, _, K, _ = distinct_topk(Dh, Ih, Ih.shape[1], km)
    lab = [JC.labels_of(K[j].tolist(), judged[j]) for j in range(nh)]
    meas = [JC.measures_of(lab[j], judged[j], CUTOFFS, 1) for j in range(nh)]
    neg = [JC.negatives_of(K[j].tolist(), judged[j], 20)[0] for j in range(nh)]
    return time.perf_counter() - t0, np.asarray(lab, np.int32), np.asarray(meas), neg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "judge_run_time.py measures on a GPU; there is no CPU fallback"
    from convdr_amd import judge
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    nq = args.nq
    say("# judge_run_time: %s; %d queries, corpus of %d rows, cutoffs %s" % (torch.cuda.get_device_name(0), nq, ROWS, CUTOFFS))
    say("# device: ms per call, median (min..max) of %d windows; host: one pass, seconds" % args.rounds)
    for n, nh in SHAPES:
        nh = nq if nh is None else min(nh, nq)
        D, I, key_map = search_output(nq, n, 3 + n)
        judged = judged_sets(I, key_map, 5 + n)
        q = judge.Qrels.from_dict(dict(enumerate(judged)), range(nq), device="cuda")
        K, labels, m = judge.judge_run(D, I, q, key_map=key_map, cutoffs=CUTOFFS)
        keys, _, counts = judge.run_negatives(K, labels, q, fill_to=20)
        host_s, lab_h, meas_h, neg_h = host_route(D, I, key_map, judged, nh)
        got_m, cnt = m.per_query[:nh].cpu().numpy(), counts[:nh].cpu().numpy()
        same = np.array_equal(labels[:nh].cpu().numpy(), lab_h) and all(
            keys[j, :cnt[j]].cpu().tolist() == neg_h[j] and cnt[j] == len(neg_h[j]) for j in range(nh))
        exact = [j for j, c in enumerate(m.columns) if not c.startswith(("map", "ndcg"))]
        same = same and np.array_equal(got_m[:, exact], meas_h[:, exact]) and np.allclose(got_m, meas_h, rtol=1e-9, atol=1e-12)
        if not same:
            say("(0) n=%d: the device route DIFFERS from the host route on the first %d queries: nothing timed" % (n, nh))
            return 1
        series = {"judge_run": [], "run_negatives": []}
        for _ in range(args.rounds):
            series["judge_run"].append(timed(lambda: judge.judge_run(D, I, q, key_map=key_map, cutoffs=CUTOFFS))[0])
            series["run_negatives"].append(timed(lambda: judge.run_negatives(K, labels, q, fill_to=20))[0])
        t0 = time.perf_counter()
        mean = m.mean()
        mean_ms = (time.perf_counter() - t0) * 1e3
        say("n=%d: (0) device == host on %d queries (labels, negatives bit for bit; measures as in the tests); num_q %d, "
            "recip_rank %.4f" % (n, nh, mean["num_q"], mean["recip_rank"]))
        for x, v in series.items():
            say("    device %-14s %9.3f ms (%.3f..%.3f)" % (x, statistics.median(v), min(v), max(v)))
        say("    device mean() host read %6.3f ms" % mean_ms)
        say("    host route (.cpu() copies, distinct_topk, oracle labels + measures + negatives): %.3f s for %d queries%s"
            % (host_s, nh, "" if nh == nq else " = %.1f s for %d (scaled)" % (host_s * nq / nh, nq)))
        del D, I, K, labels, keys, q
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
