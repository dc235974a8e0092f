#!/usr/bin/env python
"""Cost of the exact rank of given rows (FlatIPIndex.rank_rows_tensors, the band-count scan) on one GPU, beside the route the
README used to advertise for it: range_count at the target's score.

(0) equality first.  On a 20,000-row sub-sample, both stores, the ranks and scores of targets at ranks 10 / 1,000 / 5,000 /
    10,000 are compared with the definition over oracle.search.canonical_scores (bit for bit).  At the full shape every rank is
    bracketed by two range_count calls on the same tree: #{X > up(X_t)} <= rank <= #{X > down(X_t)} - 1 with up / down the
    neighbouring fp32 values of the target's fp64 score (the two agree unless another row's score falls within one fp32 ulp of
    the target's: untied data).  A mismatch ends the run with exit status 1; nothing is timed.
(a) `--rows` x 768 resident, `--pairs` (default 100 and 1,000) (query, target) pairs, both storages.  The target of a query is
    the row at rank r of a prior fp32 scoring pass (torch matmul + sort; the exact rank it lands on is whatever rank_rows says:
    within a few places), r = 10, 1,000, 100,000 and 500,000.  Per round one window each of rank_rows_tensors(Q, t) and
    range_count(Q, fp32 score of t), alternated in one process; medians and min..max of `--rounds` windows (3 when one call
    takes more than a second).  Device events around the whole call (every host read of the ladders inside).  A second,
    profiled pass reports the spans of one rank call (convdr_prof_collect: ip_scan_band, ip_rank_rescore, ip_rank_finish).

  python tools/rank_rows_time.py [--out profiles/rank_rows_time.txt] [--rows 1000000]

No ratio is fixed in advance: the figures are written down."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

D = 768
RANKS = (10, 1000, 100000, 500000)
SPANS = ("ip_scan_band", "ip_rank_rescore", "ip_rank_finish")


def corpus(n, nq, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    P = torch.randn((n, D), generator=g, device="cuda").half().float()      # both stores hold the same corpus
    Q = torch.randn((nq, D), generator=g, device="cuda")
    return P, Q


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


def rows_at_ranks(P, Q, ranks, chunk=25):
    """int64 [nq, len(ranks)]: the row at (about) each rank, from fp32 scores"""
    out = []
    r = torch.as_tensor(ranks, device=P.device)
    for a in range(0, Q.shape[0], chunk):
        order = torch.argsort(Q[a:a + chunk] @ P.T, dim=1, descending=True)
        out.append(order[:, r])
        del order
    return torch.cat(out).contiguous()


def fp32_neighbours(x):
    """(largest fp32 <= x, smallest fp32 >= x) of an fp64 tensor"""
    f = x.float()
    inf = torch.full_like(f, float("inf"))
    dn = torch.where(f.double() > x, torch.nextafter(f, -inf), f)
    up = torch.where(f.double() < x, torch.nextafter(f, inf), f)
    return dn, up


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rank_rows_time.py measures on a GPU; there is no CPU fallback"
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
    say("# rank_rows_time: %s; %d x %d rows" % (torch.cuda.get_device_name(0), n, D))

    # ---- (0) equality on a sub-sample, against the definition --------------------------------------------------------------
    P, Q = corpus(20000, 16, 11)
    S = OS.canonical_scores(Q.cpu().numpy(), P.cpu().numpy())
    sub_ranks = [10, 1000, 5000, 10000]
    order = np.stack([np.lexsort((np.arange(20000), -S[j])) for j in range(16)])
    rows = np.ascontiguousarray(order[:, sub_ranks])
    for storage in ("fp32", "fp16"):
        idx = index(storage, P)
        got = idx.rank_rows(Q, rows)
        X = idx.score_rows_tensors(Q, rows)[1].cpu().numpy()
        if not (np.array_equal(got, np.tile(sub_ranks, (16, 1))) and np.array_equal(X.view(np.uint64),
                                                                                   np.take_along_axis(S, rows, 1).view(np.uint64))):
            say("(0) %s store, 20000 x 16: rank_rows / score_rows DIFFER FROM THE DEFINITION over the oracle's scores: nothing timed" % storage)
            return 1
    say("(0) sub-sample 20000 rows x 16 queries, targets at ranks %s, both stores: ranks == the definition over the oracle's "
        "canonical scores, scores bit for bit" % (sub_ranks,))
    del P, Q, S, idx

    # ---- (a) the full shape ------------------------------------------------------------------------------------------------
    say("# (a) ms per call, medians of interleaved windows (rank_rows_tensors, range_count); spans of one profiled rank call in ms "
        "(launches)")
    for storage in ("fp32", "fp16"):
        P, _ = corpus(n, 1, 23)
        idx = index(storage, P)
        ranks = [r for r in RANKS if r < n]
        for npairs in args.pairs:
            Q = corpus(1, npairs, 29)[1]
            targets = rows_at_ranks(P, Q, ranks)
            for c, r in enumerate(ranks):
                t = targets[:, c].contiguous()
                rank = idx.rank_rows_tensors(Q, t)
                torch.cuda.synchronize()
                st = dict(idx.stats)
                X = idx.score_rows_tensors(Q, t)[1]
                dn, up = fp32_neighbours(X)
                lo = torch.as_tensor(idx.range_count(Q, up), device="cuda")
                hi = torch.as_tensor(idx.range_count(Q, dn), device="cuda") - (X > dn.double()).long()
                if not bool(((lo <= rank) & (rank <= hi)).all()):
                    say("(a) %s store pairs=%d rank ~%d: rank_rows is OUTSIDE the bracket of range_count: not timed" % (storage, npairs, r))
                    return 1
                rad = X.float()
                kinds = {"rank_rows": lambda: idx.rank_rows_tensors(Q, t), "range_count": lambda: idx.range_count(Q, rad)}
                first = {x: timed(fn)[0] for x, fn in kinds.items()}
                rounds = 3 if max(first.values()) > 1000.0 else args.rounds
                series = {x: [] for x in kinds}
                for _ in range(rounds):
                    for x, fn in kinds.items():
                        series[x].append(timed(fn)[0])
                _lib.lib().convdr_prof_enable(1)
                idx.rank_rows_tensors(Q, t)
                torch.cuda.synchronize()
                spans = {x: _lib.prof_collect(x) for x in SPANS}
                _lib.lib().convdr_prof_enable(0)
                med = {x: statistics.median(v) for x, v in series.items()}
                say("%s store pairs=%d rank ~%d (exact ranks %d..%d; %d of %d pinned by the bracket lo == hi):"
                    % (storage, npairs, r, int(rank.min()), int(rank.max()), int((lo == hi).sum()), npairs))
                for x in kinds:
                    say("    %-12s %10.3f ms (min..max %.3f..%.3f of %d windows)" % (x, med[x], min(series[x]), max(series[x]), rounds))
                say("    range_count / rank_rows = %.2f; rank ladder: rounds %d cap %d band rows %d above %d fallback %d; spans %s"
                    % (med["range_count"] / med["rank_rows"], st["rank_rounds"], st["rank_cap"], st["rank_band_rows"], st["rank_above"],
                       st["rank_fallback_pairs"], ", ".join("%s %.3f (%d)" % (x, spans[x][0], spans[x][1]) for x in SPANS)))
            del Q, targets
        del idx, P
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
