#!/usr/bin/env python
"""Cost of the exact range search (FlatIPIndex.range_search_tensors / range_count) on one GPU, beside the top-k search that
returns the same number of rows.

(0) equality first.  On a 20,000-row sub-sample the range search at the rank-100 radius is compared with the definition over
    oracle.search.canonical_scores (lims, D and I, bit for bit), both stores.  At the full shape every query's run must hold
    the leading rows of the top-k search it was derived from, in its order.  A mismatch ends the run with exit status 1; nothing
    is timed.
(a) `--rows` x 768 resident, `--queries` (default 100 and 1,000), both storages.  The radius of a query is the fp32 midpoint
    between its ranks m and m + 1, from a prior search at depth m + 8 (m = 100 and m = 5,000).  Per round one window each of
    search_tensors(Q, m), range_search_tensors(Q, radius), range_count(Q, radius), search_tensors again, interleaved; medians of
    `--rounds` windows; "spread" is the distance between the medians of the two top-k series.  Device events around the whole call
    (every host read of the ladder inside).  Where the result does not fit the first list (m >= cap = 4,096: every query overflows
    and is re-run once) a further series starts with a list that holds it.  A second, profiled pass reports the spans of one range search
    (convdr_prof_collect: ip_scan_emit, ip_range_rescore, ip_range_select).

  python tools/range_search_time.py [--out profiles/range_search_time.txt] [--rows 1000000]

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
RANKS = (100, 5000)
SPANS = ("ip_scan_emit", "ip_range_rescore", "ip_range_select")


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


def radius_at(idx, Q, m, extra=8):
    """(fp32 midpoint between ranks m and m + 1 per query, (D, I) of the top m + extra)"""
    Dk, Ik = idx.search_tensors(Q, m + extra)
    rad = (0.5 * (Dk[:, m - 1].double() + Dk[:, m].double())).float()
    return rad.contiguous(), (Dk, Ik)


def same_as_topk(lims, Dr, Ir, rad, Dk, Ik):
    """Is every query's run a prefix of its top-k list, of a length the fp32 scores allow?  Rounding to fp32 is monotone:
    D > radius implies a score above the radius, and a score above it implies D >= radius (two scores that round to one fp32
    value leave the length open by one)."""
    c = torch.diff(lims)
    lo, hi = (Dk > rad[:, None]).sum(1), (Dk >= rad[:, None]).sum(1)
    if int(hi.max()) >= Dk.shape[1] or not bool(((lo <= c) & (c <= hi)).all()):
        return False
    pre = torch.arange(Dk.shape[1], device=Dk.device)[None, :] < c[:, None]
    return torch.equal(Ik[pre], Ir) and torch.equal(Dk[pre].view(torch.int32), Dr.view(torch.int32))


def oracle_range(S, rad32):
    lims, Ds, Is = [0], [], []
    for j in range(S.shape[0]):
        keep = np.flatnonzero(S[j] > np.float64(rad32[j]))
        order = keep[np.lexsort((keep, -S[j, keep]))]
        Ds.append(S[j, order].astype(np.float32))
        Is.append(order)
        lims.append(lims[-1] + len(order))
    return np.asarray(lims, np.int64), np.concatenate(Ds), np.concatenate(Is).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "range_search_time.py measures on a GPU; there is no CPU fallback"
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
    say("# range_search_time: %s; %d x %d rows" % (torch.cuda.get_device_name(0), n, D))

    # ---- (0) equality on a sub-sample, against the definition --------------------------------------------------------------
    P, Q = corpus(20000, 16, 11)
    S = OS.canonical_scores(Q.cpu().numpy(), P.cpu().numpy())
    for storage in ("fp32", "fp16"):
        idx = index(storage, P)
        rad = radius_at(idx, Q, 100)[0]
        want = oracle_range(S, rad.cpu().numpy())
        got = idx.range_search(Q, rad)
        cnt = idx.range_count(Q, rad)
        if not (all(np.array_equal(a, b) for a, b in zip(got, want)) and np.array_equal(cnt, np.diff(want[0]))):
            say("(0) %s store, 20000 x 16, rank-100 radius: DIFFERS FROM THE DEFINITION over the oracle's scores: nothing timed" % storage)
            return 1
    say("(0) sub-sample 20000 rows x 16 queries, rank-100 radius, both stores: == the definition over the oracle's canonical scores "
        "(lims, D and I, bit for bit; range_count == diff(lims))")
    del P, Q, S, idx

    # ---- (a) the full shape ------------------------------------------------------------------------------------------------
    say("# (a) ms per call, medians of %d interleaved windows (top-k, range_search, range_count, top-k again); spans of one profiled "
        "range search in ms (launches)" % args.rounds)
    for storage in ("fp32", "fp16"):
        P, _ = corpus(n, 1, 23)
        idx = index(storage, P)
        del P
        for nq in args.queries:
            Q = corpus(1, nq, 29)[1]
            for m in RANKS:
                rad, (Dk, Ik) = radius_at(idx, Q, m)
                lims, Dr, Ir = idx.range_search_tensors(Q, rad)
                torch.cuda.synchronize()
                st = dict(idx.stats)
                if not same_as_topk(lims, Dr, Ir, rad, Dk, Ik):
                    say("(a) %s store nq=%d rank %d: the range search DIFFERS from the top-%d search it was derived from: not timed"
                        % (storage, nq, m, m))
                    return 1
                cnt = idx.range_count(Q, rad)
                if not np.array_equal(cnt, torch.diff(lims).cpu().numpy()):
                    say("(a) %s store nq=%d rank %d: range_count differs: not timed" % (storage, nq, m))
                    return 1
                kinds = {"top-k": lambda: idx.search_tensors(Q, m), "range_search": lambda: idx.range_search_tensors(Q, rad),
                         "range_count": lambda: idx.range_count(Q, rad), "top-k again": lambda: idx.search_tensors(Q, m)}
                if m >= idx.cap:        # the first list cannot hold the result: also with a first list that can (no second pass)
                    big = 1 << (2 * m - 1).bit_length()

                    def with_big_list(big=big):
                        old, idx.cap = idx.cap, big
                        try:
                            return idx.range_search_tensors(Q, rad)
                        finally:
                            idx.cap = old
                    kinds["range, cap=%d" % big] = with_big_list
                series = {x: [] for x in kinds}
                for _ in range(args.rounds):
                    for x, fn in kinds.items():
                        series[x].append(timed(fn)[0])
                _lib.lib().convdr_prof_enable(1)
                idx.range_search_tensors(Q, rad)
                torch.cuda.synchronize()
                spans = {x: _lib.prof_collect(x) for x in SPANS}
                _lib.lib().convdr_prof_enable(0)
                med = {x: statistics.median(v) for x, v in series.items()}
                say("%s store nq=%d rank %d: results equal the top-%d search; top-k %.3f  again %.3f  spread %.3f"
                    % (storage, nq, m, m, med["top-k"], med["top-k again"], abs(med["top-k"] - med["top-k again"])))
                for x in [k for k in kinds if k.startswith("range")]:
                    say("    %-16s %8.3f ms (%.2fx top-k; min..max %.3f..%.3f)" % (x, med[x], med[x] / med["top-k"], min(series[x]),
                                                                                  max(series[x])))
                say("    range ladder: rounds %d cap %d chunked %d; spans %s"
                    % (st["range_rounds"], st["range_cap"], st["range_chunked_queries"],
                       ", ".join("%s %.3f (%d)" % (x, spans[x][0], spans[x][1]) for x in SPANS)))
            del Q
        del idx
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
