#!/usr/bin/env python
"""Cost of the exact DOCUMENT rank (FlatIPIndex.rank_ids_tensors: the marking band scan) on one GPU, beside the two routes
that existed before it.

(0) equality first.  On a 20,000-row sub-sample (5,000 documents of 4 chunk rows), both stores, the ranks of documents whose
    best rows sit near row ranks 10 / 1,000 / 5,000 / 10,000 are compared with the oracle of tests/doc_rank_cases.py over
    oracle.search.canonical_scores, and doc_ordinals with its numpy oracle.  A mismatch ends the run with exit status 1;
    nothing is timed.
(a) `--rows` x 768 resident, rows r // 4 share an id (250,000 documents of 4 chunk rows at 1 M), `--pairs` (query, document)
    pairs, both stores.  The document of a query is the one that holds the row at rank r of a prior fp32 scoring pass, r = 10,
    1,000 and 100,000 (its best row may stand a little higher: the exact row ranks are printed).  Timed, device events around
    the whole call (every host read inside), medians of `--rounds` windows alternated in one process:
      doc_ordinals()                                   the query-independent pass
      rank_ids_tensors(Q, ids)                         ordinals built inside the call
      rank_ids_tensors(Q, ids, ordinals=o)             precomputed ordinals
      rank_rows_tensors(Q, best rows)                  the same scan WITHOUT marks: the difference prices the marks
                                                       (and the best-row pass of score_ids_tensors that precedes them)
      host route                                       range_search_tensors just below the document's score -> ids -> a
                                                       distinct count per query with torch.unique (what the README described)
    and the spans of one profiled rank_ids call (convdr_prof_collect).  The shader clock is read while rank_ids runs back to
    back.  The host route's counts are compared with the ranks (they agree unless another row's score falls within one fp32
    ulp below the target's: the radius is an fp32 value); the number of agreeing pairs is printed.

  python tools/doc_rank_time.py [--out profiles/doc_rank_time.txt] [--rows 1000000]

No figure is fixed in advance: what comes out is written down, including any depth at which the device route loses."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from tools.doc_ops_time import clock_under_load, span      # noqa: E402
from tools.rank_rows_time import corpus, rows_at_ranks      # noqa: E402

D, CHUNKS = 768, 4
RANKS = (10, 1000, 100000)
SPANS = ("ip_score_docs", "doc_ordinals", "ip_scan_mark", "ip_rank_rescore", "ip_docrank_finish")


def index(storage, P, ids):
    from convdr_amd.search import FlatIPIndex
    idx = FlatIPIndex(D, storage=storage, precision="auto", prepin=False)
    idx.add(P.half() if storage == "fp16" else P.clone(), ids=ids)
    return idx


def host_route(idx, Q, X):
    """documents with a row scoring above the largest fp32 below X[q], per query, the target's own document included"""
    f = X.float()
    rad = torch.where(f.double() < X, f, torch.nextafter(f, torch.full_like(f, float("-inf"))))
    lims, _, I = idx.range_search_tensors(Q, rad)
    nq = int(Q.shape[0])
    qrep = torch.repeat_interleave(torch.arange(nq, device=I.device), torch.diff(lims))
    uniq, inv = torch.unique(idx.ids[I], return_inverse=True)
    nd = max(int(uniq.numel()), 1)
    return torch.bincount(torch.unique(qrep * nd + inv) // nd, minlength=nq)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "doc_rank_time.py measures on a GPU; there is no CPU fallback"
    from convdr_amd import _lib
    from oracle import search as OS
    from tests import doc_rank_cases as RC
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    n = args.rows
    say("# doc_rank_time: %s; %d x %d rows, %d documents of %d chunk rows" % (torch.cuda.get_device_name(0), n, D, n // CHUNKS, CHUNKS))

    # ---- (0) equality on a sub-sample, against the oracle --------------------------------------------------------------------
    ns = 20000
    P, Q = corpus(ns, 16, 11)
    col = (np.arange(ns, dtype=np.int64) // CHUNKS) * 7 - 5
    S = OS.canonical_scores(Q.cpu().numpy(), P.cpu().numpy())
    sub_ranks = [10, 1000, 5000, 10000]
    order = np.stack([np.lexsort((np.arange(ns), -S[j])) for j in range(16)])
    ids = col[order[:, sub_ranks]]
    want = RC.ranks(S, col, ids)
    for storage in ("fp32", "fp16"):
        idx = index(storage, P, col)
        o = idx.doc_ordinals()
        if not (np.array_equal(o.ord.cpu().numpy().view(np.uint32), RC.ordinals(col)[0]) and o.ndocs == ns // CHUNKS
                and np.array_equal(idx.rank_ids(Q, ids, ordinals=o), want)):
            say("(0) %s store, %d x 16: doc_ordinals / rank_ids DIFFER FROM THE ORACLE: nothing timed" % (storage, ns))
            return 1
    say("(0) sub-sample %d rows x 16 queries, documents around row ranks %s, both stores: doc_ordinals and rank_ids == the oracle "
        "(document ranks %d..%d)" % (ns, sub_ranks, int(want.min()), int(want.max())))
    del P, Q, S, idx

    # ---- (a) the full shape ------------------------------------------------------------------------------------------------
    say("# (a) ms per call, medians (min..max) of %d alternated windows; spans of one profiled rank_ids call in ms (launches)" % args.rounds)
    col = (torch.arange(n, device="cuda") // CHUNKS) * 7 - 5
    for storage in ("fp32", "fp16"):
        P, _ = corpus(n, 1, 23)
        idx = index(storage, P, col)
        ranks = [r for r in RANKS if r < n]
        ts = [span(idx.doc_ordinals)[0] for _ in range(args.rounds + 1)][1:]
        o = idx.doc_ordinals()
        say("%s store doc_ordinals(): %.3f ms (%.3f..%.3f); ndocs %d; key set + scan workspace %.1f MB"
            % (storage, statistics.median(ts), min(ts), max(ts), o.ndocs, _lib.lib().convdr_doc_ordinals_workspace_bytes(n) / 1e6))
        for npairs in args.pairs:
            Q = corpus(1, npairs, 29)[1]
            targets = rows_at_ranks(P, Q, ranks)
            for c, r in enumerate(ranks):
                ids = col[targets[:, c]].contiguous()
                rank, _, R = idx.rank_ids_tensors(Q, ids, ordinals=o)
                torch.cuda.synchronize()
                st = dict(idx.stats)
                X = idx.score_rows_tensors(Q, R)[1]
                rr = idx.rank_rows_tensors(Q, R)
                kinds = {"rank_ids": lambda: idx.rank_ids_tensors(Q, ids), "rank_ids(ordinals=)": lambda: idx.rank_ids_tensors(Q, ids, ordinals=o),
                         "rank_rows(best rows)": lambda: idx.rank_rows_tensors(Q, R), "host route": lambda: host_route(idx, Q, X)}
                first = {x: span(fn) for x, fn in kinds.items()}
                agree = int((first["host route"][1] - 1 == rank).sum())
                rounds = 3 if max(v[0] for v in first.values()) > 1000.0 else args.rounds
                series = {x: [] for x in kinds}
                for _ in range(rounds):
                    for x, fn in kinds.items():
                        series[x].append(span(fn)[0])
                _lib.lib().convdr_prof_enable(1)
                idx.rank_ids_tensors(Q, ids, ordinals=o)
                torch.cuda.synchronize()
                spans = {x: _lib.prof_collect(x) for x in SPANS}
                _lib.lib().convdr_prof_enable(0)
                mhz = clock_under_load(kinds["rank_ids(ordinals=)"], seconds=1.0)
                med = {x: statistics.median(v) for x, v in series.items()}
                say("%s store pairs=%d row rank ~%d (best rows at row ranks %d..%d, median %d; document ranks %d..%d, median %d):"
                    % (storage, npairs, r, int(rr.min()), int(rr.max()), int(rr.median()), int(rank.min()), int(rank.max()), int(rank.median())))
                for x in kinds:
                    say("    %-22s %10.3f ms (min..max %.3f..%.3f of %d windows)" % (x, med[x], min(series[x]), max(series[x]), rounds))
                say("    marks = rank_ids(ordinals=) - rank_rows = %.3f ms; host route / rank_ids(ordinals=) = %.2f; host route == rank for "
                    "%d of %d pairs; shader clock %s" % (med["rank_ids(ordinals=)"] - med["rank_rows(best rows)"],
                                                        med["host route"] / med["rank_ids(ordinals=)"], agree, npairs,
                                                        "%d MHz (rocm-smi)" % mhz if mhz else "not readable"))
                say("    ladder: rounds %d cap %d band rows %d rows marked %d fallback %d; spans %s"
                    % (st["rank_rounds"], st["rank_cap"], st["rank_band_rows"], st["rank_above"], st["rank_fallback_pairs"],
                       ", ".join("%s %.3f (%d)" % (x, spans[x][0], spans[x][1]) for x in SPANS)))
            del Q, targets
        del idx, P
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
