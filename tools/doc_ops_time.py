#!/usr/bin/env python
"""Cost of the document operations of FlatIPIndex (rows_all: every row of every listed id as a CSR; score_ids_tensors: the
MaxP score and best row of (query, document) pairs) beside the route an index that knows rows only forces on its caller:
copy the id column to the host, a stable argsort and two searchsorted for the rows, score_rows_tensors on the padded row
list, a max.

Corpus: `--rows` x 768 resident, `--rows` / 4 documents of 4 chunk rows (the rows of a document follow one another, as the
encode loop writes them), in both storages.
(0) equality first: the device CSR must equal the host's, and the device (D, R) the host route's max and first argmax.  A
    mismatch ends the run with exit status 1; nothing is timed.
(a) rows_all of `--ids` ids (host int64 array, 50 of them on no row).
(b) score_ids_tensors for `--queries` queries x `--per-query` ids each (device int64 [nq, m], drawn with repeats across
    queries).
Both beside the host route, in the same process on the same box.  Times are hipEvent spans around the whole call (uploads,
launches, host reads and -- for the host route -- the host's own work lie inside the span), median and min..max of `--rounds`
calls after one warm-up call of each.

  python tools/doc_ops_time.py [--out profiles/doc_ops_time.txt] [--rows 1000000]

No bar is set: the figures are written down as they come."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

D, CHUNKS = 768, 4


def span(fn):
    """(ms between two events around fn(), its result)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def clock_under_load(fn, seconds=1.5):
    """median shader clock in MHz while fn() runs back to back (rocm-smi --showclocks read from a thread, as bench.py's
    power_under_load does); None when it cannot be read"""
    import json
    import re
    import subprocess
    import threading
    import time
    samples, stop = [], threading.Event()

    def poll():
        while not stop.is_set():
            try:
                r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--json"], capture_output=True, text=True, timeout=10)
                c = json.loads(r.stdout).get("card0", {})
                samples.extend(int(re.sub(r"\D", "", v)) for k, v in c.items() if k.lower().startswith("sclk clock speed"))
            except Exception:
                return
            stop.wait(0.05)
    th = threading.Thread(target=poll, daemon=True)
    t0 = time.perf_counter()
    th.start()
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()
    stop.set()
    th.join(timeout=12)
    return statistics.median(samples) if samples else None


def fmt(ts):
    return "%9.3f ms (%.3f..%.3f)" % (statistics.median(ts), min(ts), max(ts))


def host_table(idx):
    """the host's id -> rows map: the column's host copy, its stable argsort (rows ascend inside an id), the sorted ids"""
    tab = idx.ids.cpu().numpy()
    order = np.argsort(tab, kind="stable")
    return order, tab[order]


def host_rows_all(idx, lst):
    """(start, count, rows) by argsort + searchsorted; a repeated id would get its rows again (the timed lists have none)"""
    order, s = host_table(idx)
    lo, hi = np.searchsorted(s, lst, "left"), np.searchsorted(s, lst, "right")
    count = hi - lo
    start = np.cumsum(count) - count
    at = np.repeat(lo, count) + (np.arange(int(count.sum()), dtype=np.int64) - np.repeat(start, count))
    return start, count.astype(np.int32), order[at]


def host_score_ids(idx, Q, ids_d):
    """(D [nq, m]) by the row route: the padded [nq, m * CHUNKS] row list of the ids, score_rows_tensors, a max"""
    order, s = host_table(idx)
    ids = ids_d.cpu().numpy()
    nq, m = ids.shape
    lo, hi = np.searchsorted(s, ids.reshape(-1), "left"), np.searchsorted(s, ids.reshape(-1), "right")
    c = np.arange(CHUNKS, dtype=np.int64)
    at = lo[:, None] + c[None, :]
    rows = np.where(at < hi[:, None], order[np.minimum(at, len(order) - 1)], -1).reshape(nq, m * CHUNKS)
    Dr, _ = idx.score_rows_tensors(Q, torch.as_tensor(rows, device=Q.device))
    best, arg = Dr.reshape(nq, m, CHUNKS).max(dim=2)
    return best, torch.as_tensor(rows, device=Q.device).reshape(nq, m, CHUNKS).gather(2, arg[:, :, None])[:, :, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--ids", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--per-query", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "doc_ops_time.py measures on a GPU; there is no CPU fallback"
    from convdr_amd.search import FlatIPIndex
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    n = args.rows // CHUNKS * CHUNKS
    ndocs = n // CHUNKS
    rs = np.random.RandomState(0)
    docs = rs.permutation(ndocs).astype(np.int64) * 7919 - 3_000_000_000
    ids = np.repeat(docs, CHUNKS)
    absent = np.arange(50, dtype=np.int64) * 7919 + 1
    lst = np.concatenate([rs.choice(docs, size=min(args.ids, ndocs) - 50, replace=False), absent])
    rs.shuffle(lst)
    nq, m = args.queries, args.per_query
    say("# doc_ops_time: %s; %d x %d rows, %d documents of %d chunk rows; hipEvent spans, median (min..max) of %d calls after "
        "one warm-up" % (torch.cuda.get_device_name(0), n, D, ndocs, CHUNKS, args.rounds))
    for storage in ("fp32", "fp16"):
        g = torch.Generator(device="cuda").manual_seed(0)
        idx = FlatIPIndex(D, storage=storage, precision="auto", prepin=False)
        idx.reserve(n)
        X = torch.randn((n, D), generator=g, device="cuda")
        idx.add(X.half() if storage == "fp16" else X, ids=ids)
        del X
        Q = torch.randn((nq, D), generator=g, device="cuda")
        pair_ids = torch.as_tensor(np.concatenate([docs, absent])[rs.randint(0, ndocs + 50, size=(nq, m))], device="cuda")
        say("storage %s" % storage)
        # (0) equality (and the warm-up call of every route)
        start, count, rows = (t.cpu().numpy() for t in idx.rows_all(lst))
        hs, hc, hr = host_rows_all(idx, lst)
        if not (np.array_equal(count, hc) and np.array_equal(rows, hr) and np.array_equal(start[count > 0], hs[count > 0])):
            say("MISMATCH: rows_all")
            return 1
        Dd, Rd = idx.score_ids_tensors(Q, pair_ids)
        Dh, Rh = host_score_ids(idx, Q, pair_ids)
        # (the fp32 maximum is the rounding of the fp64 one; the row may differ only where two rows share an fp32 score)
        if not torch.equal(Dd, Dh) or int(((Rd != Rh) & (Rd >= 0)).sum()) > int((Rd >= 0).sum()) // 10000:
            say("MISMATCH: score_ids_tensors")
            return 1
        say("    (0) rows_all == the host's CSR (%d rows of %d ids); score_ids_tensors == the max over score_rows (%d pairs, "
            "%d on no row)" % (len(rows), lst.size, nq * m, int((Rd < 0).sum())))
        dev, host = [], []
        for _ in range(args.rounds):
            dev.append(span(lambda: idx.rows_all(lst))[0])
            host.append(span(lambda: host_rows_all(idx, lst))[0])
        say("    (a) rows_all %d ids                device %s     host ids.cpu + argsort + searchsorted %s"
            % (lst.size, fmt(dev), fmt(host)))
        dev, host = [], []
        for _ in range(args.rounds):
            dev.append(span(lambda: idx.score_ids_tensors(Q, pair_ids))[0])
            host.append(span(lambda: host_score_ids(idx, Q, pair_ids))[0])
        say("    (b) score_ids_tensors %d x %d ids   device %s     host row list + score_rows_tensors + max    %s"
            % (nq, m, fmt(dev), fmt(host)))
        mhz = clock_under_load(lambda: idx.score_ids_tensors(Q, pair_ids))
        say("    shader clock while score_ids_tensors runs back to back: %s" % ("%d MHz (rocm-smi)" % mhz if mhz else "not readable"))
        idx.release()
        del idx
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
