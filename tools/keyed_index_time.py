#!/usr/bin/env python
"""Cost of the id operations of FlatIPIndex (remove_ids, id_filter, rows_of: a hash set of the listed ids built on the device,
probed by one pass over the id column) beside the route an index without an id column forces on its caller: copy the id table
to the host, np.isin against the list, hand the mask to remove_rows / row_filter.

(0) equality first: the id_filter bitmap must equal pack_row_mask(np.isin) word for word, and rows_of the host's first row
    and count.  A mismatch ends the run with exit status 1; nothing is timed.
(a) `--rows` x 768 resident (fp32 store), distinct ids.  Lists of 1 % and 50 % of the ids, as host int64 arrays (pids read
    from a file): wall-clock ms, median and min..max of `--rounds` calls, torch.cuda.synchronize() before and after.
      device   idx.remove_ids(list) / idx.id_filter(list): upload of the list, build, row pass, the one host read, and for
               remove_ids the compaction of every buffer
      host     mask = np.isin(idx_ids.cpu().numpy(), list); idx.remove_rows(mask) / idx.row_filter(mask)
    Between rounds of remove_ids the row count and the id column are put back; the rows' contents do not matter to the time.
(b) rows_of for 1,000 and 100,000 ids (device: enqueued, timed to completion) beside a host route to the same answer: a stable
    argsort of the table's host copy and two searchsorted.

  python tools/keyed_index_time.py [--out profiles/keyed_index_time.txt] [--rows 1000000]

No bar is set: the figures are written down as they come."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

D = 768


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(ts):
    return "%9.3f ms (%.3f..%.3f)" % (statistics.median(ts), min(ts), max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "keyed_index_time.py measures on a GPU; there is no CPU fallback"
    from convdr_amd.search import FlatIPIndex, pack_row_mask
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    n = args.rows
    rs = np.random.RandomState(0)
    ids = rs.permutation(n).astype(np.int64) * 7919 - 3_000_000_000
    g = torch.Generator(device="cuda").manual_seed(0)
    idx = FlatIPIndex(D, precision="auto", prepin=False)
    idx.reserve(n)
    idx.add(torch.randn((n, D), generator=g, device="cuda"), ids=ids)
    ids_d = idx.ids.clone()
    say("# keyed_index_time: %s; %d x %d rows, fp32 store, distinct int64 ids" % (torch.cuda.get_device_name(0), n, D))

    def put_back():
        idx._n = n
        idx._sid[:n].copy_(ids_d)

    lists = [("%g %% of the ids" % (100 * frac), np.concatenate([rs.choice(ids, size=int(n * frac) - 50, replace=False),
                                                                  np.arange(50, dtype=np.int64) * 7919 + 1]))
             for frac in (0.01, 0.5)]
    # (0) equality
    for name, lst in lists:
        mask = np.isin(ids, lst)
        f = idx.id_filter(lst)
        if f.n_allowed != int(mask.sum()) or not torch.equal(f.bits.cpu(), pack_row_mask(torch.as_tensor(mask))):
            say("MISMATCH: id_filter, list of %s" % name)
            return 1
    order = np.argsort(ids, kind="stable")
    for m in (1000, 100000):
        lst = lists[1][1][:m]
        first, count = idx.rows_of(lst)
        lo, hi = np.searchsorted(ids[order], lst, "left"), np.searchsorted(ids[order], lst, "right")
        want = np.where(hi > lo, order[np.minimum(lo, n - 1)], -1)
        if not np.array_equal(first.cpu().numpy(), want) or not np.array_equal(count.cpu().numpy(), hi - lo):
            say("MISMATCH: rows_of, %d ids" % m)
            return 1
    say("(0) id_filter == pack_row_mask(np.isin) word for word for both lists; rows_of == the host's first row and count")
    say("# (a) wall-clock ms per call: median (min..max) of %d calls" % args.rounds)
    for name, lst in lists:
        say("list of %s (%d ids, 50 of them on no row)" % (name, lst.size))
        dev, host = [], []
        for _ in range(args.rounds):
            dev.append(wall(lambda: idx.id_filter(lst))[0])
            host.append(wall(lambda: idx.row_filter(np.isin(idx.ids.cpu().numpy(), lst)))[0])
        say("    id_filter   device %s     host np.isin + row_filter  %s" % (fmt(dev), fmt(host)))
        dev, host = [], []
        for _ in range(args.rounds):
            t, removed = wall(lambda: idx.remove_ids(lst))
            dev.append(t)
            put_back()
            t, removed_h = wall(lambda: idx.remove_rows(np.isin(idx.ids.cpu().numpy(), lst)))
            host.append(t)
            put_back()
            assert removed == removed_h == lst.size - 50
        say("    remove_ids  device %s     host np.isin + remove_rows %s" % (fmt(dev), fmt(host)))
    say("# (b) rows_of, wall-clock ms to completion")
    for m in (1000, 100000):
        lst = lists[1][1][:m]
        dev, host = [], []

        def host_route():
            tab = idx.ids.cpu().numpy()
            o = np.argsort(tab, kind="stable")
            s = tab[o]
            return np.searchsorted(s, lst, "left"), np.searchsorted(s, lst, "right")
        for _ in range(args.rounds):
            dev.append(wall(lambda: idx.rows_of(lst))[0])
            host.append(wall(host_route)[0])
        say("    rows_of %6d ids   device %s     host argsort + searchsorted %s" % (m, fmt(dev), fmt(host)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
