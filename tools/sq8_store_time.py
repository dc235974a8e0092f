#!/usr/bin/env python
"""Cost of the 8-bit passage store (FlatIPIndex(storage="sq8")) against the half store, in one process on one GPU.

(0) equality first: on a sub-sample each store's result is compared with the oracle over the rows it holds
    (oracle.search.flat_ip_search over reconstruct_n).  A mismatch ends the run with exit status 1; nothing is timed.
(a) add of `--rows` x 768 device rows into a reserved index -- the half store reads fp16 rows (converted before the clock
    starts), the sq8 store fp32 rows --: device events around add(), GB/s of that input.
(b) device bytes held by each index (its tensors without the search workspace).
(c) resident search, top-100, nq in `--queries`: hipEvent medians of `--reps` around search_tensors, the two stores
    INTERLEAVED (half, sq8, half again: "spread" is the distance between the two half medians), the shader clock under each
    store's load, and the share of a search that is its scan kernels (the library's ip_scan_emit + ip_scan_sample spans).
(d) information: the overlap at 100 of the sq8 store's top-k with the fp32 store's on the same rows.

  python tools/sq8_store_time.py [--out profiles/sq8_store_time.txt] [--rows 1000000] [--stores fp16,sq8]

`--stores fp16` times the half store alone (the form that also runs on a tree without the 8-bit store: the A/A of the half
store's search against a parent commit).  No verdict is fixed in advance."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from tools.doc_ops_time import clock_under_load          # noqa: E402

D, K = 768, 100
NAMES = {"fp16": "half store", "sq8": "sq8 store"}


def corpus(n, nq, seed):
    """device fp32 rows with per-column spreads over a factor of ~3 and a common component, and queries"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    spread = torch.exp(torch.rand(D, generator=g, device="cuda") * 1.1 - 0.55)
    P = torch.randn((n, D), generator=g, device="cuda") * spread + 0.5 * torch.randn(D, generator=g, device="cuda")
    return P, torch.randn((nq, D), generator=g, device="cuda")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def med(fn, reps):
    fn()
    return statistics.median(timed(fn)[0] for _ in range(reps))


def held_bytes(idx):
    return sum(t.numel() * t.element_size() for name, t in vars(idx).items()
               if isinstance(t, torch.Tensor) and t.is_cuda and name != "_ws" and t._base is None)


def scan_share(idx, Q):
    """(scan ms, whole-search ms) of one search with the library's spans on"""
    from convdr_amd import _lib
    L = _lib.lib()
    idx.search_tensors(Q, K)
    torch.cuda.synchronize()
    L.convdr_prof_enable(1)
    try:
        total = timed(lambda: idx.search_tensors(Q, K))[0]
        scan = sum(_lib.prof_collect(name)[0] for name in ("ip_scan_emit", "ip_scan_sample"))
    finally:
        L.convdr_prof_enable(0)
    return scan, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", default="100,479,1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stores", default="fp16,sq8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sq8_store_time.py measures on a GPU; there is no CPU fallback"
    from convdr_amd.search import FlatIPIndex
    from oracle import search as OS
    stores = args.stores.split(",")
    nqs = [int(v) for v in args.queries.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def build(storage, P):
        idx = FlatIPIndex(D, storage=storage, prepin=False)
        idx.reserve(int(P.shape[0]))
        rows = P.half() if storage == "fp16" else P       # (converted OUTSIDE the timed region: the half store's add reads halves)
        ms, _ = timed(lambda: idx.add(rows))
        return idx, ms
    n = args.rows
    say("# sq8_store_time: %s; %d x %d rows, top-%d, stores %s, medians of %d" % (torch.cuda.get_device_name(0), n, D, K, stores, args.reps))

    # ---- (0) equality -----------------------------------------------------------------------------------------------------------
    P, Q = corpus(20000, 16, 11)
    for s in stores:
        idx, _ = build(s, P)
        Dg, Ig = idx.search(Q.cpu().numpy(), K)
        Dr, Ir = OS.flat_ip_search(Q.cpu().numpy(), idx.reconstruct_n(0, idx.ntotal), K)
        if not (np.array_equal(Ig, Ir) and np.array_equal(Dg, Dr)):
            say("(0) %s DIFFERS FROM THE ORACLE over its own rows: nothing timed" % NAMES[s])
            return 1
        say("(0) %s == oracle over its reconstructed rows (20000 rows x 16 queries, D and I bit for bit)" % NAMES[s])
        del idx
    del P, Q

    # ---- (a) add, (b) bytes -------------------------------------------------------------------------------------------------------
    P, Qall = corpus(n, max(nqs), 23)
    built = {}
    for s in stores:
        build(s, P[:4096])                          # warm-up of the kernels
        built[s], ms = build(s, P)
        extra = "" if s != "sq8" else "; saturated %d" % built[s].stats.get("sq8_saturated", 0)
        esz = 2 if s == "fp16" else 4
        say("(a) %-10s add of %d device %s rows: %.2f ms = %.1f GB/s of its input%s"
            % (NAMES[s], n, "fp16" if esz == 2 else "fp32", ms, n * D * esz / ms / 1e6, extra))
    for s in stores:
        own = held_bytes(built[s])
        say("(b) %-10s holds %d bytes = %.1f per row" % (NAMES[s], own, own / n))

    # ---- (d) overlap with the fp32 store (information) -----------------------------------------------------------------------------
    if "sq8" in stores:
        f = FlatIPIndex(D, prepin=False)
        f.add(P.clone())
        If = f.search_tensors(Qall[:100], K)[1]
        Iq = built["sq8"].search_tensors(Qall[:100], K)[1]
        ov = [len(set(a.tolist()) & set(b.tolist())) for a, b in zip(If.cpu(), Iq.cpu())]
        say("(d) overlap at %d of the sq8 store's top-k with the fp32 store's, 100 queries: mean %.1f, min %d, max %d"
            % (K, float(np.mean(ov)), min(ov), max(ov)))
        del f, If, Iq
    del P
    torch.cuda.empty_cache()

    # ---- (c) resident search ------------------------------------------------------------------------------------------------------
    say("# (c) ms per search_tensors (device events, certificates read); windows half, sq8, half again")
    for nq in nqs:
        Q = Qall[:nq].contiguous()
        order = [s for s in ("fp16", "sq8", "fp16") if s in stores]
        ms, clk, share, st = {}, {}, {}, {}
        for j, s in enumerate(order):
            key = s + ("b" if j == 2 else "")
            ms[key] = med(lambda: built[s].search_tensors(Q, K), args.reps)
            if j < 2:
                st[s] = dict(built[s].stats)
                clk[s] = clock_under_load(lambda: built[s].search_tensors(Q, K), seconds=1.0)
                share[s] = scan_share(built[s], Q)
        for s in stores:
            line = "nq=%-4d %-10s %.3f ms" % (nq, NAMES[s], ms[s])
            if s == "fp16" and "fp16b" in ms:
                line += "  again %.3f  spread %.3f" % (ms["fp16b"], abs(ms["fp16"] - ms["fp16b"]))
            if s == "sq8" and "fp16" in ms:
                line += "  (%.2fx the half store's)" % (ms["sq8"] / ms["fp16"])
            sc, tot = share[s]
            line += " | scan %.3f ms = %.0f %% of a %.3f ms search with spans on | shader clock %s | retried %d, rounds %d" % (
                sc, 100 * sc / tot, tot, "%d MHz" % clk[s] if clk[s] else "not readable", st[s]["retried"], st[s]["rounds"])
            if s == "sq8":
                line += ", first pass %d" % st[s].get("sq8_first_pass", -1)
            say(line)
        if "sq8" in stores and "fp16" in stores:
            say("nq=%-4d scan alone: sq8 %.3f ms against half %.3f ms = %.2fx" % (nq, share["sq8"][0], share["fp16"][0],
                                                                                 share["sq8"][0] / share["fp16"][0]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
