#!/usr/bin/env python
"""Cost of the half-precision passage store (FlatIPIndex(storage="fp16")) against the fp32 store, in one process on one GPU.

(0) equality first: on a sub-sample of rows the half store's result is compared with the oracle's on the widened halves
    (oracle.search.flat_ip_search), and at the full shape with the fp32 store built from the SAME widened halves -- two exact
    searches of one corpus must return the same bytes.  A mismatch ends the run with exit status 1; nothing is timed.
(a) add from a block file: `--rows` x 768, fp32 store from an fp32 file against half store from a float16 file (the files are
    written by this tool right before, so they come out of the page cache: the figure is the loader + PCIe + the device
    pass, not a disk).  Wall time of add() + synchronize, GB/s of the file's payload, alternating windows.
(b) resident search: `--queries` x `--rows`, top-100, fp32 store (precision="auto") against half store ("auto"), on Gaussian
    rows and on the clustered construction (0.9 c + 0.12 noise).  Device events around the whole search; rounds of three
    windows -- fp32, half, fp32 again -- "spread" is the distance between the two fp32 medians.
(c) device bytes held by each index (its tensors without the search workspace, and the workspace).

  python tools/half_store_time.py [--out profiles/half_store_time.txt] [--rows 1000000] [--queries 1000]

No verdict is fixed in advance."""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

D, K = 768, 100


def corpus(kind, n, nq, seed):
    """device fp32 rows and queries; the rows are ROUNDED TO HALF AND WIDENED, so both stores hold the same corpus"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "gaussian":
        P = torch.randn((n, D), generator=g, device="cuda")
        Q = torch.randn((nq, D), generator=g, device="cuda")
    else:
        c = torch.randn((1, D), generator=g, device="cuda")
        P = 0.9 * c + 0.12 * torch.randn((n, D), generator=g, device="cuda")
        Q = 0.9 * c + 0.12 * torch.randn((nq, D), generator=g, device="cuda")
    return P.half().float(), Q


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def held_bytes(idx):
    own = sum(t.numel() * t.element_size() for name, t in vars(idx).items()
              if isinstance(t, torch.Tensor) and t.is_cuda and name != "_ws" and t._base is None)
    return own, (idx._ws.numel() if idx._ws is not None else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "half_store_time.py measures on a GPU; there is no CPU fallback"
    from convdr_amd import blocks
    from convdr_amd.search import FlatIPIndex
    from oracle import search as OS
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    n, nq = args.rows, args.queries
    say("# half_store_time: %s; %d x %d rows, %d queries, top-%d" % (torch.cuda.get_device_name(0), n, D, nq, K))

    # ---- (0) equality ---------------------------------------------------------------------------------------------------------
    for kind in ("gaussian", "clustered"):
        P, Q = corpus(kind, 20000, 16, 11)
        h = FlatIPIndex(D, storage="fp16", prepin=False)
        h.add(P.half())
        Dh, Ih = h.search(Q.cpu().numpy(), K)
        Dr, Ir = OS.flat_ip_search(Q.cpu().numpy(), P.cpu().numpy(), K)
        if not (np.array_equal(Ih, Ir) and np.array_equal(Dh, Dr)):
            say("(0) %s sub-sample 20000 x 16: HALF STORE DIFFERS FROM THE ORACLE: nothing timed" % kind)
            return 1
        say("(0) %s sub-sample 20000 rows x 16 queries: half store == oracle on the widened halves (D and I, bit for bit)" % kind)
        del h, P, Q

    # ---- (b) resident search, (c) bytes -----------------------------------------------------------------------------------------
    say("# (b) resident search, ms per search (device events around the whole call, certificates read); rounds of (fp32, half, fp32)")
    held = None
    for kind in ("gaussian", "clustered"):
        P, Q = corpus(kind, n, nq, 23)
        f = FlatIPIndex(D, precision="auto", prepin=False)
        f.add(P.clone())
        h = FlatIPIndex(D, storage="fp16", precision="auto", prepin=False)
        h.add(P.half())
        del P
        (Df, If), (Dh, Ih) = f.search_tensors(Q, K), h.search_tensors(Q, K)
        torch.cuda.synchronize()
        if not (torch.equal(Df.view(torch.int32), Dh.view(torch.int32)) and torch.equal(If, Ih)):
            say("(b) %s: THE TWO STORES DISAGREE on the same corpus: not timed" % kind)
            return 1
        series = {"fp32": [], "half": [], "fp32b": []}
        stats = {}
        for _ in range(args.rounds):
            for name, idx in (("fp32", f), ("half", h), ("fp32b", f)):
                series[name].append(timed(lambda: idx.search_tensors(Q, K))[0])
                stats[name] = dict(idx.stats)
        med = {m: statistics.median(v) for m, v in series.items()}

        def ladder(st):
            return "retried %d, x2 %d, x3 %d, exhaustive %d, rounds %d" % (st["retried"], st.get("x2_queries", 0), st["x3_queries"],
                                                                          st.get("exhaustive_queries", 0), st["rounds"])
        say("%-9s results equal; fp32 store %.2f  again %.2f  spread %.2f  half store %.2f  (half/fp32 %.2fx; min..max fp32 "
            "%.2f..%.2f, half %.2f..%.2f)" % (kind, med["fp32"], med["fp32b"], abs(med["fp32"] - med["fp32b"]), med["half"],
                                              med["half"] / med["fp32"], min(series["fp32"] + series["fp32b"]),
                                              max(series["fp32"] + series["fp32b"]), min(series["half"]), max(series["half"])))
        say("          fp32 store: %s;  half store: %s" % (ladder(stats["fp32"]), ladder(stats["half"])))
        if held is None:
            held = (held_bytes(f), held_bytes(h))
        del f, h, Q
        torch.cuda.empty_cache()
    say("# (c) device bytes held by an index of %d rows (its tensors; the search workspace of %d queries beside them)" % (n, nq))
    for name, (own, ws) in zip(("fp32 store", "half store"), held):
        say("%s: %d bytes = %.1f per row  (+ workspace %d)" % (name, own, own / n, ws))

    # ---- (a) add from a block file ------------------------------------------------------------------------------------------------
    say("# (a) add(BlockView) + synchronize from a block file in the page cache, wall seconds; rounds of (fp32, half, fp32)")
    with tempfile.TemporaryDirectory() as td:
        P, _ = corpus("gaussian", n, 1, 31)
        p32, p16 = os.path.join(td, "emb32.pb"), os.path.join(td, "emb16.pb")
        host = P.cpu().numpy()
        blocks.dump_block(p32, host)
        blocks.dump_block(p16, host.astype(np.float16))
        del P, host
        torch.cuda.empty_cache()
        f = FlatIPIndex(D, precision="auto")
        h = FlatIPIndex(D, storage="fp16")
        f.prepin_staging(wait=True)
        series = {"fp32": [], "half": [], "fp32b": []}
        nbytes = {}

        def load(idx, path):
            idx.reset()
            with blocks.BlockView(path) as view:
                t0 = time.perf_counter()
                idx.add(view)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, int(view.array.nbytes)
        load(f, p32), load(h, p16)                     # warm-up: storage allocated, staging pinned
        f.reserve(n), h.reserve(n)
        for _ in range(args.rounds):
            for name, idx, path in (("fp32", f, p32), ("half", h, p16), ("fp32b", f, p32)):
                s, nbytes[name] = load(idx, path)
                series[name].append(s)
        med = {m: statistics.median(v) for m, v in series.items()}
        say("fp32 file -> fp32 store %.3f s (%.1f GB/s of %.2f GB)  again %.3f  spread %.3f;  float16 file -> half store %.3f s "
            "(%.1f GB/s of %.2f GB; %.2fx the fp32 time; min..max fp32 %.3f..%.3f, half %.3f..%.3f)"
            % (med["fp32"], nbytes["fp32"] / med["fp32"] / 1e9, nbytes["fp32"] / 1e9, med["fp32b"], abs(med["fp32"] - med["fp32b"]),
               med["half"], nbytes["half"] / med["half"] / 1e9, nbytes["half"] / 1e9, med["half"] / med["fp32"],
               min(series["fp32"] + series["fp32b"]), max(series["fp32"] + series["fp32b"]), min(series["half"]), max(series["half"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
