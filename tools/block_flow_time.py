#!/usr/bin/env python
"""The block-file flow of the reference (run_convdr_inference.py:157-242) alone: search_one_by_one over two block files of
`--rows` x 768 passages, `--queries` queries, top-100 -- the leg `bench.py --full` reports as search_one_by_one_files, without
the rest of that run.  The second file holds the first one's rows reversed, as in bench.py.

Prints one JSON line: per repetition the wall seconds end to end and the two stage times search_one_by_one reports
(load_add_s: file -> pinned staging -> H2D enqueue; search_finish_merge_s: certificates, merge, next first pass).  The first
repetition pins the staging buffers and is listed apart.

  python tools/block_flow_time.py [--dir DIR] [--reps 3] [--make-only]

--dir: keep the block files there (written when missing) so that several runs -- two builds of the package, say -- read the
same files; default is a temporary directory."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

D, K = 768, 100


def make(td, n, dev):
    from convdr_amd import blocks
    if os.path.exists(os.path.join(td, "done")):
        return
    host = torch.randn(n, D, device=dev, generator=torch.Generator(device=dev).manual_seed(0)).cpu().numpy()
    for b in range(2):
        rows = host if b == 0 else np.ascontiguousarray(host[::-1])
        blocks.dump_block(os.path.join(td, "passage__emb_p__data_obj_%d.pb" % b), rows)
        blocks.dump_block(os.path.join(td, "passage__embid_p__data_obj_%d.pb" % b), np.arange(b * n, (b + 1) * n, dtype=np.int64))
    open(os.path.join(td, "done"), "w").close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--make-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "block_flow_time.py measures on a GPU; there is no CPU fallback"
    from convdr_amd.search import FlatIPIndex, search_one_by_one
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        td = args.dir or tmp
        make(td, args.rows, dev)
        if args.make_only:
            return 0
        Qh = torch.randn(args.queries, D, device=dev, generator=torch.Generator(device=dev).manual_seed(1234)).cpu().numpy()
        runs = []
        for _ in range(args.reps + 1):
            tmg = {}
            gi = FlatIPIndex(D, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mD, mI = search_one_by_one(td, gi, Qh, K, timings=tmg)
            runs.append({"seconds": time.perf_counter() - t0, "load_add_s": tmg["load_add_s"],
                         "search_finish_merge_s": tmg["search_finish_merge_s"]})
            del gi
    print(json.dumps({"rows_per_block": args.rows, "queries": args.queries, "first": runs[0], "reps": runs[1:],
                      "best": min(runs[1:], key=lambda r: r["seconds"]), "checksum": [float(mD.sum()), int(mI.sum())]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
