#!/usr/bin/env python
"""Time of the query-encode loop (convdr_amd.inference.evaluate) per DataLoader batch against the same loop with a token
budget, on one GPU, in one process.

Model: roberta-base geometry, random N(0, 0.02) weights (`rdot_nll`).  Data: `--queries` synthetic queries, lengths uniform
in 16 .. 256 (the reference's max_concat_length), per_gpu_eval_batch_size = 4, every batch padded to its own width as the
reference's collate function does.

First the two routes must agree: per query, cosine >= 1 - 1e-4 between the budgeted and the per-batch embeddings (the bound
tests/test_encoder_gpu.py puts on batch-composition dependence).  Then `--rounds` rounds of three windows each -- per-batch,
budgeted, per-batch again -- one window being one whole evaluate() call between two device synchronises.  The second
per-batch series prices the noise: "spread" is the distance between the medians of the two per-batch series.

  python tools/evaluate_time.py [--out profiles/evaluate_coalesce_time.txt]

Verdict (exit status 1 when it fails): the budgeted median is shorter than the per-batch median by more than three times
the spread."""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402


class Queries(torch.utils.data.Dataset):
    def __init__(self, n, seed=0):
        rs = np.random.RandomState(seed)
        self.lens = rs.randint(16, 257, size=n)
        self.seqs = [np.concatenate([[0], rs.randint(3, 50000, size=m - 1)]).astype(np.int64) for m in self.lens]

    def __len__(self):
        return len(self.seqs)

    def __getitem__(self, i):
        return i

    def get_collate_fn(self, args, mode):
        def collate(idx):
            width = max(len(self.seqs[i]) for i in idx)
            ids, mask = np.zeros((len(idx), width), np.int64), np.zeros((len(idx), width), np.int64)
            for r, i in enumerate(idx):
                ids[r, :len(self.seqs[i])] = self.seqs[i]
                mask[r, :len(self.seqs[i])] = 1
            return {"qid": [str(i) for i in idx], "concat_ids": torch.from_numpy(ids), "concat_id_mask": torch.from_numpy(mask),
                    "history_utterances": [[] for _ in idx]}
        return collate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--budget", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "evaluate_time.py measures on a GPU; there is no CPU fallback"
    from convdr_amd import inference
    from convdr_amd.model.models import MSMarcoConfigDict, RobertaConfig
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    torch.manual_seed(0)
    model = MSMarcoConfigDict["rdot_nll"].model_class(RobertaConfig()).cuda().eval()
    data = Queries(a.queries)
    args = SimpleNamespace(per_gpu_eval_batch_size=4, n_gpu=1, device=torch.device("cuda"), seed=42)

    def run(budget):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = inference.evaluate(args, data, model, token_budget=budget)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    say("# evaluate_time: %s, %d queries of 16..256 tokens (%d tokens, %d packed rows), batch 4, %d rounds of (per-batch, budget %d, "
        "per-batch) evaluate() calls" % (torch.cuda.get_device_name(0), a.queries, int(data.lens.sum()),
                                         int(((data.lens + 7) // 8 * 8).sum()), a.rounds, a.budget))
    # agreement first (these two calls are also the warm-up of both routes)
    _, (e0, id0, _) = run(None)
    f0 = inference.last_evaluate_stats["forwards"]
    _, (e1, id1, _) = run(a.budget)
    st = dict(inference.last_evaluate_stats)
    assert id0 == id1 and st["padded_batches"] == 0
    cs = (e0 * e1).sum(1) / (np.linalg.norm(e0, axis=1) * np.linalg.norm(e1, axis=1))
    say("agreement: min cosine %.8f over %d queries (bar 1 - 1e-4); forwards %d per batch, %d with the budget"
        % (cs.min(), len(cs), f0, st["forwards"]))
    assert cs.min() >= 1 - 1e-4, "the budgeted and the per-batch embeddings differ"
    for b in (None, a.budget):
        run(b)
    series = {"batch": [], "budget": [], "batch2": []}
    for _ in range(a.rounds):
        for name, b in (("batch", None), ("budget", a.budget), ("batch2", None)):
            series[name].append(1e3 * run(b)[0])
    med = {n: statistics.median(v) for n, v in series.items()}
    spread = abs(med["batch"] - med["batch2"])
    good = med["budget"] < med["batch"] - 3 * spread
    qps = lambda ms: a.queries / (ms * 1e-3)
    say("per-batch %.2f ms (%.0f queries/s)  per-batch again %.2f ms  spread %.2f ms  budgeted %.2f ms (%.0f queries/s)  "
        "(budgeted/per-batch %.3f; min..max per-batch %.2f..%.2f, budgeted %.2f..%.2f)"
        % (med["batch"], qps(med["batch"]), med["batch2"], spread, med["budget"], qps(med["budget"]), med["budget"] / med["batch"],
           min(series["batch"] + series["batch2"]), max(series["batch"] + series["batch2"]), min(series["budget"]),
           max(series["budget"])))
    say("  -> %s (budgeted < per-batch - 3 x spread)%s"
        % ("PASS" if good else "FAIL", "" if good else ": no gain measured; the budget stays an opt-in without a recommendation"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
