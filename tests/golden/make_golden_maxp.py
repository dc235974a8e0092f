#!/usr/bin/env python3
"""Generate tests/golden/maxp.npz: the reference's own corpus-encode loop and search run with its MaxP model class
(``rdot_nll_multi_chunk``: one embedding per 512-token chunk).  Run in the build container only, like make_golden.py,
whose shims and helpers this script imports:

    python tests/golden/make_golden_maxp.py

Nothing of the reference's source is stored: the fixture holds inputs and recorded outputs.
  * weights      the tiny RoBERTa of encode_loop.npz (same architecture, same parameters: the MaxP class adds none).  They
                 are NOT stored a second time -- 1.8 MB of incompressible floats -- but loaded from encode_loop.npz here and
                 in the tests; ``weights_sha256`` pins them.
  * token cache  23 records of 1..1,024 tokens in a 1,024-wide cache; lengths 1, 512, 513 and 1,024 are among them.
  * emb / embid  what gen_passage_embeddings.StreamInferenceDoc wrote for them at batch size 8: two rows per record
                 (chunk-major inside every batch), the second one the encoder's output on all-pad input when the record
                 has at most 512 tokens.
  * queries      six vectors built from the reference's embeddings (see the comment in main()): the documents the tiny
                 encoder cannot tell apart tie exactly, the others are a unit of score apart, and the all-pad row scores
                 below every document's best live row -- the regime of the model's own MaxP, which keeps dead chunks out of
                 the maximum with a -9999 bias (models.py:100-107).  Where a dead row outscores a document's live rows the
                 reference ranks that document by its padding.
  * ref_D/ref_I  the reference's search_one_by_one over the block it wrote (all rows: topN = 46), and ``trec``, the text its
                 EvalDevQuery writes from them (first occurrence per pid, then (0, 0) padding).
"""
import contextlib
import hashlib
import io
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.make_golden import REF, FlatIPStandIn, import_reference, tiny_roberta_config   # noqa: E402

N, L, BASE, BATCH = 23, 1024, 512, 8
FIXED_LENS = (1, 512, 513, 1024, 2, 511, 514, 1023)


def weights_sha256(names, get):
    h = hashlib.sha256()
    for k in sorted(names):
        h.update(k.encode())
        h.update(np.ascontiguousarray(get(k)).tobytes())
    return h.hexdigest()


def main():
    import torch
    import torch.distributed as dist
    sys.argv = sys.argv[:1]
    M, U, DU, T = import_reference()
    sys.path.insert(0, os.path.join(REF, "drivers"))
    import gen_passage_embeddings as G
    import run_convdr_inference as R
    zw = np.load(os.path.join(HERE, "encode_loop.npz"))
    wnames = [k for k in zw.files if k.startswith("w/")]
    model = M.MSMarcoConfigDict["rdot_nll_multi_chunk"].model_class(tiny_roberta_config())
    model.load_state_dict({k[2:]: torch.from_numpy(zw[k]) for k in wnames}, strict=True)
    model.eval()
    assert model.base_len == BASE
    rng = np.random.RandomState(17)
    lens = rng.randint(1, L + 1, size=N)
    lens[[0, 3, 8, 9, 13, 16, 20, 22]] = FIXED_LENS              # spread over the three batches of 8
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "passages")
        with open(path, "wb") as f:           # byte layout of tokenizing.py:116 minus the 8-byte pid prefix (:44)
            for n in lens:
                ids = [0] + rng.randint(3, 200, size=n - 1).tolist()
                f.write(int(n).to_bytes(4, "big") + np.array((ids + [0] * L)[:L], np.int32).tobytes())
        with open(path + "_meta", "w") as f:
            json.dump({"type": "int32", "total_number": N, "embedding_size": L}, f)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29572")
        dist.init_process_group("gloo", rank=0, world_size=1)
        out_dir = os.path.join(td, "out")
        args = types.SimpleNamespace(per_gpu_eval_batch_size=BATCH, local_rank=0, rank=0, world_size=1,
                                     device=torch.device("cpu"), output_dir=out_dir, max_seq_length=L, max_query_length=L)
        wrapped = types.SimpleNamespace(module=model, eval=model.eval)
        with U.EmbeddingCache(path) as emb_cache:
            G.StreamInferenceDoc(args, wrapped, T.GetProcessingFn(args, query=False), "passage_", emb_cache,
                                 is_query_inference=False, merge=False)
        dist.destroy_process_group()
        emb = pickle.load(open(os.path.join(out_dir, "passage__emb_p__data_obj_0.pb"), "rb"))
        embid = pickle.load(open(os.path.join(out_dir, "passage__embid_p__data_obj_0.pb"), "rb"))
        token_bytes = open(path, "rb").read()
        assert emb.shape == (2 * N, 768) and embid.shape == (2 * N,)
        # row -> chunk number: the j-th row that carries an offset is that record's chunk j
        chunk = np.zeros(2 * N, np.int64)
        seen = {}
        for r, o in enumerate(embid.tolist()):
            chunk[r] = seen.get(o, 0)
            seen[o] = chunk[r] + 1
        live = chunk * BASE < lens[embid]
        dead = emb[~live]
        assert len(dead) and np.abs(dead - dead[0]).max() < 1e-4, "the all-pad chunk has one embedding"
        # The tiny random encoder puts every chunk that starts with <s> -- and the all-pad chunk -- into one tight cluster
        # (|p - centre| ~ 3.9 at |p| = 27.7); only the second chunks of the long records lie apart (~20).  No query orders
        # the cluster's documents in a way that survives a rounding of the embeddings at the project's bar (1 - cos <= 1e-3), so
        # the queries are built to say so: the least-norm q with
        #   q . (p - c) = 0        for every live row p of the cluster (centre c): one exact tie, exchangeable by the
        #                          1e-3 rule of the search fixtures;
        #   q . (p - c) = t_j      for the far rows, t_j a permutation of -4.5, -3.5, .., 4.5: a document whose second chunk
        #                          scores above the cluster is ranked by it, one below by its first chunk;
        #   q . (dead - c) = -1    the all-pad row scores below every document's best live row, as under the model's own
        #                          MaxP bias.
        # A perturbation of every embedding at the bar itself, in a random direction, moves these scores by < 0.25.
        dist = np.linalg.norm(emb - emb[live].mean(0), axis=1)
        far = live & (dist > 10.0)
        near = live & ~far
        assert far.sum() == 10 and dist[near].max() < 7.0 and dist[far].min() > 15.0, (far.sum(), dist)
        c = emb[near].astype(np.float64).mean(0)
        A = np.vstack([emb[near] - c, emb[far] - c, dead[:1] - c]).astype(np.float64)
        Q = []
        for _ in range(6):
            t = np.concatenate([np.zeros(near.sum()), rng.permutation(10) - 4.5, [-1.0]])
            Q.append(np.linalg.lstsq(A, t, rcond=None)[0])
        Q = np.asarray(Q, np.float32)
        topN = 2 * N
        with contextlib.redirect_stdout(io.StringIO()):
            ref_D, ref_I = R.search_one_by_one(out_dir, FlatIPStandIn(768), Q, topN)
        offset2pid = (7 + 3 * np.arange(N)).tolist()
        qids = ["%d_%d" % (81 + i // 3, 1 + i % 3) for i in range(len(Q))]
        with open(os.path.join(td, "queries.raw.tsv"), "w") as f:
            for q in qids:
                f.write("%s\tquery text %s\n" % (q, q))
        with open(os.path.join(td, "collection.tsv"), "w") as f:
            for pid in offset2pid:
                f.write("%d\tpassage %d body\n" % (pid, pid))
        raw = [["hist %s" % q, "cur %s" % q] for q in qids]
        R.EvalDevQuery(qids, ref_D, {}, ref_I, topN, os.path.join(td, "o.jsonl"), os.path.join(td, "o.trec"), offset2pid, td,
                       "raw", raw_sequences=raw)
        trec = open(os.path.join(td, "o.trec")).read()
    # the smallest gap between the best scores of two documents that follow each other in a ranking (for the record)
    gaps = []
    for qx in range(len(Q)):
        best = {}
        for s, o in zip(ref_D[qx], ref_I[qx]):
            best.setdefault(int(o), float(s))
        v = sorted(best.values(), reverse=True)
        gaps.append(min(a - b for a, b in zip(v, v[1:])))
    print("smallest gap between adjacent documents per query:", ["%.4g" % g for g in gaps])
    out = {"token_cache": np.frombuffer(token_bytes, np.uint8), "N": np.array(N), "L": np.array(L), "base_len": np.array(BASE),
           "lens": lens.astype(np.int64), "batch_size": np.array(BATCH), "emb": emb, "embid": embid,
           "weights_from": np.array("encode_loop.npz"), "weights_sha256": np.array(weights_sha256(wnames, lambda k: zw[k])),
           "Q": Q, "ref_D": ref_D, "ref_I": ref_I, "ref_topN": np.array(topN), "offset2pid": np.array(offset2pid, np.int64),
           "qids": np.array(qids), "trec": np.array(trec)}
    np.savez_compressed(os.path.join(HERE, "maxp.npz"), **out)
    print("maxp fixture written", emb.shape, embid[:10], os.path.getsize(os.path.join(HERE, "maxp.npz")), "bytes")


if __name__ == "__main__":
    main()
