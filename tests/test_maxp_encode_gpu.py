"""MaxP end to end against a run of the reference (tests/golden/maxp.npz, written by tests/golden/make_golden_maxp.py): the
corpus-encode loop writes one row per live 512-token chunk, and the document-level search over that block returns the
documents of the reference's de-duplicated ranking."""
import hashlib
import json
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import cosine, margin

pytestmark = pytest.mark.gpu

COS_TOL = 1e-3          # the project's embedding bar (tests/test_encoder_gpu.py)
RANK_TOL = 1e-3         # ranks whose reference scores differ by less are exchangeable (tests/helpers.py: assert_topk_equivalent)


def _weights(golden_dir, z):
    zw = np.load(os.path.join(golden_dir, str(z["weights_from"])))
    names = sorted(k for k in zw.files if k.startswith("w/"))
    h = hashlib.sha256()
    for k in names:
        h.update(k.encode())
        h.update(np.ascontiguousarray(zw[k]).tobytes())
    assert h.hexdigest() == str(z["weights_sha256"]), "encode_loop.npz no longer holds the weights maxp.npz was recorded with"
    return {k[2:]: torch.from_numpy(zw[k]) for k in names}


def _reference_ranking(ref_D, ref_I):
    """The reference's own first-occurrence walk (run_convdr_inference.py:58-69) over its row ranking: [(offset, score)]."""
    out = []
    for d, i in zip(ref_D, ref_I):
        seen, row = set(), []
        for score, off in zip(d.tolist(), i.tolist()):
            if off not in seen:
                seen.add(off)
                row.append((off, score))
        out.append(row)
    return out


def _assert_same_documents(ref_row, docs, what):
    """Same documents rank by rank, up to permutations inside runs of reference scores closer than RANK_TOL."""
    k = len(ref_row)
    assert len(docs) == k and sorted(docs) == sorted(o for o, _ in ref_row), what
    start = 0
    while start < k:
        end = start + 1
        while end < k and abs(ref_row[end - 1][1] - ref_row[end][1]) < RANK_TOL:
            end += 1
        assert sorted(o for o, _ in ref_row[start:end]) == sorted(docs[start:end]), \
            "%s ranks %d..%d: %s vs %s" % (what, start, end, ref_row[start:end], docs[start:end])
        start = end


def test_chunk_rows_and_document_search_match_the_reference_run(golden_dir, tmp_path):
    from convdr_amd import encode
    from convdr_amd import search as S
    from convdr_amd.model.models import MSMarcoConfigDict, RobertaConfig
    z = np.load(os.path.join(golden_dir, "maxp.npz"))
    N, L, base = int(z["N"]), int(z["L"]), int(z["base_len"])
    lens = z["lens"]
    (tmp_path / "data").mkdir()
    open(tmp_path / "data" / "passages", "wb").write(z["token_cache"].tobytes())
    json.dump({"type": "int32", "total_number": N, "embedding_size": L}, open(tmp_path / "data" / "passages_meta", "w"))
    cfg = RobertaConfig(vocab_size=200, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                        intermediate_size=256, max_position_embeddings=514)
    model = MSMarcoConfigDict["rdot_nll_multi_chunk"].model_class(cfg)
    missing, unexpected = model.load_state_dict(_weights(golden_dir, z), strict=False)
    assert not unexpected and all("pooler" in k for k in missing), (missing, unexpected)
    model = model.cuda().eval()
    assert model.base_len == base
    args = SimpleNamespace(data_dir=str(tmp_path / "data"), output_dir=str(tmp_path / "out"),
                           per_gpu_eval_batch_size=int(z["batch_size"]), max_seq_length=L)
    encode.generate_new_ann(args, model)
    emb = pickle.load(open(tmp_path / "out" / "passage__emb_p__data_obj_0.pb", "rb"))      # the reference's reader
    embid = pickle.load(open(tmp_path / "out" / "passage__embid_p__data_obj_0.pb", "rb"))
    # one row per live chunk, record-major, the record offset repeated
    n_live = -(-lens // base)
    assert embid.dtype == np.int64 and embid.tolist() == np.repeat(np.arange(N), n_live).tolist()
    assert emb.dtype == np.float32 and emb.shape == (int(n_live.sum()), 768) and emb.flags.c_contiguous
    # every (record, live chunk) row against the reference's j-th row of that offset; its dead-chunk rows have no counterpart
    ref_rows = {o: np.nonzero(z["embid"] == o)[0] for o in range(N)}
    assert all(len(r) == L // base for r in ref_rows.values())
    chunk = np.concatenate([np.arange(c) for c in n_live])
    ref_of = np.array([ref_rows[int(o)][j] for o, j in zip(embid, chunk)])
    assert len(set(ref_of.tolist())) == len(ref_of) < len(z["embid"])
    cs = cosine(emb, z["emb"][ref_of])
    margin("maxp_encode/worst_1-cos", 1.0 - cs.min(), COS_TOL)
    # the document-level search over the written block against the reference's de-duplicated ranking
    Q = z["Q"]
    ranking = _reference_ranking(z["ref_D"], z["ref_I"])
    assert all(len(r) == N for r in ranking)
    D, I = S.search_distinct_one_by_one(str(tmp_path / "out"), S.FlatIPIndex(768), Q, N)
    assert D.shape == I.shape == (len(Q), N) and D.dtype == np.float64 and I.dtype == np.int64
    worst = 0.0
    for qx in range(len(Q)):
        _assert_same_documents(ranking[qx], I[qx].tolist(), "query %d" % qx)
        ref_score = dict(ranking[qx])
        worst = max(worst, max(abs(ref_score[o] - s) for o, s in zip(I[qx].tolist(), D[qx].tolist())))
    # (Cauchy-Schwarz at the embedding bar: |q . (p' - p)| <= |q| |p| sqrt(2 (1 - cos)) for rows of equal norm)
    margin("maxp_search/worst_score_err", worst,
           float(np.linalg.norm(Q, axis=1).max() * np.linalg.norm(z["emb"], axis=1).max() * np.sqrt(2 * COS_TOL)))
    # EvalDevQuery takes the result as it is: nothing to drop, no (0, 0) tail; its .trec text against the reference's
    offset2pid = z["offset2pid"].tolist()
    qids = [str(q) for q in z["qids"]]
    with open(tmp_path / "queries.raw.tsv", "w") as f:
        for q in qids:
            f.write("%s\tquery text %s\n" % (q, q))
    with open(tmp_path / "collection.tsv", "w") as f:
        for pid in offset2pid:
            f.write("%d\tpassage %d body\n" % (pid, pid))
    raw = [["hist %s" % q, "cur %s" % q] for q in qids]
    S.EvalDevQuery(qids, D, {}, I, N, str(tmp_path / "o.jsonl"), str(tmp_path / "o.trec"), offset2pid, str(tmp_path), "raw",
                   raw_sequences=raw)
    ours = open(tmp_path / "o.trec").read().splitlines()
    theirs = str(z["trec"]).splitlines()
    per_q = int(z["ref_topN"])
    assert len(ours) == len(Q) * N and len(theirs) == len(Q) * per_q
    pid2offset = {p: o for o, p in enumerate(offset2pid)}
    for qx in range(len(Q)):
        mine = [ln.split() for ln in ours[qx * N:(qx + 1) * N]]
        ref = [ln.split() for ln in theirs[qx * per_q:qx * per_q + N]]
        assert [(m[0], m[1], m[3], m[4], m[5]) for m in mine] == [(r[0], r[1], r[3], r[4], r[5]) for r in ref]
        assert [pid2offset[int(r[2])] for r in ref] == [o for o, _ in ranking[qx]]
        _assert_same_documents(ranking[qx], [pid2offset[int(m[2])] for m in mine], "trec of query %d" % qx)
        assert all(r.split()[2] == "0" for r in theirs[qx * per_q + N:(qx + 1) * per_q])      # the reference's (0, 0) padding
