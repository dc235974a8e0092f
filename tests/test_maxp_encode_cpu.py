"""Chunk rows in the corpus-encode loop (encode.encode_shard with a model that carries ``base_len``), on the host device
with a stand-in tower: which chunk ids and lengths reach the tower, the row order, the repeated record offsets, and that
pure-padding chunks are absent.  Only the index work around the encoder is under test (no GPU)."""
import json
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from convdr_amd import blocks, encode

BASE, L = 512, 1024
LENS = (1, 512, 513, 1024, 700, 2, 511, 514, 1023, 300, 512, 1024, 600)


class _Tower:
    """Records every call; embedding = (first token, last token, length, sum of the live tokens, 0, ...)."""

    def __init__(self):
        self.W = torch.zeros(1)
        self.calls = []

    def embed(self, ids, mask, head=None, seq_lens=None):
        assert mask is None and ids.dtype == torch.int32
        lens = np.asarray(seq_lens)
        self.calls.append((ids.clone().numpy(), lens.copy()))
        out = torch.zeros((ids.shape[0], 8))
        for b in range(ids.shape[0]):
            live = ids[b, :int(lens[b])].long()
            out[b, 0], out[b, 1], out[b, 2], out[b, 3] = live[0], live[-1], int(lens[b]), live.sum()
        return out


class _Model:
    def __init__(self, base_len=None):
        self.roberta, self.embeddingHead, self.norm = _Tower(), None, None
        if base_len:
            self.base_len = base_len

    def parameters(self):
        return iter([self.roberta.W])


def _write_cache(path, lens, width, seed=4):
    rs = np.random.RandomState(seed)
    ids = rs.randint(3, 30000, size=(len(lens), width)).astype(np.int32)
    with open(path, "wb") as f:
        for i, n in enumerate(lens):
            ids[i, n:] = 0
            f.write(int(n).to_bytes(4, "big") + ids[i].tobytes())
    with open(path + "_meta", "w") as f:
        json.dump({"type": "int32", "total_number": len(lens), "embedding_size": width}, f)
    return ids


def _expected_rows(lens, idx):
    """[(record offset, chunk number, first token position, chunk length)] record-major, live chunks only."""
    rows = []
    for i in idx:
        for j in range(max(1, -(-lens[i] // BASE))):
            rows.append((i, j, j * BASE, min(lens[i], (j + 1) * BASE) - j * BASE))
    return rows


@pytest.mark.parametrize("rank,world,batch_size,token_budget", [(0, 1, 4, None), (0, 1, 64, None), (1, 2, 3, None), (0, 1, 64, 1100)])
def test_chunk_rows_lengths_order_and_offsets(tmp_path, rank, world, batch_size, token_budget):
    ids = _write_cache(str(tmp_path / "passages"), LENS, L)
    model = _Model(BASE)
    with blocks.TokenCache(str(tmp_path / "passages")) as cache:
        emb, embid = encode.encode_shard(model, cache, rank, world, batch_size, token_budget=token_budget)
    rows = _expected_rows(LENS, range(rank, len(LENS), world))
    assert embid.dtype == np.int64 and embid.tolist() == [r[0] for r in rows]          # the offset repeated per live chunk
    assert emb.dtype == np.float32 and emb.shape == (len(rows), 8)
    for e, (i, j, t0, n) in zip(emb, rows):                                            # record-major rows, chunk j = its tokens
        assert (e[0], e[1], e[2], e[3]) == (ids[i, t0], ids[i, t0 + n - 1], n, float(np.float32(ids[i, t0:t0 + n].sum()))), (i, j)
    # what the tower saw: 2-D int32 chunk rows no wider than base_len, their lengths, nothing of a dead chunk
    seen = 0
    for cids, clens in model.roberta.calls:
        assert cids.ndim == 2 and cids.shape[1] == clens.max() <= BASE and len(clens) <= batch_size
        if token_budget and len(clens) > 1:
            assert ((clens + 7) // 8 * 8).sum() <= token_budget
        for b in range(len(clens)):
            i, j, t0, n = rows[seen + b]
            assert clens[b] == n >= 1 and np.array_equal(cids[b, :n], ids[i, t0:t0 + n])
        seen += len(clens)
    assert seen == len(rows)
    # lengths 1 / 512 / 513 / 1,024 give 1 / 1 / 2 / 2 rows, the 513th token alone in its chunk
    per = {i: [r for r in rows if r[0] == i] for i in range(len(LENS))}
    if world == 1:
        assert [len(per[i]) for i in range(4)] == [1, 1, 2, 2]
        assert per[2][1] == (2, 1, 512, 1) and per[3][1] == (3, 1, 512, 512) and per[0][0] == (0, 0, 0, 1)


def test_stream_inference_doc_writes_chunk_rows(tmp_path):
    _write_cache(str(tmp_path / "passages"), LENS, L)
    args = SimpleNamespace(data_dir=str(tmp_path), output_dir=str(tmp_path / "out"), per_gpu_eval_batch_size=5, max_seq_length=L)
    emb, embid = encode.generate_new_ann(args, _Model(BASE))
    femb = pickle.load(open(tmp_path / "out" / "passage__emb_p__data_obj_0.pb", "rb"))
    fid = pickle.load(open(tmp_path / "out" / "passage__embid_p__data_obj_0.pb", "rb"))
    rows = _expected_rows(LENS, range(len(LENS)))
    assert fid.dtype == np.int64 and fid.tolist() == [r[0] for r in rows] and np.array_equal(femb, emb) and np.array_equal(fid, embid)
    assert blocks.max_rows_per_key(str(tmp_path / "out")) == 2


def test_width_must_be_a_multiple_of_base_len(tmp_path):
    _write_cache(str(tmp_path / "passages"), (5, 700, 1000), 1000)
    with blocks.TokenCache(str(tmp_path / "passages")) as cache:
        with pytest.raises(ValueError, match="base_len"):
            encode.encode_shard(_Model(BASE), cache)
        with pytest.raises(ValueError, match="base_len"):
            encode.encode_shard(_Model(BASE), cache, max_seq_length=768)
        emb, embid = encode.encode_shard(_Model(BASE), cache, max_seq_length=512)      # cut to one chunk: fine
        assert embid.tolist() == [0, 1, 2] and emb[:, 2].tolist() == [5, 512, 512]


def test_queries_and_2d_models_are_unchanged(tmp_path):
    """A model without base_len, and a MaxP model encoding queries, take the one-row-per-record path as before."""
    ids = _write_cache(str(tmp_path / "passages"), LENS, L)
    with blocks.TokenCache(str(tmp_path / "passages")) as cache:
        for model, is_query in ((_Model(), False), (_Model(BASE), True)):
            emb, embid = encode.encode_shard(model, cache, 0, 1, 4, is_query)
            assert embid.tolist() == list(range(len(LENS))) and emb.shape == (len(LENS), 8)
            for i, n in enumerate(LENS):
                assert (emb[i, 0], emb[i, 1], emb[i, 2]) == (ids[i, 0], ids[i, n - 1], n)
            for cids, clens in model.roberta.calls:
                assert cids.shape[1] == clens.max()
            assert sum(len(c[1]) for c in model.roberta.calls) == len(LENS)
            assert max(c[0].shape[1] for c in model.roberta.calls) == 1024                 # whole records, not chunks
