"""Shared cases of the distinct-document search tests (CPU and GPU): a literal restatement of the reference's `seen_pid`
walk, the exhaustive document-level answer over the search's canonical total order, and a three-block corpus whose keys
repeat inside and across blocks."""
import os

import numpy as np

PAD_SCORE = np.float32(-3.4028234663852886e38)


def seen_walk(D, I, k, key_map=None):
    """run_convdr_inference.py:58-69, entry by entry, with the contract of convdr_topk_distinct around it: padding ids
    (< 0) are skipped, an id past key_map is skipped and flags the row.  -> (D [nq, k], I, K, counts [nq, 2])."""
    D, I = np.asarray(D), np.asarray(I)
    nq = I.shape[0]
    Do = np.full((nq, k), PAD_SCORE, D.dtype)
    Io = np.full((nq, k), -1, np.int64)
    Ko = np.full((nq, k), -1, np.int64)
    counts = np.zeros((nq, 2), np.int32)
    for q in range(nq):
        seen, rank, valid, oob = set(), 0, 0, False
        for score, idx in zip(D[q], I[q].tolist()):
            if idx < 0:
                continue
            if key_map is not None and idx >= len(key_map):
                oob = True
                continue
            valid += 1
            key = int(key_map[idx]) if key_map is not None else idx
            if key not in seen:
                if rank < k:
                    Do[q, rank], Io[q, rank], Ko[q, rank] = score, idx, key
                rank += 1
                seen.add(key)
        counts[q] = (-1 if oob else rank, valid)
    return Do, Io, Ko, counts


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- three block files, keys with 1..4 rows, one key across two blocks, exact duplicates across blocks -----------------
SIZES, DIM, NQ, TOPN, ROWS_PER_KEY = (700, 690, 710), 64, 9, 20, 4


def corpus():
    """-> (Q [NQ, DIM], [(emb, row keys)] per block).  The row key plays the record offset of a MaxP block (repeated for
    every chunk row of a record).  Planted, each the best hits of one query:
      query 0   four rows of key 5000 at decreasing scores, two in block 0 and two in block 1 (a key across blocks);
      query 1   one vector three times: key 5001 in block 0, key 5002 in block 1 and again key 5001 in block 2 (exact
                duplicates across blocks, with the same and with another key);
      query 2   one vector twice inside block 2 under two keys."""
    rs = np.random.RandomState(11)
    Q = rs.randn(NQ, DIM).astype(np.float32)
    embs = [rs.randn(n, DIM).astype(np.float32) for n in SIZES]
    keys, nxt = [], 0
    for n in SIZES:
        k = []
        while len(k) < n:
            k += [nxt] * int(rs.randint(1, ROWS_PER_KEY + 1))
            nxt += 1
        k = np.asarray(k[:n], np.int64)
        keys.append(k[rs.permutation(n)])
    for (b, r), scale in zip(((0, 10), (0, 400), (1, 3), (1, 500)), (3.0, 2.9, 2.8, 2.7)):
        embs[b][r] = scale * Q[0]
        keys[b][r] = 5000
    for (b, r), key in zip(((0, 77), (1, 78), (2, 79)), (5001, 5002, 5001)):
        embs[b][r] = 3.0 * Q[1]
        keys[b][r] = key
    for r, key in ((5, 5003), (600, 5004)):
        embs[2][r] = 3.0 * Q[2]
        keys[2][r] = key
    allk = np.concatenate(keys)
    assert np.unique(allk, return_counts=True)[1].max() == ROWS_PER_KEY
    return Q, list(zip(embs, keys))


def write_blocks(dirname, blocks_, ids=None):
    from convdr_amd import blocks
    for b, (emb, key) in enumerate(blocks_):
        blocks.dump_block(os.path.join(dirname, "passage__emb_p__data_obj_%d.pb" % b), emb)
        blocks.dump_block(os.path.join(dirname, "passage__embid_p__data_obj_%d.pb" % b), key if ids is None else ids[b])


def total_order(Q, blocks_):
    """Every row of every block in the search's canonical total order: (D fp32 [nq, n], block-order row number [nq, n]).
    Inside a block the oracle's order (canonical fp64 score descending, row ascending); across blocks a stable merge on
    the fp32 scores, earlier block first -- what search_one_by_one's chain of `>=` merges gives at any depth."""
    from oracle import search as OS
    Ds, Is, base = [], [], 0
    for emb, _ in blocks_:
        D, I = OS.flat_ip_search(Q, emb, len(emb))
        Ds.append(D)
        Is.append(I + base)
        base += len(emb)
    D, I = np.concatenate(Ds, 1), np.concatenate(Is, 1)
    order = np.argsort(-D.astype(np.float64), axis=1, kind="stable")
    return np.take_along_axis(D, order, 1), np.take_along_axis(I, order, 1)


def exhaustive(Q, blocks_, k):
    """The document-level answer by the walk over ALL rows: (D float64 [nq, k], row keys int64 [nq, k])."""
    D, rows = total_order(Q, blocks_)
    keys = np.concatenate([key for _, key in blocks_])
    Do, Io, _, _ = seen_walk(D, keys[rows], k)
    return Do.astype(np.float64), Io


class OracleIndex:
    """add / search / reset played by the CPU oracle (no search_begin: the host path of the flow)."""

    def __init__(self):
        self.x = None

    def add(self, x):
        assert self.x is None
        self.x = np.asarray(x, np.float32)

    def search(self, q, k):
        from oracle import search as OS
        return OS.flat_ip_search(q, self.x, k)

    def reset(self):
        self.x = None
