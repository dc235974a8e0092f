"""Shared cases of the deep-list tests (CPU and GPU): ranked lists for the distinct kernel, sorted lists for the W-way merge
with their reference (numpy's stable descending sort of the concatenation), the workspace formula of
convdr_topk_distinct_deep, and a three-block corpus deep enough for a MaxP search at row depth 4,400."""
import numpy as np

from tests import distinct_cases as DC

PAD_SCORE = DC.PAD_SCORE
KINDS = ("equal", "distinct", "mult", "high", "padded", "map", "oob")


def distinct_case(kind, nq, n, seed):
    """-> (D [nq, n] descending with ties, I [nq, n], key_map or None).
    equal: one id throughout; distinct: no repeats; mult / padded: every key on 1..4 rows (padded: a FAISS padding tail and
    padding ids inside the row); high: ids that differ only above bit 32; map / oob: keys through a key_map (oob: ids past it)."""
    if nq == 0:
        D, I, key_map = distinct_case(kind, 1, n, seed)
        return D[:0], I[:0], key_map
    rs = np.random.RandomState(seed)
    D = np.sort(rs.randint(0, 40, size=(nq, n)).astype(np.float32) * 0.25 - 3.0, axis=1)[:, ::-1].copy()
    key_map = None
    if kind == "equal":
        I = np.full((nq, n), 2 ** 40 + 17, np.int64)
    elif kind == "distinct":
        I = np.stack([rs.permutation(n) for _ in range(nq)]).astype(np.int64).reshape(nq, n) * 3 + 2 ** 33
    elif kind == "high":
        I = (rs.randint(0, max(1, n // 2), size=(nq, n)).astype(np.int64) << 32) + 12345
    elif kind in ("map", "oob"):
        nids = max(2, n)
        I = rs.randint(0, nids, size=(nq, n)).astype(np.int64)
        key_map = (rs.randint(0, max(1, n // 2), size=nids).astype(np.int64) << (32 * (seed % 2))) + 7
        if kind == "oob" and n:
            I[0, n // 2] = nids                       # one id past the map in query 0: never looked up
            if nq > 1 and n > 2:
                I[nq - 1, n - 1] = 2 ** 62
    else:
        I = np.stack([np.repeat(rs.permutation(n), rs.randint(1, 5, size=n))[:n][rs.permutation(n)] for _ in range(nq)])
        I = I.astype(np.int64).reshape(nq, n) + 2 ** 35
    if kind == "padded" and n:
        for q in range(nq):
            t = rs.randint(0, n // 2 + 1)
            D[q, n - t:], I[q, n - t:] = PAD_SCORE, -1
        I[rs.rand(nq, n) < 0.1] = -1
    return D, I, key_map


def distinct_ws_bytes(nq, n):
    """convdr_topk_distinct_deep_workspace_bytes as include/convdr_hip.h states it: keys int64 [nq][n] rounded up to 256 bytes,
    then tables uint32 [nq][2^hbits], 2^hbits the smallest power of two >= 2n and >= 64."""
    slots = 64
    while slots < 2 * n:
        slots *= 2
    return (nq * n * 8 + 255) // 256 * 256 + nq * slots * 4


# ---- the W-way merge -------------------------------------------------------------------------------------------------
def merge_lists(rs, W, n, nq):
    """[W, nq, n] scores drawn from 40 distinct values (ties inside and across lists are the rule), rows descending, the
    last list ending in a run of FAISS padding; ids random."""
    D = np.sort(rs.randint(0, 40, size=(W, nq, n)).astype(np.float32) * 0.25 - 3.0, axis=2)[:, :, ::-1].copy()
    I = rs.randint(0, 2 ** 62, size=(W, nq, n), dtype=np.int64)
    npad = max(1, n // 3) if n > 1 else 0
    if npad:
        D[W - 1, :, n - npad:] = PAD_SCORE
        I[W - 1, :, n - npad:] = -1
    return D, I


def merge_reference(D, I, n_out):
    W, nq, n = D.shape
    d = D.transpose(1, 0, 2).reshape(nq, W * n)
    i = I.transpose(1, 0, 2).reshape(nq, W * n)
    order = np.argsort(-d.astype(np.float64), axis=1, kind="stable")[:, :n_out]
    return np.take_along_axis(d, order, 1), np.take_along_axis(i, order, 1)


def merge_pack(D, I):
    """[W, nq, n] -> the wire format [W, nq, n, 3] int32: score bits, offset low word, offset high word."""
    W, nq, n = D.shape
    buf = np.empty((W, nq, n, 3), np.int32)
    buf[..., 0] = D.view(np.int32)
    buf[..., 1:] = np.ascontiguousarray(I).view(np.int32).reshape(W, nq, n, 2)
    return buf


# ---- three block files for a MaxP search at row depth m = TOPN * ROWS_PER_KEY = 4,400 ----------------------------------------
SIZES, DIM, NQ, TOPN, ROWS_PER_KEY = (4500, 4600, 4700), 64, 5, 1100, 4
M = TOPN * ROWS_PER_KEY


def corpus():
    """distinct_cases.corpus at depth: every block holds at least M rows (the host path looks all M ids up in every block),
    keys own 1..4 rows, and the same plants lead three queries: a key across two blocks (query 0), exact duplicates across
    blocks under the same and under another key (query 1), one vector twice inside a block under two keys (query 2)."""
    rs = np.random.RandomState(12)
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
    assert nxt < 50000
    for (b, r), scale in zip(((0, 10), (0, 4400), (1, 3), (1, 4500)), (3.0, 2.9, 2.8, 2.7)):
        embs[b][r] = scale * Q[0]
        keys[b][r] = 50000
    for (b, r), key in zip(((0, 77), (1, 78), (2, 79)), (50001, 50002, 50001)):
        embs[b][r] = 3.0 * Q[1]
        keys[b][r] = key
    for r, key in ((5, 50003), (4600, 50004)):
        embs[2][r] = 3.0 * Q[2]
        keys[2][r] = key
    assert np.unique(np.concatenate(keys), return_counts=True)[1].max() == ROWS_PER_KEY
    return Q, list(zip(embs, keys))
