"""Documents by id: the numpy oracle and the cases of tests/test_doc_ops_{cpu,gpu}.py.

A document is every row that carries one id.  The oracle is np.nonzero(col == id) per id and np.argmax for the MaxP pair
(the first maximum: rows ascend, so the lowest row wins a tie); the brute_* functions restate both with nothing but == and a
walk (the CPU test holds them against each other on small inputs).  `interleaved` is the column the key_cases families do
not have: the rows of a document lie apart, between the rows of other documents, and one id sits on thousands of rows."""
import functools

import numpy as np

from tests import key_cases as K

PAD_SCORE = np.float32(-3.4028234663852886e38)
BIG_ID = 777_000_000_007                     # the id of `interleaved` that sits on every fourth row
FAMILIES = ("chunks", "triple", "absent", "random", "interleaved")


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def rows_of(col, key):
    """ascending rows that carry `key` (the reserved id is on no row)"""
    if key == K.I64_MIN:
        return np.zeros(0, np.int64)
    return np.nonzero(col == key)[0].astype(np.int64)


def rows_all(col, lst):
    """(start int64 [m], count int32 [m], rows int64 [total], dup_of int32 [m]): the segments follow the list, a repeated key
    shares the segment of its first occurrence, total counts every distinct key once"""
    first, start, count, dup, rows, total = {}, [], [], [], [], 0
    for j, k in enumerate(lst.tolist()):
        if k in first and k != K.I64_MIN:
            o = first[k]
            start.append(start[o]); count.append(count[o]); dup.append(o)
            continue
        first[k] = j
        r = rows_of(col, k)
        start.append(0 if k == K.I64_MIN else total)
        count.append(len(r)); dup.append(j)
        rows.append(r)
        total += len(r)
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    return (np.array(start, np.int64).reshape(-1), np.array(count, np.int32).reshape(-1), rows.astype(np.int64),
            np.array(dup, np.int32).reshape(-1))


def maxp(scores, rows):
    """(best score, the row that attains it -- the lowest on a tie) of one segment; rows ascend.  Empty: (None, -1)."""
    if not len(rows):
        return None, -1
    i = int(np.argmax(scores))
    return scores[i], int(rows[i])


def brute_rows_all(col, lst):
    start, count, rows, total = [], [], [], 0
    for j, k in enumerate(lst):
        o = next(i for i, x in enumerate(lst) if x == k)
        if o != j and k != K.I64_MIN:
            start.append(start[o]); count.append(count[o])
            continue
        mine = [] if k == K.I64_MIN else [r for r, c in enumerate(col) if c == k]
        start.append(0 if k == K.I64_MIN else total); count.append(len(mine))
        rows += mine
        total += len(mine)
    return np.array(start, np.int64).reshape(-1), np.array(count, np.int32).reshape(-1), np.array(rows, np.int64).reshape(-1)


def brute_maxp(scores, rows):
    best, row = None, -1
    for s, r in zip(scores, rows):
        if best is None or s > best or (s == best and r < row):
            best, row = s, int(r)
    return best, row


# ---- the interleaved column ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def interleaved(n):
    """column int64 [n], read-only: BIG_ID on every row r with r % 4 == 3 (5,000 rows at n = 20,000); documents of three rows
    at (r, r + 7, r + 300) wherever the three are free, in between one another; the edge keys; every other row its own id"""
    col = np.full(n, K.I64_MIN, np.int64)
    col[3::4] = BIG_ID
    free = col == K.I64_MIN
    doc = 0
    for r in range(n):
        if r + 300 < n and free[r] and free[r + 7] and free[r + 300]:
            col[[r, r + 7, r + 300]] = 5_000_000 + 11 * doc
            free[[r, r + 7, r + 300]] = False
            doc += 1
    rest = np.nonzero(free)[0]
    col[rest] = -9_000_000_000 - 3 * np.arange(rest.size, dtype=np.int64)
    col[rest[:len(K.EDGE_KEYS)]] = K.EDGE_KEYS[:rest.size]
    col.setflags(write=False)
    return col


@functools.lru_cache(maxsize=None)
def case(family, n, m, seed=0):
    """(column int64 [n], list int64 [m]), read-only.  The key_cases families as they are; the interleaved column with a list
    of present ids (BIG_ID and the edge keys among them), absent ids and repeats."""
    if family != "interleaved":
        return K.case(family, n, m, seed)
    col = interleaved(n)
    rs = np.random.RandomState(K._seed("interleaved", n, m, seed))
    present = np.concatenate([[BIG_ID], K.EDGE_KEYS, rs.choice(col, size=m) if n else np.zeros(0, np.int64)]).astype(np.int64)
    absent = 123_456_789_000 + 5 * np.arange(m + 1, dtype=np.int64)
    lst = np.where(rs.rand(m) < 0.7, np.resize(present, m), absent[:m]).astype(np.int64)
    if m > 2:
        rep = rs.randint(0, m, size=m // 4)
        lst[rep] = lst[rs.randint(0, m, size=m // 4)]             # repeats anywhere in the list
    lst.setflags(write=False)
    return col, lst


# ---- a chunked corpus: documents of 1 .. 6 rows, anywhere in the block ---------------------------------------------------------
def chunked_ids(n, seed=0, most=6):
    """int64 [n]: every id on 1 .. `most` rows, the rows of a document scattered over the block; negative and positive ids"""
    rs = np.random.RandomState(seed + n)
    ids, nxt = [], 0
    while len(ids) < n:
        ids += [nxt * 1000003 - 40_000_000] * int(rs.randint(1, most + 1))
        nxt += 1
    return np.asarray(ids[:n], np.int64)[rs.permutation(n)]
