"""Row ids: the numpy oracle and the key families of tests/test_keyed_index_{cpu,gpu}.py.

The oracle is np.isin for membership and a dict walk for (first row, count, smallest list position); the brute_* functions
restate it with nothing but == (the CPU test holds the two against each other on small inputs).
A family gives, for any (n, m), a column of n row keys and a list of m keys.  Every list mixes keys that are on rows with
keys that are on none; the families differ in what a hash set finds hard or what a column looks like in practice."""
import functools
import zlib

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
EDGE_KEYS = (0, -1, I64_MAX, I64_MIN + 1, 1, -2)           # (I64_MIN itself is the reserved id)
FAMILIES = ("random", "consecutive", "shift20", "strides", "triple", "chunks", "absent")


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def member(col, lst):
    return np.isin(col, lst)


def missing(col, lst):
    """distinct listed keys that are on no row"""
    return int(np.setdiff1d(np.unique(lst), col).size)


def locate(col, lst):
    """(first_row int64 [m], count int32 [m], dup_of int32 [m])"""
    first, cnt = _rows_by_key(col.tobytes())
    pos = {}
    for j, k in enumerate(lst.tolist()):
        pos.setdefault(k, j)
    keys = lst.tolist()
    return (np.array([first.get(k, -1) for k in keys], np.int64).reshape(-1),
            np.array([cnt.get(k, 0) for k in keys], np.int32).reshape(-1),
            np.array([pos[k] for k in keys], np.int32).reshape(-1))


@functools.lru_cache(maxsize=64)
def _rows_by_key(col_bytes):
    first, cnt = {}, {}
    for r, k in enumerate(np.frombuffer(col_bytes, np.int64).tolist()):
        first.setdefault(k, r)
        cnt[k] = cnt.get(k, 0) + 1
    return first, cnt


def brute_member(col, lst):
    return np.array([any(c == k for k in lst) for c in col], bool).reshape(-1)


def brute_locate(col, lst):
    first = [next((r for r, c in enumerate(col) if c == k), -1) for k in lst]
    count = [sum(1 for c in col if c == k) for k in lst]
    dup = [next(i for i, x in enumerate(lst) if x == k) for k in lst]
    return np.array(first, np.int64).reshape(-1), np.array(count, np.int32).reshape(-1), np.array(dup, np.int32).reshape(-1)


# ---- the families -----------------------------------------------------------------------------------------------------------
def _full_range(rs, size):
    return rs.randint(0, 1 << 32, size=size, dtype=np.uint64).astype(np.int64) << 32 | rs.randint(0, 1 << 32, size=size, dtype=np.int64)


def _pools(family, n, rs):
    """(keys the column is drawn from, in column order; a function i -> a key that is on no row)"""
    i = np.arange(max(n, 1), dtype=np.int64)
    if family in ("random", "triple", "absent"):
        pool = _full_range(rs, i.size)
        pool[pool == I64_MIN] = 5
        pool[:len(EDGE_KEYS)] = EDGE_KEYS[:i.size]
        rs.shuffle(pool)
        return pool, lambda j: (np.asarray(j, np.int64) * 2654435761 + 12345) ^ (1 << 61)      # (not in the pool but by accident: checked)
    if family == "consecutive":
        return i + 1000, lambda j: np.asarray(j, np.int64) + 1000 + i.size
    if family == "shift20":
        return i << 20, lambda j: (np.asarray(j, np.int64) + i.size) << 20
    if family == "strides":
        # three power-of-two strides side by side, negatives included: (i - n / 2) << 40, i << 32 | 7, i << 12 | 1
        pool = np.where(i % 3 == 0, (i - i.size // 2) << 40, np.where(i % 3 == 1, i << 32 | 7, i << 12 | 1))
        return pool, lambda j: (np.asarray(j, np.int64) + 1) << 52 | 3
    if family == "chunks":
        # MaxP chunk rows: an id sits on 1 .. 7 consecutive rows
        reps = rs.randint(1, 8, size=i.size)
        return np.repeat(i * 3 - 50, reps)[:i.size], lambda j: np.asarray(j, np.int64) * 3 - 49
    raise ValueError(family)


def _seed(*what):
    return zlib.crc32(repr(what).encode()) % (1 << 31)


@functools.lru_cache(maxsize=None)
def case(family, n, m, seed=0):
    """(column int64 [n], list int64 [m]), read-only"""
    rs = np.random.RandomState(_seed(family, n, seed))
    pool, absent = _pools(family, n, rs)
    col = pool[:n].copy()
    rl = np.random.RandomState(_seed(family, n, m, seed, 1))
    if family == "triple":
        col, base = case("random", n, (m + 2) // 3, seed)          # every key of the list three times, shuffled
        col, lst = col.copy(), np.tile(base, 3)[:m].copy()
        rl.shuffle(lst)
    else:
        on = rl.randint(0, max(n, 1), size=m)
        off = absent(rl.randint(0, 4 * max(m, 1), size=m))
        take_on = (rl.rand(m) < 0.5) & (n > 0) & (family != "absent")
        lst = np.where(take_on, pool[on], off).astype(np.int64)
        if family == "absent":
            lst = lst[~np.isin(lst, col)] if m else lst
            lst = np.resize(lst, m) if lst.size else absent(np.arange(m))
    lst[lst == I64_MIN] = 6
    col.setflags(write=False)
    lst.setflags(write=False)
    return col, lst
