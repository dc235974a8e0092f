"""Document rank: the numpy oracle of tests/test_doc_rank_{cpu,gpu}.py.

A document is every row that carries one id; it stands where its best row stands in the canonical row order (fp64 canonical
score descending, row ascending).  With S = oracle.search.canonical_scores(Q, P) the rank of document `key` for query j is the
number of distinct ids among the (allowed) rows that precede its best row, its own id left out.  brute_rank restates it with
nothing but a walk over the canonical row order (the CPU test holds the two against each other); ordinals is the oracle of
FlatIPIndex.doc_ordinals."""
import numpy as np

from tests import key_cases as K


def best_row(s, col, key):
    """the row of `key` with the largest score, the lowest on a tie; -1 when the id is on no row"""
    if key == K.I64_MIN:
        return -1
    T = np.nonzero(col == key)[0]
    return int(T[np.argmax(s[T])]) if len(T) else -1       # (argmax: the first maximum, and T ascends)


def rank(s, col, key, mask=None):
    """rank of document `key` for one query's scores s over the column col; mask: bool [n], the allowed rows"""
    t = best_row(s, col, key)
    if t < 0:
        return -1
    m = np.ones(len(s), bool) if mask is None else mask
    prec = ((s > s[t]) | ((s == s[t]) & (np.arange(len(s)) < t))) & m & (col != key)
    return len(np.unique(col[prec]))


def ranks(S, col, ids, mask=None):
    ids2 = np.asarray(ids).reshape(S.shape[0], -1)
    return np.asarray([[rank(S[j], col, int(k), mask) for k in ids2[j]] for j in range(S.shape[0])],
                      np.int64).reshape(np.asarray(ids).shape)


def brute_rank(s, col, key, mask=None):
    """walk the canonical row order, collecting the ids of the allowed rows, until the document's first row appears"""
    if key == K.I64_MIN or not any(c == key for c in col):
        return -1
    order = sorted(range(len(s)), key=lambda r: (-s[r], r))
    seen = set()
    for r in order:
        if col[r] == key:
            return len(seen)
        if mask is None or mask[r]:
            seen.add(int(col[r]))
    raise AssertionError("unreachable")


def row_rank(s, t, mask=None):
    """rank of ROW t among the (allowed) rows (the oracle of rank_rows)"""
    m = np.ones(len(s), bool) if mask is None else mask
    return int(((s > s[t]) & m).sum() + ((s == s[t]) & m & (np.arange(len(s)) < t)).sum())


def ordinals(col):
    """(ord uint32 [n], ndocs): documents numbered in the order of their first rows"""
    if not len(col):
        return np.zeros(0, np.uint32), 0
    _, first, inv = np.unique(col, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inv.reshape(-1)].astype(np.uint32), len(first)
