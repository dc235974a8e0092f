"""Per-query exclusions: the numpy oracle and the exclusion recipes of tests/test_exclude_{cpu,gpu}.py.

The oracle is the definition: per query the canonical order np.lexsort((rows, -S[q])) restricted to the allowed rows, with the
query's excluded rows removed; D is S rounded to fp32.  Every recipe is built from that ranking, so that it bites by construction
(`bites` says whether a list reaches into the top-k it is used with).  The brute_* functions restate the oracle with nothing
but comparisons and a walk; the CPU test holds the two against each other on tiny inputs."""
import numpy as np

PAD_SCORE = np.float32(-3.4028234663852886e38)
RECIPES = ("none", "top1", "whole_topk", "scattered", "uneven")      # (+ "nearly_all", on n = 300 only)


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def clean(excluded, n):
    """the distinct rows of one query's list (negative entries are padding)"""
    e = np.asarray(excluded, dtype=np.int64).reshape(-1)
    return np.unique(e[(e >= 0) & (e < n)])


def order(s, allowed=None, excluded=()):
    """the rows of one query in the residual canonical order: score descending, row ascending, allowed, not excluded"""
    n = len(s)
    keep = np.ones(n, bool) if allowed is None else np.asarray(allowed, bool).copy()
    keep[clean(excluded, n)] = False
    o = np.lexsort((np.arange(n), -s))
    return o[keep[o]]


def topk(S, k, allowed=None, lists=None):
    """(D fp32 [nq, k], I int64 [nq, k]) with FAISS padding"""
    nq = S.shape[0]
    D = np.full((nq, k), PAD_SCORE, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for j in range(nq):
        o = order(S[j], allowed, () if lists is None else lists[j])[:k]
        D[j, :len(o)] = S[j, o].astype(np.float32)
        I[j, :len(o)] = o
    return D, I


def rank(s, t, allowed=None, excluded=()):
    """the rows of the residual order that precede row t (t itself need be neither allowed nor kept)"""
    o = order(s, allowed, excluded)
    o = o[o != t]
    return int(np.count_nonzero((s[o] > s[t]) | ((s[o] == s[t]) & (o < t))))


def in_range(s, radius, allowed=None, excluded=()):
    """the rows of the residual order whose score is strictly above float64(radius)"""
    o = order(s, allowed, excluded)
    return o[s[o] > np.float64(np.float32(radius))]


def docs(s, col, k, allowed=None, excluded=()):
    """(D, ids, rows) of the first k documents of the residual order: the first row per id"""
    seen, D, K, R = set(), [], [], []
    for r in order(s, allowed, excluded):
        if int(col[r]) in seen:
            continue
        seen.add(int(col[r]))
        D.append(np.float32(s[r])), K.append(int(col[r])), R.append(int(r))
        if len(K) == k:
            break
    pad = k - len(K)
    return (np.array(D + [PAD_SCORE] * pad, np.float32), np.array(K + [-1] * pad, np.int64), np.array(R + [-1] * pad, np.int64))


def brute_order(s, allowed, excluded):
    rows = [r for r in range(len(s)) if (allowed is None or allowed[r]) and r not in set(int(x) for x in excluded)]
    out = []
    while rows:                 # selection by the definition: the best remaining row, the lowest on equal scores
        best = rows[0]
        for r in rows[1:]:
            if s[r] > s[best] or (s[r] == s[best] and r < best):
                best = r
        out.append(best)
        rows.remove(best)
    return out


def brute_rank(s, t, allowed, excluded):
    ex = set(int(x) for x in excluded)
    return sum(1 for r in range(len(s)) if r != t and (allowed is None or allowed[r]) and r not in ex
               and (s[r] > s[t] or (s[r] == s[t] and r < t)))


# ---- the recipes --------------------------------------------------------------------------------------------------------------
def recipe(name, S, k, allowed=None):
    """one int64 list per query (any order, repeats, -1 padding), built from the oracle's ranking of the allowed rows"""
    nq, n = S.shape
    rs = np.random.RandomState(1000 + n + k)
    lists = []
    for j in range(nq):
        o = order(S[j], allowed)
        if name == "none":
            e = np.full(3, -1, np.int64)
        elif name == "top1":
            e = o[:1]
        elif name == "whole_topk":
            e = o[:k]
        elif name == "scattered":
            ranks = [r for r in (0, 2, 3, 7, k - 1, k, k + 5) if r < len(o)]
            far = [r for r in (2 * k + 1, 2 * k + 2, 2 * k + 9, 2 * k + 40, len(o) - 1) if 2 * k < r < len(o)]
            e = o[np.array(ranks + far, np.int64)] if ranks else o[:0]
            e = np.concatenate([e, e[:3], np.full(4, -1, np.int64)])            # repeats and padding
            e = e[rs.permutation(len(e))]                                       # interleaved, unsorted
        elif name == "uneven":
            want = (37 * j) % 301
            pick = np.array([r for r in range(len(o)) if r % 3 != 1][:want], np.int64)
            e = o[pick][::-1]
        elif name == "nearly_all":
            e = np.delete(o, [1, 5, 100, len(o) - 1]) if j == 0 else o[:0]
        else:
            raise AssertionError(name)
        lists.append(np.asarray(e, np.int64))
    return lists


def padded(lists):
    """the lists as one int64 array [nq, e], -1 padded"""
    out = np.full((len(lists), max([len(e) for e in lists] + [1])), -1, np.int64)
    for j, e in enumerate(lists):
        out[j, :len(e)] = e
    return out


def e_max(lists, n):
    return max(len(clean(e, n)) for e in lists)


def bites(S, k, lists, allowed=None):
    """does any list remove a row from the top-k of its query?"""
    return any(len(np.intersect1d(order(S[j], allowed)[:k], clean(lists[j], S.shape[1]))) for j in range(S.shape[0]))
