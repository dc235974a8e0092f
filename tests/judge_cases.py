"""Shared cases of the run-judging tests (CPU and GPU): the oracle, written from the definitions in include/convdr_hip.h
("Judging a run") with dict lookups and plain loops in Python floats, and the generator of ranked lists and qrels.

  labels     the grade of the key in the query's dict, UNJUDGED when it is not there, PAD for a negative key;
  measures   ranks start at 1; relevant iff label >= rel_level, gain = max(label, 0); every sum is made in ascending rank;
  negatives  the two passes over the list: first the judged non-positives, then non-positives of any kind until the list
             holds fill_to entries (the second pass does not look at what the first one took)."""
import functools
import math

import numpy as np

PAD, UNJUDGED = -2 ** 31, -2 ** 31 + 1
HIGH = 1 << 32


def columns(cutoffs):
    return ("num_rel", "num_rel_ret", "recip_rank", "map") + tuple("ndcg_cut_%d" % c for c in cutoffs) + \
        tuple("recall_%d" % c for c in cutoffs) + tuple("P_%d" % c for c in cutoffs)


def labels_of(keys, judged):
    return [PAD if k < 0 else judged.get(k, UNJUDGED) for k in keys]


def measures_of(labels, judged, cutoffs, rel_level):
    """One query's row, in the order of columns(cutoffs)."""
    n = len(labels)
    rel = [lab >= rel_level and lab not in (PAD, UNJUDGED) for lab in labels]
    gain = [lab if lab > 0 and lab not in (PAD, UNJUDGED) else 0 for lab in labels]
    num_rel = sum(1 for g in judged.values() if g >= rel_level)
    num_rel_ret = sum(rel)
    recip_rank, ap, seen = 0.0, 0.0, 0
    for r in range(1, n + 1):
        if rel[r - 1]:
            seen += 1
            if seen == 1:
                recip_rank = 1.0 / r
            ap += seen / r
    ideal = sorted((g for g in judged.values() if g > 0), reverse=True)
    ndcg, recall, prec = [], [], []
    for c in cutoffs:
        dcg = 0.0
        for r in range(1, min(c, n) + 1):
            dcg += gain[r - 1] / math.log2(r + 1)
        idcg = 0.0
        for r in range(1, min(c, len(ideal)) + 1):
            idcg += ideal[r - 1] / math.log2(r + 1)
        hits = sum(rel[:min(c, n)])
        ndcg.append(dcg / idcg if idcg > 0 else 0.0)
        recall.append(hits / num_rel if num_rel else 0.0)
        prec.append(hits / c)
    return [float(num_rel), float(num_rel_ret), recip_rank, ap / num_rel if num_rel else 0.0] + ndcg + recall + prec


def negatives_of(keys, judged, fill_to, rows=None):
    """-> (negative keys, their rows or None) of one query."""
    positives = {p for p, g in judged.items() if g > 0}
    judged_neg = {p for p, g in judged.items() if g <= 0}
    out = []
    if not positives:
        return out, (None if rows is None else [])
    for i, k in enumerate(keys):                       # first pass: retrieved and judged non-relevant
        if k >= 0 and k not in positives and k in judged_neg:
            out.append(i)
    for i, k in enumerate(keys):                       # second pass: anything that is not a positive, up to fill_to in all
        if len(out) >= fill_to:
            break
        if k >= 0 and k not in positives:
            out.append(i)
    return [keys[i] for i in out], (None if rows is None else [rows[i] for i in out])


# ---- generated cases ----------------------------------------------------------------------------------------------------
SEGMENTS = (0, 1, 2, 33, 5000)                       # judged entries per query, cycled over the queries
MODES = ("mixed", "nopos", "allret", "noneret", "first", "last", "tailpad", "midpad")
GRADES = (-5, -1, 0, 0, 1, 1, 2, 3, 2 ** 31 - 1)
FILL_TO = (0, 3, 20)
PITCH_EXTRA = 3                                      # K is a view of a wider buffer: row pitch n + 3


def cutoffs_for(n):
    """1, exactly n, and beyond n, among the usual ones."""
    return tuple(sorted({1, 3, 10, max(n, 1), n + 5}))


def _query(rs, n, seg, mode):
    m = 3 * (n + seg) + 8
    perm = rs.permutation(m).astype(np.int64)
    jk = perm[:seg].copy()
    jk[rs.rand(seg) < 0.5] += HIGH                     # half of the judged keys live above bit 32 ...
    grades = rs.choice((-3, 0, 0, -1) if mode == "nopos" else GRADES, size=seg)
    judged = {int(k): int(g) for k, g in zip(jk, grades)}
    if mode in ("first", "last") and seg and not any(g > 0 for g in judged.values()):
        judged[int(jk[0])] = 2
    n_pad = {"tailpad": n // 3, "midpad": n // 4}.get(mode, 0)
    n_real = n - n_pad
    pos = [k for k, g in judged.items() if g > 0]
    neg = [k for k, g in judged.items() if g <= 0]
    if mode == "allret":
        take = pos + neg[:len(neg) // 2]
    elif mode == "noneret":
        take = neg[:len(neg) // 2 + 1]
    else:
        take = [k for k in judged if rs.rand() < 0.5]
    take = take[:n_real]
    twins = [k ^ HIGH for k in list(judged)[:8]]       # ... and their twins below it are NOT judged (and the other way round)
    fresh = [int(k) for k in perm[seg:]]
    rest = (twins + fresh)[:n_real - len(take)]
    keys = take + rest
    keys = [keys[i] for i in rs.permutation(len(keys))]
    if mode in ("first", "last") and pos and keys:
        p = pos[0]
        if p in keys:
            keys.remove(p)
        else:
            keys.pop()
        keys.insert(0 if mode == "first" else len(keys), p)
    assert len(keys) == n_real and len(set(keys)) == n_real
    if mode == "midpad":
        for at in sorted(rs.randint(0, n_real + 1, size=n_pad).tolist(), reverse=True):
            keys.insert(at, -1)
    else:
        keys += [-1] * n_pad
    return keys, judged


@functools.lru_cache(maxsize=None)
def case(nq, n, seed=0):
    """-> dict: K int64 [nq, n + PITCH_EXTRA] (the list in the first n columns, other keys behind it), I (row ids of the
    same entries, -1 under padding), judged (a dict per query), cutoffs, and the oracle's answers: labels, measures[rel_level],
    negatives[fill_to] = (keys, rows, counts) padded as the kernel pads.  Computed once per shape; treat it as read-only."""
    rs = np.random.RandomState(1000 * seed + 7 * nq + n)
    K = rs.randint(0, 1 << 40, size=(nq, n + PITCH_EXTRA)).astype(np.int64)
    I = rs.randint(0, 1 << 30, size=(nq, n + PITCH_EXTRA)).astype(np.int64)
    judged = []
    for q in range(nq):
        keys, j = _query(rs, n, SEGMENTS[(q + n) % len(SEGMENTS)], MODES[(q + n + seed) % len(MODES)])
        K[q, :n] = keys
        judged.append(j)
    I[:, :n][K[:, :n] < 0] = -1
    cuts = cutoffs_for(n)
    out = {"K": K, "I": I, "n": n, "nq": nq, "judged": judged, "cutoffs": cuts}
    lab = [labels_of(K[q, :n].tolist(), judged[q]) for q in range(nq)]
    out["labels"] = np.asarray(lab, np.int32).reshape(nq, n)
    out["measures"] = {lvl: np.asarray([measures_of(lab[q], judged[q], cuts, lvl) for q in range(nq)],
                                       np.float64).reshape(nq, 4 + 3 * len(cuts)) for lvl in (1, 2)}
    out["negatives"] = {}
    for fill_to in FILL_TO:
        w = max(n, fill_to)
        nk, nr, cnt = np.full((nq, w), -1, np.int64), np.full((nq, w), -1, np.int64), np.zeros(nq, np.int32)
        for q in range(nq):
            kk, rr = negatives_of(K[q, :n].tolist(), judged[q], fill_to, I[q, :n].tolist())
            nk[q, :len(kk)], nr[q, :len(rr)], cnt[q] = kk, rr, len(kk)
        out["negatives"][fill_to] = (nk, nr, cnt)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
