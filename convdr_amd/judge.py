"""Judging a run on the device: qrels labels, rank measures and ranking negatives (include/convdr_hip.h, "Judging a run").

The reference judges a search result on the host, three ways: ``EvalDevQuery`` looks every (query, rank) up in a dict
(drivers/run_convdr_inference.py:98-99), the measures come from trec_eval run on the .trec file it writes, and the negatives
of the ranking file come from two walks over a text run file (data/gen_ranking_data.py:539-567).  All three join a ranked
key list with a per-query judged set; here that join is one kernel (``label_run``) and the other two read its labels:

    K, labels, m = judge_run(D, I, qrels, key_map=offset2pid)      # from raw search output, nothing leaves the device
    m.mean()["recip_rank"]                                         # the one host read
    keys, rows, counts = run_negatives(K, labels, qrels, rows=I_distinct)
    doc_embs = idx.rows_tensors(rows[j, :m])                       # m <= counts[j] negatives of query j, no host text

The measures are the usual trec_eval per-query definitions, restated in include/convdr_hip.h and in tests/judge_cases.py; they
are claimed to agree with THOSE FORMULAS, not with the trec_eval binary (which this project never runs).
"""
import csv
import ctypes as C

import numpy as np

from . import _lib

LABEL_PAD = -2 ** 31             # CONVDR_LABEL_PAD: the entry is padding
LABEL_UNJUDGED = -2 ** 31 + 1    # CONVDR_LABEL_UNJUDGED: the key is not in the query's segment
GRADE_MIN, GRADE_MAX = -2 ** 31 + 2, 2 ** 31 - 1
MAX_N = 65536                    # FlatIPIndex.DEEP_MAX_K
MAX_CUTOFFS = 16
BASE_COLUMNS = ("num_rel", "num_rel_ret", "recip_rank", "map")


def _torch():
    import torch
    return torch


def ideal_grades(off, grade):
    """Per segment: the positive grades sorted descending, then zeros (int32 [nnz]); what the IDCG reads as a prefix."""
    off, grade = np.asarray(off, np.int64), np.asarray(grade, np.int64)
    gain = np.where(grade > 0, grade, 0)
    seg = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return gain[np.lexsort((-gain, seg))].astype(np.int32)


def _checked(off, key, grade, ideal):
    """The four arrays as numpy (int64, int64, int32, int32), or ValueError."""
    try:
        off = np.asarray(off, dtype=np.int64).reshape(-1)
        key = np.asarray(key, dtype=np.int64).reshape(-1)
        grade = np.asarray(grade, dtype=np.int64).reshape(-1)
    except OverflowError as e:
        raise ValueError("Qrels: a value does not fit 64 bits (%s)" % e)
    nnz = len(key)
    if len(grade) != nnz:
        raise ValueError("Qrels: %d keys but %d grades" % (nnz, len(grade)))
    if len(off) < 1 or off[0] != 0 or off[-1] != nnz or (np.diff(off) < 0).any():
        raise ValueError("Qrels: off must start at 0, never decrease and end at nnz = %d" % nnz)
    if nnz:
        if grade.min() < GRADE_MIN or grade.max() > GRADE_MAX:
            raise ValueError("Qrels: grades must lie in [-2^31 + 2, 2^31 - 1] (the two values below are the label sentinels); "
                             "got %d..%d" % (grade.min(), grade.max()))
        inner = np.ones(nnz, bool)                      # entries that have a predecessor in their own segment
        inner[off[:-1][off[:-1] < nnz]] = False
        if (np.diff(key) <= 0)[inner[1:]].any():
            raise ValueError("Qrels: keys must be strictly ascending inside every segment")
    want = ideal_grades(off, grade)
    if ideal is not None:
        ideal = np.asarray(ideal).reshape(-1)
        if ideal.shape != want.shape or (ideal != want).any():
            raise ValueError("Qrels: ideal must hold every segment's positive grades sorted descending, then zeros")
    return off, key, grade.astype(np.int32), want


class Qrels:
    """The device form of ``{qid: {pid: rel}}``, aligned to the query order of a search (``query_embedding2id``):

        off    int64 [nq + 1]  segment offsets
        key    int64 [nnz]     the judged pids of query j in key[off[j]:off[j + 1]], strictly ascending
        grade  int32 [nnz]     the judgement; <= 0 is judged non-relevant
        ideal  int32 [nnz]     per segment the positive grades sorted descending, then zeros

    Everything is checked on the host when it is packed (ValueError); the kernels take the arrays as they are."""

    def __init__(self, off, key, grade, ideal=None, device=None):
        torch = _torch()
        host = [np.asarray(t.cpu()) if torch.is_tensor(t) else t for t in (off, key, grade, ideal)]
        off, key, grade, ideal = _checked(*host)
        if device is None:
            device = "cuda"
        self.nq, self.nnz = len(off) - 1, len(key)
        self.device = torch.device(device)
        self.off, self.key, self.grade, self.ideal = (torch.from_numpy(a).to(self.device) for a in (off, key, grade, ideal))

    @classmethod
    def from_dict(cls, qrels, qids, device=None):
        """qrels: {qid: {pid: rel}}; qids: the queries in search order.  A query missing from the dict gets an empty segment."""
        off, key, grade = [0], [], []
        for qid in qids:
            judged = qrels.get(qid) or {}
            try:
                items = sorted((int(p), int(r)) for p, r in judged.items())
            except (TypeError, ValueError) as e:
                raise ValueError("Qrels: pids and grades must be integers (query %r: %s)" % (qid, e))
            if any(r < GRADE_MIN or r > GRADE_MAX for _, r in items):
                raise ValueError("Qrels: grades must lie in [-2^31 + 2, 2^31 - 1] (query %r)" % (qid,))
            key += [p for p, _ in items]
            grade += [r for _, r in items]
            off.append(len(key))
        return cls(off, key, grade, device=device)

    @classmethod
    def from_file(cls, path, qids, device=None):
        """The 4-column TSV both reference scripts read (``topicid \\t _ \\t docid \\t rel``; run_convdr_inference.py:374-385,
        gen_ranking_data.py:512-516).  Every line is kept at every grade; for a repeated (topic, doc) the last line wins.
        Topics are compared as strings (``str(qid)``)."""
        qrels = {}
        with open(path, "r", encoding="utf8") as f:
            for row in csv.reader(f, delimiter="\t"):
                if not row:
                    continue
                if len(row) != 4:
                    raise ValueError("%s: expected 4 tab-separated columns, got %r" % (path, row))
                topicid, _, docid, rel = row
                qrels.setdefault(str(topicid), {})[int(docid)] = int(rel)
        return cls.from_dict({qid: qrels.get(str(qid), {}) for qid in qids}, qids, device=device)


def _need_device(who, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.ConvdrError("%s: tensors must live on the GPU (there is no CPU path)" % who)


def _rows_of(who, t, qrels, dtype):
    torch = _torch()
    if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 2:
        raise ValueError("%s: expected a 2-d %s tensor" % (who, dtype))
    nq, n = int(t.shape[0]), int(t.shape[1])
    if qrels.nq != nq:
        raise ValueError("%s: %d rows but the qrels hold %d queries (off has %d entries)" % (who, nq, qrels.nq, qrels.nq + 1))
    if n > MAX_N:
        raise ValueError("%s: n = %d is beyond %d (FlatIPIndex.DEEP_MAX_K)" % (who, n, MAX_N))
    return nq, n


def _pitched(t, n):
    """(tensor with unit column stride, its row pitch in elements)."""
    if t.numel() and (t.stride(1) != 1 or t.stride(0) < n):
        t = t.contiguous()
    return t, max(int(t.stride(0)), n)


def label_run(K, qrels):
    """labels int32 [nq, n] of a ranked key list K int64 [nq, n] (``distinct_topk_device``'s K; -1 pads anywhere): the grade of
    each key in its query's segment, LABEL_UNJUDGED for a key that is not there, LABEL_PAD for padding.  No sync."""
    torch = _torch()
    nq, n = _rows_of("label_run", K, qrels, torch.int64)
    _need_device("label_run", K, qrels.off)
    K, ld = _pitched(K, n)
    labels = torch.empty((nq, n), dtype=torch.int32, device=K.device)
    with torch.cuda.device(K.device):
        _lib.check(_lib.lib().convdr_run_label(_lib.ptr(K), n, ld, nq, _lib.ptr(qrels.off), _lib.ptr(qrels.key), _lib.ptr(qrels.grade),
                                               qrels.nnz, _lib.ptr(labels), _lib.stream_ptr()), "convdr_run_label")
    return labels


class Measures:
    """per_query: device fp64 [nq, len(columns)]; columns: "num_rel", "num_rel_ret", "recip_rank", "map", then "ndcg_cut_c",
    "recall_c" and "P_c" for every cutoff c."""

    def __init__(self, per_query, columns):
        self.per_query, self.columns = per_query, tuple(columns)

    def mean(self):
        """The one host read.  This project's own averaging rule: the mean of every column over the queries with num_rel > 0
        (a query without a relevant judgement says nothing about a ranking), and their number under "num_q"."""
        pq = self.per_query.cpu().numpy()
        judged = pq[pq[:, 0] > 0] if len(pq) else pq
        means = judged.mean(0) if len(judged) else np.zeros(len(self.columns))
        out = {c: float(v) for c, v in zip(self.columns, means)}
        out["num_q"] = len(judged)
        return out


def measure_columns(cutoffs):
    return BASE_COLUMNS + tuple("%s_%d" % (m, c) for m in ("ndcg_cut", "recall", "P") for c in cutoffs)


def run_measures(labels, qrels, cutoffs=(3, 10, 100), rel_level=1):
    """Per-query rank measures from ``label_run``'s labels -> Measures.  An entry is relevant iff label >= rel_level; its gain
    is max(label, 0) at every rel_level.  cutoffs: at most 16, >= 1, strictly ascending.  No sync."""
    torch = _torch()
    cutoffs = tuple(int(c) for c in cutoffs)
    rel_level = int(rel_level)
    if len(cutoffs) > MAX_CUTOFFS or any(c < 1 or c > GRADE_MAX for c in cutoffs) or any(b <= a for a, b in zip(cutoffs, cutoffs[1:])):
        raise ValueError("run_measures: at most %d cutoffs, each >= 1, strictly ascending (got %r)" % (MAX_CUTOFFS, cutoffs))
    if rel_level < 1 or rel_level > GRADE_MAX:
        raise ValueError("run_measures: rel_level must be >= 1 (got %d)" % rel_level)
    nq, n = _rows_of("run_measures", labels, qrels, torch.int32)
    _need_device("run_measures", labels, qrels.off)
    labels = labels.contiguous()
    columns = measure_columns(cutoffs)
    out = torch.empty((nq, len(columns)), dtype=torch.float64, device=labels.device)
    cuts = (C.c_int32 * max(len(cutoffs), 1))(*cutoffs)
    with torch.cuda.device(labels.device):
        _lib.check(_lib.lib().convdr_run_measures(_lib.ptr(labels), n, nq, _lib.ptr(qrels.off), _lib.ptr(qrels.grade),
                                                  _lib.ptr(qrels.ideal), qrels.nnz, rel_level, cuts, len(cutoffs), _lib.ptr(out),
                                                  _lib.stream_ptr()), "convdr_run_measures")
    return Measures(out, columns)


def run_negatives(K, labels, qrels, fill_to=20, rows=None):
    """The ranking negatives of data/gen_ranking_data.py:539-567 from one ranked list per query -> (keys, rows or None, counts):
    keys (and rows, when the row ids ``rows`` of the same entries are given) int64 [nq, max(n, fill_to)] padded with -1, counts
    int32 [nq].  A query with no qrels entry of grade > 0 gets nothing.  Otherwise the list is A followed by B:

      A  every entry judged with a grade <= 0, in list order, uncapped;
      B  the first max(0, fill_to - |A|) entries, in list order, that are not positives (grade <= 0 or not judged).

    B repeats members of A: the reference's second pass appends every non-positive it meets without checking whether the
    first pass already took it, and this reproduces that.  Sampling ``num_negs`` of the list (the reference's
    ``random.sample``) stays with the caller.  The qrels are needed for "has a positive at all", which the labels of the
    retrieved entries cannot tell.  No sync."""
    torch = _torch()
    fill_to = int(fill_to)
    if fill_to < 0 or fill_to > MAX_N:
        raise ValueError("run_negatives: fill_to = %d outside [0, %d]" % (fill_to, MAX_N))
    nq, n = _rows_of("run_negatives", K, qrels, torch.int64)
    if tuple(labels.shape) != (nq, n) or labels.dtype != torch.int32:
        raise ValueError("run_negatives: labels must be int32 [%d, %d]" % (nq, n))
    if rows is not None and (tuple(rows.shape) != (nq, n) or rows.dtype != torch.int64):
        raise ValueError("run_negatives: rows must be int64 [%d, %d]" % (nq, n))
    _need_device("run_negatives", K, labels, rows, qrels.off)
    K, ld = _pitched(K, n)
    if rows is not None:
        rows, ldr = _pitched(rows, n)
        if ldr != ld:
            K, rows, ld = K.contiguous(), rows.contiguous(), n
    labels = labels.contiguous()
    W = max(n, fill_to)
    keys = torch.empty((nq, W), dtype=torch.int64, device=K.device)
    out_rows = None if rows is None else torch.empty((nq, W), dtype=torch.int64, device=K.device)
    counts = torch.empty((nq,), dtype=torch.int32, device=K.device)
    with torch.cuda.device(K.device):
        _lib.check(_lib.lib().convdr_run_negatives(_lib.ptr(K), _lib.ptr(rows), n, ld, nq, _lib.ptr(labels), _lib.ptr(qrels.off),
                                                   _lib.ptr(qrels.grade), qrels.nnz, fill_to, _lib.ptr(keys), _lib.ptr(out_rows),
                                                   _lib.ptr(counts), _lib.stream_ptr()), "convdr_run_negatives")
    return keys, out_rows, counts


def judge_run(D, I, qrels, key_map=None, topN=None, cutoffs=(3, 10, 100), rel_level=1):
    """From raw search output (what ``EvalDevQuery`` is handed: D fp32 / I int64 [nq, n] device tensors, key_map = offset2pid as
    a device int64 vector or None) to (K, labels, measures): ``distinct_topk_device(D, I, topN or n, key_map)``, then
    ``label_run``, then ``run_measures``.  No sync."""
    from .search import distinct_topk_device
    n = int(I.shape[1])
    if qrels.nq != int(I.shape[0]):
        raise ValueError("judge_run: %d rows but the qrels hold %d queries (off has %d entries)" % (I.shape[0], qrels.nq, qrels.nq + 1))
    _, _, K, _ = distinct_topk_device(D, I, n if topN is None else int(topN), key_map)
    labels = label_run(K, qrels)
    return K, labels, run_measures(labels, qrels, cutoffs=cutoffs, rel_level=rel_level)
