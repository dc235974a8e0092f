"""Judging a run, the parts that need no GPU: the oracle on a hand-worked case, Qrels packing and validation, and the argument
checks of the three C entries (which return before anything touches a device)."""
import ctypes as C
import math

import numpy as np
import pytest

from convdr_amd import _lib, judge
from tests import judge_cases as JC

U, P = JC.UNJUDGED, JC.PAD
LIST = [5, 9, 2, 7, 3]
QRELS = {9: 2, 3: 1, 4: 3, 7: 0}


def test_sentinels_agree_with_the_header():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "convdr_hip.h")).read()
    pad = re.search(r"#define CONVDR_LABEL_PAD \((-?\d+) - 1\)", src)
    unj = re.search(r"#define CONVDR_LABEL_UNJUDGED \((-?\d+)\)", src)
    assert int(pad.group(1)) - 1 == judge.LABEL_PAD == P == -2 ** 31
    assert int(unj.group(1)) == judge.LABEL_UNJUDGED == U == -2 ** 31 + 1
    assert judge.GRADE_MIN == U + 1 and judge.MAX_N == 65536


def test_hand_worked_case():
    labels = JC.labels_of(LIST, QRELS)
    assert labels == [U, 2, U, 0, 1]
    got = dict(zip(JC.columns((3,)), JC.measures_of(labels, QRELS, (3,), 1)))
    # relevant at level 1: grades 2, 1, 3 (pids 9, 3, 4) -> three; retrieved at ranks 2 and 5
    assert got["num_rel"] == 3.0 and got["num_rel_ret"] == 2.0
    assert got["recip_rank"] == 1.0 / 2
    assert got["map"] == (1 / 2 + 2 / 5) / 3
    dcg3 = 2 / math.log2(2 + 1)                                          # only rank 2 gains inside the first three
    idcg3 = 3 / math.log2(1 + 1) + 2 / math.log2(2 + 1) + 1 / math.log2(3 + 1)      # ideal 3, 2, 1
    assert idcg3 == 3 + 2 / math.log2(3) + 1 / 2
    assert got["ndcg_cut_3"] == dcg3 / idcg3
    assert got["recall_3"] == 1 / 3 and got["P_3"] == 1 / 3
    assert JC.negatives_of(LIST, QRELS, 3)[0] == [7, 5, 2]               # A = [7]; B = the first two non-positives
    assert JC.negatives_of(LIST, QRELS, 20)[0] == [7, 5, 2, 7]           # B runs out of list after 5, 2, 7: 7 twice
    assert JC.negatives_of(LIST, QRELS, 0)[0] == [7]                     # A is not capped
    assert JC.negatives_of(LIST, {7: 0, 5: -1}, 20)[0] == []             # no positive at all: nothing
    rows = [50, 90, 20, 70, 30]
    assert JC.negatives_of(LIST, QRELS, 3, rows) == ([7, 5, 2], [70, 50, 20])


def test_hand_worked_case_at_level_two():
    labels = JC.labels_of(LIST, QRELS)
    got = dict(zip(JC.columns((1, 3, 9)), JC.measures_of(labels, QRELS, (1, 3, 9), 2)))
    # relevant at level 2: grades 2 and 3 (pids 9, 4); only 9 is retrieved, at rank 2.  The gains do not move with the level.
    assert got["num_rel"] == 2.0 and got["num_rel_ret"] == 1.0
    assert got["recip_rank"] == 0.5 and got["map"] == (1 / 2) / 2
    idcg = 3 + 2 / math.log2(3) + 1 / 2
    assert got["ndcg_cut_1"] == 0.0
    assert got["ndcg_cut_3"] == (2 / math.log2(3)) / idcg
    assert got["ndcg_cut_9"] == (2 / math.log2(3) + 1 / math.log2(6)) / idcg        # the list ends at 5: min(c, n)
    assert (got["recall_1"], got["recall_3"], got["recall_9"]) == (0.0, 0.5, 0.5)
    assert (got["P_1"], got["P_3"], got["P_9"]) == (0.0, 1 / 3, 1 / 9)              # P divides by c, not by min(c, n)


def test_padding_and_wide_keys_in_the_oracle():
    hi = JC.HIGH
    judged = {7: 1, 7 + hi: 0}
    assert JC.labels_of([-1, 7 + hi, 7, -1, 8], judged) == [P, 0, 1, P, U]
    got = JC.measures_of([P, 0, 1, P, U], judged, (2,), 1)
    assert got[:3] == [1.0, 1.0, 1 / 3]                                  # padding keeps its rank slot
    assert JC.negatives_of([-1, 7 + hi, 7, -1, 8], judged, 3)[0] == [7 + hi, 7 + hi, 8]


def test_generated_cases_cover_the_ground():
    """The generator the GPU tests draw from does produce what they are meant to meet (two small shapes stand for all)."""
    seen = set()
    for nq, n in ((5, 100), (37, 100)):
        c = JC.case(nq, n)
        assert c["K"].shape == (nq, n + JC.PITCH_EXTRA) and c["cutoffs"] == (1, 3, 10, 100, 105)
        for q in range(nq):
            keys, judged, lab = c["K"][q, :n].tolist(), c["judged"][q], c["labels"][q].tolist()
            real = [k for k in keys if k >= 0]
            assert len(set(real)) == len(real)
            pos = {k for k, g in judged.items() if g > 0}
            seen.add("segment of %d" % len(judged))
            seen.add("no positive" if not pos else "all retrieved" if pos <= set(real) else
                     "none retrieved" if not pos & set(real) else "some retrieved")
            if lab[0] > 0:
                seen.add("relevant at rank 1")
            if lab[-1] > 0:
                seen.add("relevant at rank n")
            if keys[-1] < 0:
                seen.add("padding tail")
            if any(a < 0 <= b for a, b in zip(keys, keys[1:])):
                seen.add("padding inside")
            if any(k >= JC.HIGH and (k ^ JC.HIGH) in judged for k in real) or any(k < JC.HIGH and (k ^ JC.HIGH) in judged for k in real):
                seen.add("a key that differs from a judged one only above bit 32")
            if sum(1 for x in lab if JC.UNJUDGED < x <= 0) > 20:
                seen.add("more judged negatives than fill_to")
            if any(g == 2 ** 31 - 1 for g in judged.values()) and any(g < 0 for g in judged.values()):
                seen.add("grades from negative to 2^31 - 1")
            if 0 < c["negatives"][20][2][q] < 20:
                seen.add("fewer non-positives than fill_to")
    want = {"segment of %d" % s for s in JC.SEGMENTS} | {
        "no positive", "all retrieved", "none retrieved", "some retrieved", "relevant at rank 1", "relevant at rank n",
        "padding tail", "padding inside", "a key that differs from a judged one only above bit 32",
        "more judged negatives than fill_to", "grades from negative to 2^31 - 1"}
    assert want <= seen, sorted(want - seen)


# ---- Qrels -------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.cpu().numpy()


def test_qrels_from_dict():
    q = judge.Qrels.from_dict({"a": {9: 2, 3: 1, 4: 3, 7: 0}, "c": {1: 0, 5 + JC.HIGH: 4, 5: -2}}, ["a", "b", "c", "a"], device="cpu")
    assert (q.nq, q.nnz) == (4, 11)
    assert _np(q.off).tolist() == [0, 4, 4, 7, 11] and q.off.dtype.is_floating_point is False
    assert _np(q.key).tolist() == [3, 4, 7, 9, 1, 5, 5 + JC.HIGH, 3, 4, 7, 9]
    assert _np(q.grade).tolist() == [1, 3, 0, 2, 0, -2, 4, 1, 3, 0, 2]
    assert _np(q.ideal).tolist() == [3, 2, 1, 0, 4, 0, 0, 3, 2, 1, 0]
    assert str(q.key.dtype) == "torch.int64" and str(q.grade.dtype) == "torch.int32" and str(q.ideal.dtype) == "torch.int32"
    empty = judge.Qrels.from_dict({}, [], device="cpu")
    assert (empty.nq, empty.nnz) == (0, 0) and _np(empty.off).tolist() == [0]


def test_qrels_from_arrays_and_validation():
    off, key, grade = [0, 2, 2, 5], [3, 8, 1, 2, 3], [1, 0, 2, 5, -1]
    q = judge.Qrels(off, key, grade, device="cpu")
    assert _np(q.ideal).tolist() == [1, 0, 5, 2, 0]
    q2 = judge.Qrels(np.asarray(off), np.asarray(key), np.asarray(grade, np.int32), ideal=[1, 0, 5, 2, 0], device="cpu")
    assert _np(q2.key).tolist() == key and q2.nq == 3
    bad = [
        ([0, 2, 1, 5], key, grade, None),                      # off decreases
        ([0, 2, 2, 4], key, grade, None),                      # off does not end at nnz
        ([1, 2, 2, 5], key, grade, None),                      # off does not start at 0
        ([], key, grade, None),
        (off, [3, 3, 1, 2, 3], grade, None),                   # equal keys inside a segment
        (off, [8, 3, 1, 2, 3], grade, None),                   # descending keys inside a segment
        (off, key, [1, 0, 2, 5], None),                        # lengths
        (off, key, [1, 0, 2, -2 ** 31, -1], None),             # the PAD sentinel as a grade
        (off, key, [1, 0, 2, -2 ** 31 + 1, -1], None),         # the UNJUDGED sentinel as a grade
        (off, key, [1, 0, 2, 2 ** 31, -1], None),              # beyond int32
        (off, key, grade, [0, 1, 5, 2, 0]),                    # ideal not sorted
        (off, key, grade, [1, 0, 5, 2]),
    ]
    for o, k, g, i in bad:
        with pytest.raises(ValueError):
            judge.Qrels(o, k, g, ideal=i, device="cpu")
    # the boundary values are grades; a segment boundary may step down in key
    ok = judge.Qrels(off, [3, 8, 1, 2, 3], [1, 0, 2 ** 31 - 1, -2 ** 31 + 2, -1], device="cpu")
    assert _np(ok.grade).tolist() == [1, 0, 2 ** 31 - 1, -2 ** 31 + 2, -1]
    for d in ({1: {2: 2 ** 31}}, {1: {2: -2 ** 31 + 1}}, {1: {"x": 1}}):
        with pytest.raises(ValueError):
            judge.Qrels.from_dict(d, [1], device="cpu")


def test_a_failed_pack_leaves_nothing_behind():
    class Probe(judge.Qrels):
        pass
    try:
        obj = Probe([0, 2], [4, 4], [1, 1], device="cpu")
    except ValueError:
        obj = None
    assert obj is None
    shell = Probe.__new__(Probe)
    with pytest.raises(ValueError):
        shell.__init__([0, 2], [4, 4], [1, 1], device="cpu")
    assert not vars(shell), "a rejected pack set %s" % sorted(vars(shell))


def test_qrels_from_file(tmp_path):
    path = tmp_path / "qrels.tsv"
    path.write_text("31_1\t0\t100\t2\n"
                    "31_1\t0\t7\t0\n"
                    "31_2\t0\t5\t0\n"             # a query with only grade-0 lines keeps them
                    "31_2\t0\t9\t0\n"
                    "31_1\t0\t100\t1\n"           # a repeated (topic, doc): the last line wins
                    "31_1\t0\t8589934599\t3\n"    # 7 + 2^33
                    "99\tQ0\t1\t-1\n", encoding="utf8")
    q = judge.Qrels.from_file(str(path), ["31_2", "31_1", "77", 99], device="cpu")
    assert _np(q.off).tolist() == [0, 2, 5, 5, 6]
    assert _np(q.key).tolist() == [5, 9, 7, 100, 8589934599, 1]
    assert _np(q.grade).tolist() == [0, 0, 0, 1, 3, -1]
    assert _np(q.ideal).tolist() == [0, 0, 3, 1, 0, 0]
    (tmp_path / "bad.tsv").write_text("1\t0\t2\n", encoding="utf8")
    with pytest.raises(ValueError):
        judge.Qrels.from_file(str(tmp_path / "bad.tsv"), ["1"], device="cpu")


def test_python_surface_checks_need_no_gpu():
    import torch
    q = judge.Qrels.from_dict({0: {1: 1}}, [0, 1], device="cpu")
    K3 = torch.zeros((3, 4), dtype=torch.int64)
    L2 = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="3 entries"):
        judge.label_run(K3, q)
    with pytest.raises(ValueError, match="3 entries"):
        judge.run_measures(torch.zeros((3, 4), dtype=torch.int32), q)
    with pytest.raises(ValueError, match="3 entries"):
        judge.run_negatives(K3, torch.zeros((3, 4), dtype=torch.int32), q)
    with pytest.raises(ValueError, match="3 entries"):
        judge.judge_run(torch.zeros((3, 4)), K3, q)
    for cutoffs in ((10, 3), (3, 3), (0, 1), tuple(range(1, 18))):
        with pytest.raises(ValueError, match="cutoffs"):
            judge.run_measures(L2, q, cutoffs=cutoffs)
    with pytest.raises(ValueError, match="rel_level"):
        judge.run_measures(L2, q, rel_level=0)
    with pytest.raises(ValueError, match="fill_to"):
        judge.run_negatives(K3[:2], L2, q, fill_to=-1)
    with pytest.raises(ValueError, match="65536"):
        judge.label_run(torch.zeros((2, 65537), dtype=torch.int64), q)
    with pytest.raises(_lib.ConvdrError):                       # no CPU path
        judge.label_run(K3[:2], q)
    assert judge.measure_columns((3, 10)) == JC.columns((3, 10))


# ---- the C entries ----------------------------------------------------------------------------------------------------------
def _fails(rc, L, *words):
    msg = L.convdr_last_error()
    assert rc != 0, "accepted"
    for w in words:
        assert w in msg, (w, msg)


def test_argument_validation_needs_no_gpu():
    L = _lib.lib()
    p = C.c_void_p(256)                      # a non-NULL pointer nobody dereferences: every call below fails its checks first
    cuts = (C.c_int32 * 17)(*range(1, 18))
    down = (C.c_int32 * 2)(10, 3)
    # convdr_run_label(K, n, ld, nq, off, key, grade, nnz, labels, stream)
    _fails(L.convdr_run_label(None, 5, 5, 2, p, p, p, 4, p, None), L, b"convdr_run_label", b"NULL")
    _fails(L.convdr_run_label(p, 5, 5, 2, None, p, p, 4, p, None), L, b"NULL")
    _fails(L.convdr_run_label(p, 5, 5, 2, p, None, p, 4, p, None), L, b"NULL")
    _fails(L.convdr_run_label(p, 5, 5, 2, p, p, p, 4, None, None), L, b"NULL")
    _fails(L.convdr_run_label(p, 65537, 65537, 2, p, p, p, 4, p, None), L, b"n=65537")
    _fails(L.convdr_run_label(p, -1, 5, 2, p, p, p, 4, p, None), L, b"n=-1")
    _fails(L.convdr_run_label(p, 5, 5, -2, p, p, p, 4, p, None), L, b"nq=-2")
    _fails(L.convdr_run_label(p, 5, 5, 2, p, p, p, -4, p, None), L, b"nnz=-4")
    _fails(L.convdr_run_label(p, 5, 4, 2, p, p, p, 4, p, None), L, b"pitch")
    # convdr_run_measures(labels, n, nq, off, grade, ideal, nnz, rel_level, cutoffs, n_cutoffs, out, stream)
    _fails(L.convdr_run_measures(None, 5, 2, p, p, p, 4, 1, cuts, 2, p, None), L, b"convdr_run_measures", b"NULL")
    _fails(L.convdr_run_measures(p, 5, 2, None, p, p, 4, 1, cuts, 2, p, None), L, b"NULL")
    _fails(L.convdr_run_measures(p, 5, 2, p, p, None, 4, 1, cuts, 2, p, None), L, b"NULL")
    _fails(L.convdr_run_measures(p, 5, 2, p, p, p, 4, 1, cuts, 2, None, None), L, b"NULL")
    _fails(L.convdr_run_measures(p, 5, 2, p, p, p, 4, 1, None, 2, p, None), L, b"cutoffs is NULL")
    _fails(L.convdr_run_measures(p, 65537, 2, p, p, p, 4, 1, cuts, 2, p, None), L, b"n=65537")
    _fails(L.convdr_run_measures(p, 5, 2, p, p, p, 4, 1, cuts, 17, p, None), L, b"at most 16 cutoffs")
    _fails(L.convdr_run_measures(p, 5, 2, p, p, p, 4, 1, cuts, -1, p, None), L, b"cutoffs")
    _fails(L.convdr_run_measures(p, 5, 2, p, p, p, 4, 1, down, 2, p, None), L, b"strictly ascending")
    _fails(L.convdr_run_measures(p, 5, 2, p, p, p, 4, 0, cuts, 2, p, None), L, b"rel_level")
    _fails(L.convdr_run_measures(p, -5, 2, p, p, p, 4, 1, cuts, 2, p, None), L, b"n=-5")
    _fails(L.convdr_run_measures(p, 5, -1, p, p, p, 4, 1, cuts, 2, p, None), L, b"nq=-1")
    # convdr_run_negatives(K, I, n, ld, nq, labels, off, grade, nnz, fill_to, out_keys, out_rows, counts, stream)
    _fails(L.convdr_run_negatives(None, None, 5, 5, 2, p, p, p, 4, 20, p, None, p, None), L, b"convdr_run_negatives", b"NULL")
    _fails(L.convdr_run_negatives(p, None, 5, 5, 2, None, p, p, 4, 20, p, None, p, None), L, b"NULL")
    _fails(L.convdr_run_negatives(p, None, 5, 5, 2, p, None, p, 4, 20, p, None, p, None), L, b"NULL")
    _fails(L.convdr_run_negatives(p, None, 5, 5, 2, p, p, p, 4, 20, None, None, p, None), L, b"NULL")
    _fails(L.convdr_run_negatives(p, None, 5, 5, 2, p, p, p, 4, 20, p, None, None, None), L, b"NULL")
    _fails(L.convdr_run_negatives(p, p, 5, 5, 2, p, p, p, 4, 20, p, None, p, None), L, b"out_rows is NULL")
    _fails(L.convdr_run_negatives(p, None, 5, 5, 2, p, p, p, 4, 20, p, p, p, None), L, b"I is NULL")
    _fails(L.convdr_run_negatives(p, None, 65537, 65537, 2, p, p, p, 4, 20, p, None, p, None), L, b"n=65537")
    _fails(L.convdr_run_negatives(p, None, 5, 5, 2, p, p, p, 4, -1, p, None, p, None), L, b"fill_to=-1")
    _fails(L.convdr_run_negatives(p, None, 5, 5, 2, p, p, p, 4, 65537, p, None, p, None), L, b"fill_to=65537")
    _fails(L.convdr_run_negatives(p, None, 5, 5, -2, p, p, p, 4, 20, p, None, p, None), L, b"nq=-2")
    _fails(L.convdr_run_negatives(p, None, 5, 3, 2, p, p, p, 4, 20, p, None, p, None), L, b"pitch")
    # nothing to do is not an error, and needs no pointer at all
    assert L.convdr_run_label(None, 5, 5, 0, None, None, None, 0, None, None) == 0
    assert L.convdr_run_measures(None, 5, 0, None, None, None, 0, 1, cuts, 3, None, None) == 0
    assert L.convdr_run_negatives(None, None, 5, 5, 0, None, None, None, 0, 20, None, None, None, None) == 0
