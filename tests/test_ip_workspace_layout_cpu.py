"""The workspace layout of the three search plans (shallow, deep, range) is part of the ABI in practice: the debug accessors and
convdr_ip_range_pack find regions by offset, and callers size and poison the workspace by the byte counts.  The fixture
tests/golden/ip_workspace_layout.json records, over a grid of shapes (both query tile classes, ragged and empty blocks, both
ends of every cap range, n up to 2^31 - 1, and shapes outside the contract), what the library returned BEFORE the three plans
were given a common base and one workspace cursor; every later library must reproduce every value.  Pure host arithmetic."""
import json
import os

from convdr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sizes_and_region_offsets_are_the_recorded_ones():
    L = _lib.lib()
    with open(os.path.join(ROOT, "tests", "golden", "ip_workspace_layout.json")) as f:
        rec = json.load(f)
    base = rec["base"]
    for name in ("convdr_ip_workspace_bytes", "convdr_ip_deep_workspace_bytes", "convdr_ip_range_workspace_bytes"):
        assert len(rec[name]) > 400
        for *args, want in rec[name]:
            assert getattr(L, name)(*args) == want, (name, args, want)
        assert any(r[-1] == 0 for r in rec[name]) and any(r[-1] > 0 for r in rec[name])
    for name in ("convdr_ip_debug_counts", "convdr_ip_debug_band"):     # (these offsets depend on nq and d only: a coarser grid)
        assert len(rec[name]) >= 48
        for *args, want in rec[name]:
            assert getattr(L, name)(base, *args) - base == want, (name, args, want)
    # the raw scan scores (test aids): list ids / scores, and the threshold sample with its pitch (-1: the plan has no sample).
    # The same coarse grid, plus shapes with cap < n <= 32,768 (the sample is the whole block) -- these offsets depend on n.
    import ctypes as C
    for name, second in (("convdr_ip_debug_list", C.c_void_p), ("convdr_ip_debug_sample", C.c_int64)):
        assert len(rec[name]) >= 48
        for *args, want_a, want_b in rec[name]:
            a, b = C.c_void_p(), second()
            assert getattr(L, name)(base, *args, C.byref(a), C.byref(b)) == 0, (name, args)
            got_a = -1 if a.value is None else a.value - base
            got_b = b.value - base if second is C.c_void_p else b.value
            assert (got_a, got_b) == (want_a, want_b), (name, args, got_a, got_b)
    assert any(r[-2] == -1 for r in rec["convdr_ip_debug_sample"]) and any(r[-2] > 0 for r in rec["convdr_ip_debug_sample"])
    # list, sample and the two older accessors describe ONE plan: counts < band < sample <= list ids < list scores
    for (*args, o_id, o_s), (*_, o_T, ld) in zip(rec["convdr_ip_debug_list"], rec["convdr_ip_debug_sample"]):
        nq, cap = args[0], args[4]
        assert o_s - o_id == (nq * cap * 4 + 255) // 256 * 256 and ld >= nq and ld % 128 == 0, args
        band = L.convdr_ip_debug_band(base, *args) - base
        assert band < (o_T if o_T >= 0 else o_id) <= o_id, args
