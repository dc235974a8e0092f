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
