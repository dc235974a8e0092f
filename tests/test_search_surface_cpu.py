"""The surface of convdr_amd.search, pinned against the commit BEFORE search.py was split into staging / toplists /
block_search / index_store: every name the module offered, every attribute of FlatIPIndex and every signature.

tests/golden/search_surface.json was RECORDED from that parent commit (`python tests/test_search_surface_cpu.py --record` with
that version of convdr_amd first on the path, CONVDR_SURFACE_PACKAGE_ROOT), not from the code under test.  The branch may
offer more; it may not offer less, and no recorded callable may change its parameters or defaults."""
import inspect
import json
import os
import subprocess
import sys
import types

import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.environ.get("CONVDR_SURFACE_PACKAGE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from convdr_amd import search as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "search_surface.json")

# what left search.py, by the module that owns it now
MOVED = {
    "staging": ("_STAGING", "_STAGING_THREADS", "_STAGING_LOCK", "_STAGING_BUILD", "_POOLS", "_NUMA", "gpu_numa_cpus", "_on_cpus",
                "pinned_near", "_staging_key", "_staging", "_copy_pool"),
    "toplists": ("merge_topk", "merge_topk_sorted", "merge_topk_device", "MERGE_KERNEL_MAX", "distinct_topk", "distinct_topk_device",
                 "DISTINCT_KERNEL_MAX", "DISTINCT_DEEP_WS_BYTES", "_check_max_depth", "_distinct_row_depth"),
    "block_search": ("load_block", "search_one_by_one", "search_distinct_one_by_one", "_search_block_list",
                     "_check_distinct_certificate", "EvalDevQuery", "_Passages", "_load_collection"),
    "index_store": ("pack_row_mask", "RowFilter", "DocOrdinals", "RESERVED_ID", "ROW_FILTER_TILE", "HALF_NORM_LIMIT", "KEY_ST_LIST",
                    "KEY_ST_PROBE", "KEY_ST_COLUMN", "KEY_ST_NOSET", "_KINDS", "_HALF_PRECISIONS"),
}


def _signature(obj):
    """[[parameter name, kind, repr(default) or None], ...] of a callable; None where inspect finds no signature"""
    try:
        sig = inspect.signature(obj)
    except (TypeError, ValueError):
        return None
    return [[p.name, p.kind.name, None if p.default is p.empty else repr(p.default)] for p in sig.parameters.values()]


def surface():
    names = {}
    for name, obj in vars(S).items():
        if (name.startswith("__") and name.endswith("__")) or isinstance(obj, types.ModuleType):
            continue
        names[name] = _signature(obj) if callable(obj) else "value"
    attrs = {}
    for name in dir(S.FlatIPIndex):
        if name.startswith("__") and name.endswith("__") and name != "__init__":
            continue
        static = inspect.getattr_static(S.FlatIPIndex, name)
        if isinstance(static, property):
            attrs[name] = "property"
        else:
            obj = getattr(S.FlatIPIndex, name)
            attrs[name] = _signature(obj) if callable(obj) else "value"
    return {"module": names, "FlatIPIndex": attrs}


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("part", ["module", "FlatIPIndex"])
def test_every_recorded_name_is_still_offered_with_its_signature(recorded, part):
    now = surface()[part]
    assert len(recorded[part]) >= (54 if part == "module" else 113)     # (the record is the whole surface, not a sample)
    missing = sorted(set(recorded[part]) - set(now))
    assert not missing, "%s no longer offers %s" % (part, missing)
    changed = {n: (was, now[n]) for n, was in recorded[part].items() if now[n] != was}
    assert not changed, changed


def test_a_moved_name_is_one_object_in_search_and_in_its_module(recorded):
    import importlib
    for module, names in MOVED.items():
        owner = importlib.import_module("convdr_amd." + module)
        for name in names:
            assert name in recorded["module"], name
            assert getattr(S, name) is getattr(owner, name), (module, name)
    assert S.FlatIPIndex.__mro__[1].__module__ == "convdr_amd.index_store"
    assert S.FlatIPIndex.__module__ == "convdr_amd.search"


def test_the_dependency_runs_one_way():
    """nothing below search.py brings search.py in"""
    code = ("import sys\n"
            "import convdr_amd.index_store, convdr_amd.toplists, convdr_amd.staging\n"
            "assert 'convdr_amd.search' not in sys.modules, 'search was imported'\n")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_search_surface_cpu.py --record    (writes %s)" % GOLDEN)
    print("recording from", S.__file__)
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
