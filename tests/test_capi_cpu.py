"""The C-ABI library builds, loads without a GPU and exports every symbol that
include/convdr_hip.h declares (no compute calls here)."""
import os
import re

from convdr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    names = set()
    for fn in os.listdir(os.path.join(ROOT, "include")):
        src = open(os.path.join(ROOT, "include", fn)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names |= set(re.findall(r"\b(convdr_[a-z0-9_]+)\s*\(", src))
    return names


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    declared = _declared()
    assert declared, "no declarations found"
    for name in declared:
        assert hasattr(L, name), "libconvdr_hip.so does not export %s" % name
    assert declared == set(_lib.exported_symbols()), declared ^ set(_lib.exported_symbols())
    assert L.convdr_version() >= 100


# entries whose declaration tests/capi_decl.py cannot read, each with the reason (at most 5: beyond that the pattern wants mending)
UNPARSED = {}


def test_every_ctypes_signature_has_the_declared_parameter_count():
    from tests import capi_decl
    assert len(UNPARSED) <= 5
    for name, (_, argtypes) in _lib._SIGNATURES.items():
        if name in UNPARSED:
            continue
        params = capi_decl.params(name).strip()
        declared = 0 if params in ("", "void") else len(params.split(","))
        assert declared == len(argtypes), "%s: the header declares %d parameters, _lib._SIGNATURES has %d" % (name, declared, len(argtypes))
    assert set(UNPARSED) <= set(_lib._SIGNATURES)


def test_scan_score_accessors_are_declared_bound_and_refuse_null():
    """convdr_ip_debug_list / convdr_ip_debug_sample: the argument list of convdr_ip_debug_counts plus two out-pointers."""
    import ctypes as C
    from tests import capi_decl
    L = _lib.lib()
    head = capi_decl.params("convdr_ip_debug_counts").strip()
    for name, tail in (("convdr_ip_debug_list", ("const uint32_t** id", "const float** s")),
                       ("convdr_ip_debug_sample", ("const float** T", "int64_t* ld"))):
        assert name in _declared() and name in _lib.exported_symbols()
        params = [p.strip() for p in capi_decl.params(name).split(",")]
        assert ", ".join(params[:-2]) == ", ".join(p.strip() for p in head.split(",")) and tuple(params[-2:]) == tail, params
        assert getattr(L, name)(None, 1, 10, 64, 1, 1024, None, None) != 0 and name.encode() in L.convdr_last_error()
    base, T, ld = 1 << 20, C.c_void_p(), C.c_int64()
    assert L.convdr_ip_debug_sample(base, 5, 1024, 64, 10, 1024, C.byref(T), C.byref(ld)) == 0 and T.value is None and ld.value == 128
    assert L.convdr_ip_debug_sample(base, 5, 1025, 64, 10, 1024, C.byref(T), C.byref(ld)) == 0 and T.value > base


def test_argument_validation_needs_no_gpu():
    L = _lib.lib()
    assert L.convdr_ip_workspace_bytes(1000, 1_000_000, 768, 100, 4096) > 0
    rc = L.convdr_ip_prepare_block(None, 10, 70, None, None, None, None, None)     # d % 64 != 0 -> rejected before any launch
    assert rc != 0 and b"d % 64" in L.convdr_last_error()


def test_product_path_has_no_cpu_fallback():
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from convdr_amd.search import FlatIPIndex
    with pytest.raises(_lib.ConvdrError):
        FlatIPIndex(768)
