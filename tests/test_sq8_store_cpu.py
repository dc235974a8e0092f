"""The 8-bit store (FlatIPIndex(storage="sq8")) without a GPU: the numpy model of tests/sq8_cases.py held to the documented band
on every family, the ranges of the integer operands, the quantiser's edge cases, the argument validation of the new C entries
and the entries the store refuses."""
import numpy as np
import pytest

from tests import sq8_cases as M

f32 = np.float32


def _model(fam, d, nq, n):
    Q, P = M.family(fam, d, nq, n)
    centre = P.astype(np.float64).mean(axis=0).astype(f32)
    step = M.step_of(P, centre)
    codes, sat = M.codes_of(P, centre, step)
    hi, lo, te = M.query_split(Q, step)
    return Q, P, centre, step, codes, sat, hi, lo, te


@pytest.mark.parametrize("d", [128, 768, 1024])
@pytest.mark.parametrize("fam", M.FAMILIES)
def test_integer_scan_is_inside_the_documented_band(fam, d):
    Q, P, centre, step, codes, sat, hi, lo, te = _model(fam, d, 16, 2000)
    assert sat == 0 and codes.min() >= -127                         # the first add never saturates, -128 is never stored
    S, s_hi, s_lo = M.int_scan(hi, lo, codes)
    assert np.abs(S).max() < 2 ** 31 and np.abs(128 * s_hi).max() < 2 ** 31
    Sf = S.astype(f32).astype(np.float64)                           # the int-to-float conversion, round to nearest even
    E = M.exact_scaled(Q, codes, centre, step, te)
    eps = M.eps_doc(Q, codes, centre, step, te)
    ratio = np.abs(Sf - E) / eps[:, None]
    print("SQ8ERR-model %-9s d=%-4d max |S~ - E| / eps_doc = %.4f" % (fam, d, ratio.max()))
    assert ratio.max() <= 1.0, (fam, d, ratio.max())
    if fam == "saturated":
        assert (np.abs(codes) == 127).all()


@pytest.mark.parametrize("fam", M.FAMILIES)
def test_hi_and_lo_stay_in_range(fam):
    Q, P, centre, step, codes, sat, hi, lo, te = _model(fam, 768, 64, 500)
    assert hi.min() >= -127 and hi.max() <= 127 and lo.min() >= -64 and lo.max() <= 63
    qi = 128 * hi.astype(np.int64) + lo
    assert np.abs(qi).max() <= M.QMAX
    assert (np.abs(qi).max(axis=1) > M.QMAX // 2).all()             # t is the SMALLEST admitted power of two


def test_int32_holds_the_widest_row_of_extreme_codes():
    d = 1024
    codes = np.full((2, d), 127, dtype=np.int8)
    codes[1] = -127
    Q = np.full((1, d), 3.0, dtype=f32)                             # equal magnitudes: every Qi at the limit
    hi, lo, te = M.query_split(Q, np.ones(d, dtype=f32))
    qi = 128 * hi.astype(np.int64) + lo
    assert (qi == qi[0, 0]).all() and M.QMAX // 2 < int(qi[0, 0]) <= M.QMAX
    S, s_hi, s_lo = M.int_scan(hi, lo, codes)
    for v in (S, 128 * s_hi, s_hi, s_lo):
        assert np.abs(v).max() < 2 ** 31
    assert d * 127 * M.QMAX < 2 ** 31 <= (d + 128) * 127 * M.QMAX      # the bound the entries' d <= 1024 rests on


def test_constant_column_and_saturation():
    rs = np.random.RandomState(3)
    P = rs.randn(300, 128).astype(f32)
    P[:, 5] = f32(2.5)
    centre = P.astype(np.float64).mean(axis=0).astype(f32)
    step = M.step_of(P, centre)
    codes, sat = M.codes_of(P, centre, step)
    assert step[5] == 0 and (codes[:, 5] == 0).all() and sat == 0
    v = M.reconstruct(codes, centre, step)
    assert (v[:, 5] == centre[5]).all()
    assert np.abs(v - P).max() <= 0.5 * step.max() * (1 + 1e-5) + 1e-6
    later = (P * f32(3)).astype(f32)                                # a later add outside the first add's range
    codes2, sat2 = M.codes_of(later, centre, step)
    want = int((np.abs(np.rint((later - centre)[:, step > 0] / step[step > 0])) > 127).sum())
    assert sat2 == want > 0 and np.abs(codes2.astype(int)).max() == 127 and codes2.min() >= -127


def test_new_c_entries_validate_their_arguments_without_a_gpu():
    from convdr_amd import _lib
    L = _lib.lib()
    one = 1 << 20            # a non-NULL address that must never be dereferenced
    assert L.convdr_ip_store_rows_q8(one, 10, 192, one, one, one, one, one, one, None) != 0 and b"d % 128" in L.convdr_last_error()
    assert L.convdr_ip_store_rows_q8(one, 10, 1152, one, one, one, one, one, one, None) != 0 and b"1024" in L.convdr_last_error()
    assert L.convdr_ip_store_rows_q8(None, 10, 128, one, one, one, one, one, one, None) != 0 and b"NULL" in L.convdr_last_error()
    assert L.convdr_ip_column_absdev(one, 0, 128, one, one, one, None) != 0 and b"empty" in L.convdr_last_error()
    assert L.convdr_ip_column_absdev(one, 5, 128, None, one, one, None) != 0 and b"NULL" in L.convdr_last_error()
    ws = L.convdr_ip_workspace_bytes(5, 2000, 192, 10, 1024)
    args = (one, 5, one, one, one, 2000, 192, 10, one, None, 1024, 0, one, ws, one, one, one, one, None)
    assert L.convdr_ip_search_q8(*args) != 0 and b"d % 128" in L.convdr_last_error() and b"convdr_ip_search_q8" in L.convdr_last_error()
    args = (one, 5, one, one, one, 2000, 128, 10, one, None, 1000, 0, one, ws, one, one, one, one, None)
    assert L.convdr_ip_search_q8(*args) != 0 and b"cap" in L.convdr_last_error()
    args = (one, 5, None, one, one, 2000, 128, 10, one, None, 1024, 0, one, ws, one, one, one, one, None)
    assert L.convdr_ip_search_q8(*args) != 0 and b"NULL" in L.convdr_last_error()
    args = (one, 5, one, one, one, 2000, 128, 5000, one, None, 16384, 0, one, 0, one, one, one, one, None)
    assert L.convdr_ip_search_deep_q8(*args) != 0 and b"workspace" in L.convdr_last_error()
    args = (2, one, 5, one, one, one, 2000, 128, 10, one, None, 1024, 0, one, ws, one, 64, 10, one, one, one, one, None)
    assert L.convdr_ip_search_filtered_q8(*args) != 0 and b"deep" in L.convdr_last_error()
    args = (0, one, 5, one, one, one, 2000, 128, 10, one, None, 1024, 0, one, ws, None, 64, 10, one, one, one, one, None)
    assert L.convdr_ip_search_filtered_q8(*args) != 0 and b"row_bits" in L.convdr_last_error()
    args = (0, one, 5, one, one, one, 2000, 128, 10, one, None, 1024, 0, one, ws, 16, 8, 10, one, one, one, one, None)
    assert L.convdr_ip_search_filtered_q8(*args) != 0 and b"bitmap" in L.convdr_last_error()
    assert L.convdr_ip_score_rows_q8(one, 2, one, one, one, 10, 100, one, 1, 1, one, one, None) != 0 and b"d % 128" in L.convdr_last_error()
    assert L.convdr_ip_score_rows_q8(one, 2, None, one, one, 10, 128, one, 1, 1, one, one, None) != 0 and b"NULL" in L.convdr_last_error()


def test_constructor_checks_come_before_the_device():
    from convdr_amd.search import FlatIPIndex
    with pytest.raises(ValueError, match="sq8"):
        FlatIPIndex(768, storage="sq8", precision="fp16", prepin=False)
    with pytest.raises(ValueError, match="sq8"):
        FlatIPIndex(1100, storage="sq8", prepin=False)
    with pytest.raises(ValueError, match="sq8"):
        FlatIPIndex(768, storage="sq8", center=False, prepin=False)
    with pytest.raises(ValueError, match="sq8"):
        FlatIPIndex(768, storage="fp32", precision="i8", prepin=False)
    with pytest.raises(ValueError, match="'sq8'"):
        FlatIPIndex(768, storage="int4", prepin=False)


def test_refused_entries_raise_naming_the_storage():
    from convdr_amd import index_store, stores
    from convdr_amd.search import FlatIPIndex
    idx = object.__new__(FlatIPIndex)           # no device: every refusal comes before anything else is touched
    idx._store, idx.storage = stores.STORES["sq8"], "sq8"
    q, v = np.zeros((1, 128), dtype=f32), np.zeros(1, dtype=np.int64)
    calls = {"range_search": (q, 0.0), "range_search_tensors": (q, 0.0), "range_count": (q, 0.0), "rank_rows": (q, v),
             "rank_rows_tensors": (q, v), "rank_ids": (q, v), "rank_ids_tensors": (q, v), "excluding": ([[0]],),
             "score_ids": (q, v), "score_ids_tensors": (q, v), "search_docs": (q, 1), "search_distinct": (q, 1, v),
             "update_rows": (0, q), "upsert": (v, q), "upsert_docs": (v, v, q)}
    assert sorted(calls) == sorted(index_store.SQ8_REFUSED)
    for name, args in calls.items():
        with pytest.raises(ValueError, match="storage='sq8'"):
            getattr(idx, name)(*args)
