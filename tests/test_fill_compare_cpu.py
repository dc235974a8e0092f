"""The comparison helper of tests/test_stale_memory_gpu.py must itself be sensitive: plain CPU tensors."""
import pytest
import torch

from tests.helpers import FILLS, assert_fills_agree, fill_bytes


def _runs():
    g = torch.Generator().manual_seed(0)
    emb = torch.randn(5, 16, generator=g)
    ids = torch.arange(10).reshape(5, 2)
    return {f: ({"emb": emb.clone(), "I": ids.clone()}, (1000, 2000), (1000, 2000)) for f in FILLS + ("S",)}


def test_identical_runs_pass():
    assert_fills_agree(_runs(), "same")


def test_one_differing_element_fails():
    r = _runs()
    r["R"][0]["emb"][3, 7] = torch.nextafter(r["R"][0]["emb"][3, 7], torch.tensor(10.0))      # one ulp
    with pytest.raises(AssertionError, match="depends on the scratch memory"):
        assert_fills_agree(r, "ulp")
    r = _runs()
    r["S"][0]["I"][4, 1] += 1
    with pytest.raises(AssertionError, match="depends on the scratch memory"):
        assert_fills_agree(r, "index")


def test_one_nan_fails():
    r = _runs()
    r["N"][0]["emb"][0, 0] = float("nan")
    with pytest.raises(AssertionError, match="depends on the scratch memory"):
        assert_fills_agree(r, "nan")
    r = _runs()
    for f in r:                                  # "all fills equally wrong": NaN at the same place in every run
        r[f][0]["emb"][2, 2] = float("nan")
    with pytest.raises(AssertionError, match="not finite"):
        assert_fills_agree(r, "nan everywhere")


def test_changed_buffer_pointer_fails():
    r = _runs()
    r["N"] = (r["N"][0], (1000, 2000), (1000, 4096))
    with pytest.raises(AssertionError, match="did not use"):
        assert_fills_agree(r, "ptr")


def test_missing_baseline_or_output_fails():
    r = _runs()
    del r["Z"]
    with pytest.raises(AssertionError):
        assert_fills_agree(r, "no Z")
    r = _runs()
    del r["R"][0]["I"]
    with pytest.raises(AssertionError):
        assert_fills_agree(r, "missing output")


def test_fill_bytes_patterns():
    for dt in (torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.uint8):
        t = torch.ones(33, dtype=dt)
        assert fill_bytes(t, "Z").view(torch.uint8).sum() == 0
        assert bool((fill_bytes(t, "N").view(torch.uint8) == 0xFF).all())
        a = fill_bytes(t, "R", seed=3).clone()
        b = fill_bytes(torch.zeros(33, dtype=dt), "R", seed=3)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and len(torch.unique(a.view(torch.uint8))) > 8
    assert bool(torch.isnan(fill_bytes(torch.zeros(4), "N")).all())
    assert fill_bytes(torch.zeros(3, dtype=torch.int64), "N").tolist() == [-1, -1, -1]
