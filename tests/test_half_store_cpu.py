"""The half-precision passage store (FlatIPIndex(storage="fp16"), include/convdr_hip.h "Half-precision passage store"),
the parts that need no GPU: argument validation of the three C entries, the header / export agreement, float16 blocks
out of the corpus-encode loop, and the constructor's argument check."""
import json
import os
import pickle
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from convdr_amd import _lib, blocks, encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("convdr_ip_store_rows_f16", "convdr_ip_search_h16", "convdr_ip_search_deep_h16")


def _store(L, d=768, scale=4.0, n=10, src=None, store=None, f32=0):
    return L.convdr_ip_store_rows_f16(src, f32, n, d, scale, store, None, None, None)


def _search(L, name, d=768, scale=4.0, k=100, cap=4096, n=100000):
    return getattr(L, name)(None, 5, None, scale, 0, n, d, k, None, None, cap, 0, None, 0, None, None, None, None, None)


@pytest.mark.parametrize("name,cap,big_k", [("convdr_ip_search_h16", 4096, 2049), ("convdr_ip_search_deep_h16", 16384, 8193)])
def test_search_entries_reject_bad_arguments_before_any_device_call(name, cap, big_k):
    """Every pointer is NULL and the workspace has 0 bytes: a call that got past validation could not return these messages."""
    L = _lib.lib()
    for kw, msg in (({"d": 70}, b"d % 64"), ({"scale": 0.75}, b"power of two"), ({"scale": 0.5}, b"power of two >= 1"),
                    ({"k": big_k}, b"too large for cap")):
        rc = _search(L, name, cap=cap, **kw)
        assert rc != 0 and msg in L.convdr_last_error(), (name, kw, L.convdr_last_error())
    assert _search(L, name, cap=cap, k=big_k - 1) != 0 and b"workspace too small" in L.convdr_last_error()   # (the first check past them)


def test_deep_entry_rejects_blocks_of_2_to_the_31_rows():
    L = _lib.lib()
    assert _search(L, "convdr_ip_search_deep_h16", cap=16384, n=1 << 31) != 0 and b"2^31" in L.convdr_last_error()


def test_store_rows_rejects_bad_arguments_before_any_device_call():
    L = _lib.lib()
    assert _store(L, d=70) != 0 and b"d % 64" in L.convdr_last_error()
    assert _store(L, scale=0.75) != 0 and b"power of two" in L.convdr_last_error()
    assert _store(L, scale=0.0) != 0 and b"power of two" in L.convdr_last_error()
    assert _store(L, scale=float("inf")) != 0 and b"power of two" in L.convdr_last_error()
    # a factor below 1 is the in-place rescale of a half store only: not out of place, not from fp32 rows
    assert _store(L, scale=0.5, src=1 << 20, store=2 << 20) != 0 and b">= 1" in L.convdr_last_error()
    assert _store(L, scale=0.5, src=1 << 20, store=1 << 20, f32=1) != 0 and b">= 1" in L.convdr_last_error()
    assert _store(L, scale=4.0, src=1 << 20, store=2 << 20) != 0 and b"flags" in L.convdr_last_error()
    assert _store(L, n=0) == 0                                      # nothing to do, nothing launched


def test_header_ctypes_and_exports_agree_on_the_new_entries():
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "convdr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(convdr_[a-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(L, name), name
    assert declared == set(_lib.exported_symbols()), declared ^ set(_lib.exported_symbols())
    # argument counts of the ctypes signatures against the header's parameter lists
    for name in NEW:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(params.split(",")) == len(_lib._SIGNATURES[name][1]), name


def test_constructor_checks_its_arguments_before_it_looks_for_a_gpu(monkeypatch):
    from convdr_amd.search import FlatIPIndex
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for kw in ({"precision": "bf16"}, {"precision": "fp16x3"}, {"precision": "bf16x3"}, {"center": True}):
        with pytest.raises(ValueError):
            FlatIPIndex(768, storage="fp16", **kw)
    with pytest.raises(ValueError):
        FlatIPIndex(768, storage="int8")
    with pytest.raises(_lib.ConvdrError):                          # valid arguments: only the GPU is missing
        FlatIPIndex(768, storage="fp16", precision="fp16x2")


# ---- float16 blocks out of the encode loop (a stand-in tower on the host path encode_shard supports) ---------------------
class _Tower:
    def __init__(self, dim=768):
        self.W = torch.from_numpy(np.random.RandomState(5).randn(500, dim).astype(np.float32))

    def embed(self, ids, mask, head=None, seq_lens=None):
        lens = torch.as_tensor(np.asarray(seq_lens), dtype=torch.int64)
        live = (torch.arange(ids.shape[1])[None, :] < lens[:, None]).float()
        return (self.W[ids.long()] * live[:, :, None]).sum(1) * 0.37


class _Model:
    def __init__(self, base_len=None):
        self.roberta, self.embeddingHead, self.norm = _Tower(), None, None
        if base_len:
            self.base_len = base_len

    def parameters(self):
        return iter([self.roberta.W])


def _write_cache(path, n, L, seed=4):
    rs = np.random.RandomState(seed)
    lens = rs.randint(1, L + 1, size=n)
    ids = rs.randint(3, 500, size=(n, L)).astype(np.int32)
    with open(path, "wb") as f:
        for i in range(n):
            ids[i, lens[i]:] = 0
            f.write(int(lens[i]).to_bytes(4, "big") + ids[i].tobytes())
    with open(path + "_meta", "w") as f:
        json.dump({"type": "int32", "total_number": n, "embedding_size": L}, f)


@pytest.mark.parametrize("base_len", [None, 8])
def test_encode_shard_rounds_to_half_once(tmp_path, base_len):
    _write_cache(str(tmp_path / "passages"), 37, 16)
    with blocks.TokenCache(str(tmp_path / "passages")) as cache:
        e32, i32 = encode.encode_shard(_Model(base_len), cache, 1, 2, 5)
        e16, i16 = encode.encode_shard(_Model(base_len), cache, 1, 2, 5, out_dtype=np.float16)
        empty, _ = encode.encode_shard(_Model(base_len), cache, 40, 41, 5, out_dtype=np.float16)
        with pytest.raises(ValueError):
            encode.encode_shard(_Model(base_len), cache, out_dtype=np.float64)
    assert e32.dtype == np.float32 and e16.dtype == np.float16 and empty.dtype == np.float16 and len(empty) == 0
    assert np.abs(e32).max() > 1.0 and (e32 != e16.astype(np.float32)).any()        # (the rounding is not vacuous)
    np.testing.assert_array_equal(e16.view(np.uint16), e32.astype(np.float16).view(np.uint16))
    np.testing.assert_array_equal(i16, i32)


@pytest.mark.parametrize("how", ["keyword", "args.emb_dtype"])
def test_stream_inference_doc_writes_a_float16_block(tmp_path, how):
    """800 x 768 halves = 1.2 MB: past the size where dump_block writes the streamed block format BlockView maps."""
    n = 800
    _write_cache(str(tmp_path / "passages"), n, 6)
    outs = {}
    for tag in ("f32", "f16"):
        args = SimpleNamespace(output_dir=str(tmp_path / tag), per_gpu_eval_batch_size=128, max_seq_length=6)
        kw = {}
        if tag == "f16" and how == "keyword":
            kw["out_dtype"] = np.float16
        elif tag == "f16":
            args.emb_dtype = "float16"
        with blocks.TokenCache(str(tmp_path / "passages")) as cache:
            outs[tag] = encode.StreamInferenceDoc(args, _Model(), cache, **kw)
    want = outs["f32"][0].astype(np.float16)
    assert outs["f16"][0].dtype == np.float16
    with blocks.BlockView(str(tmp_path / "f16" / "passage__emb_p__data_obj_0.pb")) as view:
        assert view.array.dtype == np.float16 and view.array.shape == (n, 768)
        np.testing.assert_array_equal(view.array.view(np.uint16), want.view(np.uint16))
        part = np.empty((300, 768), np.float16)
        view.read_rows_into(part, 100, 400)
        np.testing.assert_array_equal(part.view(np.uint16), want[100:400].view(np.uint16))
    with open(str(tmp_path / "f16" / "passage__emb_p__data_obj_0.pb"), "rb") as h:           # still a pickle the reference's loader reads
        np.testing.assert_array_equal(pickle.load(h).view(np.uint16), want.view(np.uint16))
    a = open(str(tmp_path / "f16" / "passage__embid_p__data_obj_0.pb"), "rb").read()
    b = open(str(tmp_path / "f32" / "passage__embid_p__data_obj_0.pb"), "rb").read()
    assert a == b
