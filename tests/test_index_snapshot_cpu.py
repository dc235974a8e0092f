"""Snapshots, the parts that need no GPU: the two digest entries are declared and exported, every refusal (argument validation
happens before anything touches a device), convdr_digest_host against the numpy oracle of tests/snapshot_cases.py, and the
snapshot file format of convdr_amd/snapshot.py against the reference writer and reader there: round trip, verify_file naming
the section and window of a flipped byte, every refusal of read_header, the atomic write."""
import ctypes
import os
import struct

import numpy as np
import pytest

from convdr_amd import _lib, snapshot
from convdr_amd import search as S
from tests import capi_decl
from tests import snapshot_cases as C

ENTRIES = ("convdr_digest_rows", "convdr_digest_host")
P = 1 << 20                     # a pointer that is never dereferenced on the host (16-byte aligned)
W = 256                         # window_rows of the file tests: 1,300 rows make 6 windows, the last one short


def test_header_ctypes_and_exports_agree_on_the_entries():
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.exported_symbols() and hasattr(L, name)
        assert len(capi_decl.params(name).split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert S.snapshot_info is snapshot.read_header and S.verify_snapshot is snapshot.verify_file
    for name in ("save", "load", "fingerprint"):
        assert callable(getattr(S.FlatIPIndex, name))


def _refused(L, name, rc, msg):
    err = L.convdr_last_error()
    assert rc < 0 and msg in err and name in err, (name, rc, msg, err)


def test_every_refusal_of_the_device_entry_is_a_negative_code_with_a_message():
    L = _lib.lib()
    name = b"convdr_digest_rows"

    def rows(buf=P, n_rows=100, row_bytes=64, word0=0, window_rows=10, out=P):
        return L.convdr_digest_rows(buf, n_rows, row_bytes, word0, window_rows, out, None)
    for rb in (0, 12, -8):
        _refused(L, name, rows(row_bytes=rb), b"row_bytes")
    _refused(L, name, rows(buf=P + 4), b"8-byte aligned")
    _refused(L, name, rows(window_rows=0), b"window_rows")
    _refused(L, name, rows(window_rows=-3), b"window_rows")
    _refused(L, name, rows(n_rows=-1), b"bad row count")
    _refused(L, name, rows(out=None), b"NULL argument")
    _refused(L, name, rows(buf=None), b"NULL argument")
    _refused(L, name, rows(n_rows=0, row_bytes=12), b"row_bytes")           # (validated before the empty case returns)
    assert rows(n_rows=0, buf=None, out=None) == 0                         # nothing to read, nothing launched, nothing written
    assert rows(n_rows=0, buf=P + 8, out=P, word0=(1 << 64) - 1) == 0


def test_every_refusal_of_the_host_entry_is_a_negative_code_with_a_message():
    L = _lib.lib()
    name = b"convdr_digest_host"
    out = (ctypes.c_uint64 * 2)()
    for nb in (4, 12, 8007, -8):
        _refused(L, name, L.convdr_digest_host(P, nb, 0, out), b"n_bytes")
    _refused(L, name, L.convdr_digest_host(P, 8, 0, None), b"NULL argument")
    _refused(L, name, L.convdr_digest_host(None, 8, 0, out), b"NULL argument")
    out[0] = out[1] = 77
    assert L.convdr_digest_host(None, 0, 5, out) == 0 and (out[0], out[1]) == (0, 0)      # the empty buffer


def test_the_oracle_agrees_with_its_word_by_word_form_and_has_the_documented_properties():
    rs = np.random.RandomState(1)
    raw = rs.bytes(64)
    for word0 in (0, 7, 1 << 40, (1 << 64) - 3):
        assert C.digest(raw, word0) == C.digest_slow(raw, word0)
    assert C.digest(b"") == (0, 0)
    base = C.digest(raw)
    for bit in range(512):                                  # every single-bit flip changes both sums
        b = bytearray(raw)
        b[bit >> 3] ^= 1 << (bit & 7)
        got = C.digest(bytes(b))
        assert got[0] != base[0] and got[1] != base[1], bit
    swapped = raw[8:16] + raw[:8] + raw[16:]
    assert C.digest(swapped)[0] != base[0] and C.digest(swapped)[1] != base[1]
    z = bytes(64)
    assert C.digest(z, 0) != C.digest(z, 8) and C.digest(z) != (0, 0)          # zeros at another place, and zeros are not nothing


@pytest.mark.parametrize("nbytes", (0, 8, 24, 8008))
def test_the_host_digest_equals_the_oracle_and_is_additive(nbytes):
    raw = np.frombuffer(np.random.RandomState(nbytes).bytes(nbytes), dtype=np.uint8)
    for word0 in (0, 7, 1 << 40):
        want = C.digest(raw, word0)
        assert snapshot.digest_host(raw, word0) == want, (nbytes, word0)
        assert snapshot.digest_bytes(raw.tobytes(), word0) == want
        for cut in sorted({0, 8, 16, nbytes // 16 * 8, nbytes - 8, nbytes} & set(range(0, nbytes + 1, 8))):
            parts = C.add(snapshot.digest_host(raw[:cut], word0), snapshot.digest_host(raw[cut:], word0 + cut // 8))
            assert parts == want, (nbytes, word0, cut)
    # an unaligned host buffer is legal
    shifted = np.zeros(nbytes + 1, dtype=np.uint8)
    shifted[1:] = raw
    assert snapshot.digest_host(shifted[1:], 3) == C.digest(raw, 3)


def _producers(arrays, window_rows):
    secs = []
    for name, a in arrays.items():
        rb = a.nbytes // max(1, a.shape[0])

        def produce(fd, offset, a=a, rb=rb):
            os.pwrite(fd, a.tobytes(), offset)
            return C.window_digests(a, rb, window_rows)
        secs.append((name, a.nbytes, rb, produce))
    return secs


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """one snapshot of numpy sections written by convdr_amd.snapshot: (path, meta, arrays, its bytes)"""
    arrays = C.sample_arrays()
    meta = C.reference_meta(1300, 64, W, scale=4.0, max_norm=11.5)
    path = str(tmp_path_factory.mktemp("snap") / "index.convdr")
    size = snapshot.write_snapshot(path, dict(meta), _producers(arrays, W))
    raw = open(path, "rb").read()
    assert size == len(raw) and not os.path.exists(path + ".tmp")
    return path, meta, arrays, raw


def test_the_written_file_is_the_reference_file_and_round_trips(written):
    path, meta, arrays, raw = written
    assert raw == C.reference_bytes(meta, arrays)           # byte for byte what the documented layout says
    h, secs = C.reference_read(raw)
    assert (h["_version"], h["_zero"]) == (1, 0) and raw[C.OFF_FILL:C.HEADER_BYTES] == bytes(24)
    for name, a in arrays.items():
        assert secs[name] == a.tobytes() and h["sections"][name]["offset"] % C.SECTION_ALIGN == 0
    got = snapshot.read_header(path)
    assert got["file_bytes"] == len(raw) and {k: got[k] for k in meta} == meta
    assert got["sections"]["rows"]["digests"] == C.window_digests(arrays["rows"], 256, W) and len(got["sections"]["rows"]["digests"]) == 6
    assert got["sections"]["centre"]["digests"] == [C.digest(arrays["centre"])]
    assert snapshot.verify_file(path, threads=3)["n"] == 1300 and S.verify_snapshot(path)["n"] == 1300


def test_the_layout_constants_of_the_header_hold(written):
    _, _, _, raw = written
    assert (snapshot.MAGIC, snapshot.VERSION, snapshot.HEADER_BYTES, snapshot.SECTION_ALIGN) == (b"CONVDRIX", 1, 64, 4096)
    assert raw[:8] == b"CONVDRIX" and struct.unpack_from("<I", raw, 8)[0] == 1 and struct.unpack_from("<I", raw, 12)[0] == 0
    json_len = struct.unpack_from("<Q", raw, 16)[0]
    js = raw[64:64 + json_len]
    assert js[:1] == b"{" and js[-1:] == b"}"
    assert struct.unpack_from("<QQ", raw, 24) == C.digest(js + bytes(-len(js) % 8), 0)
    assert raw[40:64] == bytes(24)


def _with(tmp_path, raw, name="bad.convdr"):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(raw)
    return p


@pytest.mark.parametrize("section", ("rows", "ids", "centre"))
def test_a_flipped_byte_is_reported_as_its_section_and_window(written, tmp_path, section):
    path, meta, arrays, raw = written
    sec = snapshot.read_header(path)["sections"][section]
    window = 0 if section == "centre" else 2
    at = sec["offset"] + window * W * sec["row_bytes"] + (W * sec["row_bytes"] // 2 if section != "centre" else sec["bytes"] // 2)
    bad = bytearray(raw)
    bad[at] ^= 0x10
    p = _with(tmp_path, bytes(bad))
    with pytest.raises(_lib.ConvdrError, match=r"section '%s', window %d:" % (section, window)):
        snapshot.verify_file(p)
    assert snapshot.read_header(p)["n"] == 1300             # (the header itself is intact)


def test_every_refusal_of_the_reader_has_its_own_message(written, tmp_path):
    path, meta, arrays, raw = written
    json_len = struct.unpack_from("<Q", raw, 16)[0]
    cases = (
        (b"CONVDRIY" + raw[8:], "bad magic"),
        (raw[:8] + struct.pack("<I", 2) + raw[12:], "unknown version 2"),
        (raw[:70] + bytes([raw[70] ^ 1]) + raw[71:], "header digest mismatch"),
        (raw[:40], "truncated file"),
        (raw[:64 + json_len - 1], "truncated file"),
        (raw[:-1], r"truncated file: section 'centre'.*from window 0 on"),
        (raw[:snapshot.read_header(path)["sections"]["rows"]["offset"] + 3 * W * 256 + 5], r"section 'rows'.*runs past the end.*from window 3 on"),
    )
    for i, (data, msg) in enumerate(cases):
        p = _with(tmp_path, data, "bad%d.convdr" % i)
        for call in (snapshot.read_header, snapshot.verify_file, S.snapshot_info):
            with pytest.raises(_lib.ConvdrError, match=msg):
                call(p)


def test_a_failed_save_leaves_an_existing_snapshot_untouched(written, tmp_path):
    _, meta, arrays, raw = written
    p = _with(tmp_path, raw, "keep.convdr")
    with pytest.raises(OSError):
        snapshot.write_snapshot(str(tmp_path / "no_such_dir" / "x.convdr"), dict(meta), _producers(arrays, W))

    def boom(fd, offset):
        raise RuntimeError("producer failed")
    with pytest.raises(RuntimeError, match="producer failed"):
        snapshot.write_snapshot(p, dict(meta), _producers(arrays, W)[:1] + [("ids", arrays["ids"].nbytes, 8, boom)])
    assert open(p, "rb").read() == raw and not os.path.exists(p + ".tmp")


def test_an_empty_snapshot_round_trips(tmp_path):
    arrays = {"rows": np.zeros((0, 64), np.float32)}
    meta = C.reference_meta(0, 64, 65536, has_ids=False)
    p = str(tmp_path / "empty.convdr")
    snapshot.write_snapshot(p, dict(meta), [("rows", 0, 256, lambda fd, off: [])])
    assert open(p, "rb").read() == C.reference_bytes(meta, arrays)
    h = snapshot.verify_file(p)
    assert h["n"] == 0 and h["sections"]["rows"]["digests"] == [] and h["sections"]["rows"]["bytes"] == 0
