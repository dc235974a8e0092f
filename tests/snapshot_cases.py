"""The numpy oracle of the snapshot digest (csrc/ip_digest.hpp; include/convdr_hip.h, "Digest and snapshot file") and a reference
writer and reader of the snapshot file format on numpy arrays.  Restated from the documented definition and layout, not from
convdr_amd/snapshot.py: the tests hold the two against each other."""
import json
import struct

import numpy as np

K1, K2 = 0x9e3779b97f4a7c15, 0xd6e8feb86659fd93
M64 = (1 << 64) - 1
# the layout constants include/convdr_hip.h documents
MAGIC, VERSION, HEADER_BYTES, SECTION_ALIGN = b"CONVDRIX", 1, 64, 4096
OFF_VERSION, OFF_ZERO, OFF_JSON_LEN, OFF_A, OFF_B, OFF_FILL = 8, 12, 16, 24, 32, 40


def _u(x):
    return np.uint64(x & M64)


def mix(x):
    """the splitmix64 finaliser on a uint64 array"""
    x = x ^ (x >> _u(30))
    x = x * _u(0xbf58476d1ce4e5b9)
    x = x ^ (x >> _u(27))
    x = x * _u(0x94d049bb133111eb)
    return x ^ (x >> _u(31))


def digest(buf, word0=0):
    """(A, B) of a buffer of a multiple of 8 bytes (bytes or any numpy array), its first word at index word0"""
    w = np.frombuffer(np.ascontiguousarray(buf).tobytes() if isinstance(buf, np.ndarray) else bytes(buf), dtype="<u8").astype(np.uint64)
    if not w.size:
        return 0, 0
    g = np.arange(1, w.size + 1, dtype=np.uint64) + _u(word0)
    a = mix(w ^ (g * _u(K1))).sum(dtype=np.uint64)
    b = mix(((w << _u(29)) | (w >> _u(35))) ^ (g * _u(K2))).sum(dtype=np.uint64)
    return int(a), int(b)


def digest_slow(buf, word0=0):
    """the same with Python integers, word by word (the oracle's own check)"""
    def m(x):
        x ^= x >> 30
        x = x * 0xbf58476d1ce4e5b9 & M64
        x ^= x >> 27
        x = x * 0x94d049bb133111eb & M64
        return x ^ (x >> 31)
    raw = bytes(buf)
    a = b = 0
    for i in range(len(raw) // 8):
        w = int.from_bytes(raw[8 * i:8 * i + 8], "little")
        g = (word0 + i + 1) & M64
        a = (a + m(w ^ (g * K1 & M64))) & M64
        b = (b + m((((w << 29) | (w >> 35)) & M64) ^ (g * K2 & M64))) & M64
    return a, b


def add(x, y):
    return (x[0] + y[0]) & M64, (x[1] + y[1]) & M64


def window_digests(arr, row_bytes, window_rows, word0=0):
    """per-window digests of a buffer of rows, window j at word0 + j * window_rows * row_bytes / 8"""
    raw = np.ascontiguousarray(arr).tobytes()
    step = window_rows * row_bytes
    return [digest(raw[a:a + step], word0 + a // 8) for a in range(0, len(raw), step)]


def f32_bits(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(x)))[0]


def reference_meta(n, d_in, window_rows, storage="fp32", precision="auto", center=True, scale=1.0, max_norm=0.0, has_ids=True):
    return {"d_in": d_in, "d": (d_in + 63) // 64 * 64, "storage": storage, "precision": precision, "center": center, "n": n,
            "scale": f32_bits(scale), "max_norm": f32_bits(max_norm), "x3_first": False, "has_ids": has_ids, "window_rows": window_rows}


def reference_bytes(meta, arrays):
    """The whole file as bytes.  arrays: {name: numpy array [rows, ...]} in file order ("rows", "ids", "centre"; the centre is
    ONE row)."""
    w = meta["window_rows"]
    table = {}
    for name, a in arrays.items():
        rb = a.nbytes if name == "centre" else (a.nbytes // a.shape[0] if a.shape[0] else int(np.prod(a.shape[1:], dtype=np.int64)) * a.itemsize)
        table[name] = {"offset": 0, "bytes": a.nbytes, "row_bytes": rb,
                       "digests": [["%016x" % x, "%016x" % y] for x, y in window_digests(a, rb, w)]}
    for _ in range(8):         # offsets depend on the JSON's length, which depends on their digits
        js = json.dumps(dict(meta, sections=table), sort_keys=True).encode()
        at = HEADER_BYTES + len(js)
        for name, a in arrays.items():
            at = -(-at // SECTION_ALIGN) * SECTION_ALIGN
            table[name]["offset"] = at
            at += a.nbytes
    js = json.dumps(dict(meta, sections=table), sort_keys=True).encode()
    out = bytearray(at if arrays else HEADER_BYTES + len(js))
    a_, b_ = digest(js + b"\0" * (-len(js) % 8))
    out[:HEADER_BYTES] = MAGIC + struct.pack("<IIQQQ", VERSION, 0, len(js), a_, b_) + b"\0" * (HEADER_BYTES - OFF_FILL)
    out[HEADER_BYTES:HEADER_BYTES + len(js)] = js
    for name, a in arrays.items():
        out[table[name]["offset"]:table[name]["offset"] + a.nbytes] = np.ascontiguousarray(a).tobytes()
    return bytes(out)


def reference_read(raw):
    """(header dict, {name: bytes}) of a file's bytes, by the documented layout; no check beyond the magic"""
    assert raw[:8] == MAGIC
    version, zero, json_len = struct.unpack_from("<IIQ", raw, OFF_VERSION)
    h = json.loads(raw[HEADER_BYTES:HEADER_BYTES + json_len].decode())
    h["_version"], h["_zero"], h["_json_digest"] = version, zero, struct.unpack_from("<QQ", raw, OFF_A)
    return h, {name: raw[s["offset"]:s["offset"] + s["bytes"]] for name, s in h["sections"].items()}


def sample_arrays(n=1300, d=64, seed=0, ids=True, centre=True):
    rs = np.random.RandomState(seed)
    arrays = {"rows": rs.randn(n, d).astype(np.float32)}
    if ids:
        arrays["ids"] = rs.randint(-2 ** 62, 2 ** 62, size=n).astype(np.int64)
    if centre:
        arrays["centre"] = rs.randn(1, d).astype(np.float32)
    return arrays
