#!/usr/bin/env python3
"""tools/code_objects.py LIB [LIB2] -- the device code of a build (no GPU).

libpifft.so carries one offload bundle per translation unit, stored
zstd-compressed (--offload-compress: a "CCOB" header -- magic, version 3,
method 1 = zstd, total size, inflated size, hash -- then the frame).  This
inflates each (libzstd through ctypes) and prints its SHA-256; with two
libraries it compares bundle by bundle and exits 1 unless every one is
byte-identical: what a host-only change must show (the k_pass parts and
csrc/pifft.hip's own kernels -- tree, interleave, real fix-ups, generator).

  python tools/code_objects.py cs87project-msolano2_amd/libpifft.so other/libpifft.so
"""
import ctypes
import ctypes.util
import hashlib
import re
import struct
import sys


def bundles(path: str) -> list:
    """The inflated offload bundles of a library, in file order."""
    z = ctypes.CDLL(ctypes.util.find_library("zstd") or "libzstd.so.1")
    z.ZSTD_decompress.restype = ctypes.c_size_t
    z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    data = open(path, "rb").read()
    out = []
    for m in re.finditer(rb"CCOB\x03\x00\x01\x00", data):
        total, size, _ = struct.unpack_from("<QQQ", data, m.start() + 8)
        frame = data[m.start() + 32:m.start() + total]
        buf = ctypes.create_string_buffer(size)
        got = z.ZSTD_decompress(buf, size, frame, len(frame))
        if got != size:
            raise RuntimeError(f"{path}: bundle at {m.start()} inflates to {got} bytes, header says {size}")
        out.append(buf.raw)
    if not out:
        raise RuntimeError(f"{path}: no compressed offload bundle (CCOB version 3, zstd) found")
    return out


def main() -> int:
    if len(sys.argv) not in (2, 3):
        sys.stderr.write(__doc__)
        return 2
    a = bundles(sys.argv[1])
    if len(sys.argv) == 2:
        for k, raw in enumerate(a):
            print(f"{k:3d} {len(raw):9d} {hashlib.sha256(raw).hexdigest()}")
        return 0
    b = bundles(sys.argv[2])
    same = len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        ok = x == y
        same = same and ok
        print(f"{k:3d} {len(x):9d} {hashlib.sha256(x).hexdigest()[:16]} {'same' if ok else 'DIFFERENT ' + hashlib.sha256(y).hexdigest()[:16]}")
    print(f"{len(a)} and {len(b)} code-object bundles: {'identical' if same else 'NOT identical'}")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
