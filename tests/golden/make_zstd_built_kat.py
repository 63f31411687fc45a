"""Writes tests/golden/zstd_built_kat.json: what libzstd says about the frames that tests/zstd_build.py writes.

    python tests/golden/make_zstd_built_kat.py

Runs on the development machine only: it loads ``libzstd.so.1`` with ctypes.  The tests read the JSON and need
no libzstd.

"version": ZSTD_versionString().  "families": per family of ``zstd_build.FAMILIES`` one record per case, in the
family's order: [what, the first 16 hex digits of the frame's SHA-256, ``ZSTD_decompress``'s return value when
offered the case's output size (the size, or the error's name), the first 16 hex digits of the SHA-256 of its
output where it returned that size, else ""], and as a fifth item, where libzstd accepts a frame that the
decode contract (top of dwarfs_amd/csrc/zstd_host.cpp) refuses, the RFC 8878 section that states the rule.  No
frame bytes are stored: the builder is deterministic.  Any other disagreement between libzstd, the builder's
record and tests/zstd_ref.py stops the generator; it also asserts that the frames libzstd judges differently
stay below 5 % of the records, and that the accepted frames reach every feature of ``zstd_ref.FEATURES``.
"""
import ctypes as C
import hashlib
import json
import sys
from collections import Counter
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import make_zstd_kat as K  # noqa: E402

# the reader's refusals of frames that libzstd 1.4.8 accepts: the kat's, and the window rules the contract claims
STRICTER = dict(K.STRICTER, **{
    "offset before the start of the output or beyond the window": "3.1.1.1.2",
    "block above the block maximum": "3.1.1.2.3",
    "block above the block maximum or the content size": "3.1.1.2.3",
})


def digest(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()[:16]


def libzstd():
    """libzstd.so.1 with the two functions' types set, or None where it does not load."""
    try:
        L = C.CDLL("libzstd.so.1")
    except OSError:
        return None
    L.ZSTD_versionString.restype = C.c_char_p
    L.ZSTD_getErrorName.restype = C.c_char_p
    L.ZSTD_getErrorName.argtypes = [C.c_size_t]
    L.ZSTD_isError.argtypes = [C.c_size_t]
    L.ZSTD_decompress.restype = C.c_size_t
    L.ZSTD_decompress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    return L


def verdict(L, frame: bytes, n: int):
    """(the size ZSTD_decompress returned or its error's name, its output)"""
    buf = C.create_string_buffer(max(n, 1))
    r = L.ZSTD_decompress(buf, n, frame, len(frame))
    if L.ZSTD_isError(r):
        return L.ZSTD_getErrorName(r).decode(), b""
    return int(r), buf.raw[:r]


def main():
    import zstd_build as B
    import zstd_ref as R

    L = libzstd()
    families, total, stricter, coverage = {}, 0, 0, Counter()
    for family, make in B.FAMILIES.items():
        recs = []
        for c in make():
            ret, out = verdict(L, c.frame, c.out_n)
            rec = [c.what, digest(c.frame), ret, digest(out) if ret == c.out_n else ""]
            stats = Counter()
            try:
                ours = R.decode(c.frame, stats, size=c.out_n)
            except R.ZstdError as e:
                assert not c.ok, (c.what, str(e))
                if ret == c.out_n:
                    rec.append(STRICTER[str(e)])  # (a KeyError here is a disagreement that needs looking at)
                    stricter += 1
            else:
                assert c.ok and ret == c.out_n and ours == out == c.want, (c.what, ret)
                coverage += stats
            recs.append(rec)
        families[family] = recs
        total += len(recs)
    assert 20 * stricter <= total, (stricter, total)
    assert all(coverage[k] for k in R.FEATURES), [k for k in R.FEATURES if not coverage[k]]
    body = ",\n".join('%s:[\n%s\n]' % (json.dumps(f), ",\n".join(json.dumps(r, separators=(",", ":")) for r in recs))
                      for f, recs in families.items())
    (HERE / "zstd_built_kat.json").write_text('{"version":%s,\n"families":{\n%s\n}}\n'
                                              % (json.dumps(L.ZSTD_versionString().decode()), body))
    print(f"{total} frames ({stricter} stricter), libzstd {L.ZSTD_versionString().decode()}")


if __name__ == "__main__":
    main()
