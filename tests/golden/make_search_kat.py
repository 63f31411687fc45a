"""Writes tests/golden/search_kat.json: what liblz4 and libzstd say about the blocks and frames that this
project's encoders write under each search word (depth | 0x100 for LAZY; 0 is the one-candidate search).

    python tests/golden/make_search_kat.py

Runs on the development machine only: it loads ``liblz4.so.1`` and ``libzstd.so.1`` with ctypes (there are no
headers) and needs the built library.  The tests read the JSON and need neither.

"versions": LZ4_versionString() and ZSTD_versionString().  "words": the search words in the order of every list
below (0, then the eight words).  "cases": per input of tests/search_cases.py its name and size, for comparison the
sizes of LZ4_compress_HC at level 9 and of ZSTD_compress at levels 1 and 3 ("libs", in that order), and per format
-- ``rpp_lz4_host_encode_search``'s block ("lz4"), ``rpp_zstd_host_encode_search``'s frame under options 0 and 3
("zstd0", "zstd3") -- the sizes under each word ("sizes"), ONE SHA-256 over the nine results one behind the other
("sha256": the file stays small, and a byte that moves under any word moves it), and what the library's decoder
returned for every one of those nine ("decoded": the input's size; each result was decoded and compared with the
input here, and anything else stops this script).  "totals": per search word and format the sizes added up
over all inputs ("all"), over the inputs of the existing lists ("base") and over the constructed ones
("constructed"), and the libraries' own totals under "hc9", "zstd1" and "zstd3".  "grew": per search word and
format how many inputs came out larger than under search 0, and the largest growth in bytes.  Totals and growth
are recorded; tests/test_search_host.py asserts one condition on the constructed totals.
"""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))

FORMATS = ("lz4", "zstd0", "zstd3")


def main():
    import search_cases as SC
    from dwarfs_amd import lz4, zstd

    L, Z = C.CDLL("liblz4.so.1"), C.CDLL("libzstd.so.1")
    L.LZ4_versionString.restype = C.c_char_p
    L.LZ4_compressBound.argtypes = [C.c_int]
    L.LZ4_compress_HC.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    Z.ZSTD_versionString.restype = C.c_char_p
    Z.ZSTD_compressBound.restype = C.c_size_t
    Z.ZSTD_compressBound.argtypes = [C.c_size_t]
    Z.ZSTD_compress.restype = C.c_size_t
    Z.ZSTD_compress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int]
    Z.ZSTD_decompress.restype = C.c_size_t
    Z.ZSTD_decompress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    Z.ZSTD_isError.argtypes = [C.c_size_t]

    def hc9(data):
        cap = L.LZ4_compressBound(len(data))
        buf = C.create_string_buffer(max(cap, 1))
        return int(L.LZ4_compress_HC(data, buf, len(data), cap, 9))

    def zstd_level(data, level):
        cap = Z.ZSTD_compressBound(len(data))
        buf = C.create_string_buffer(cap)
        r = Z.ZSTD_compress(buf, cap, data, len(data), level)
        assert not Z.ZSTD_isError(r)
        return int(r)

    def verdict(fmt, data, enc):
        buf = C.create_string_buffer(max(len(data), 1))
        if fmt == "lz4":
            r = L.LZ4_decompress_safe(enc, buf, len(enc), len(data))
        else:
            r = Z.ZSTD_decompress(buf, len(data), enc, len(enc))
            assert not Z.ZSTD_isError(r)
        assert r == len(data) and buf.raw[:len(data)] == data, fmt
        return int(r)

    words = (0,) + SC.WORDS
    base = len(SC.AC.inputs())
    groups = ("all", "base", "constructed")
    totals = {str(w): {f: dict.fromkeys(groups, 0) for f in FORMATS} for w in words}
    for lib in ("hc9", "zstd1", "zstd3"):
        totals[lib] = dict.fromkeys(groups, 0)
    grew = {str(w): {f: {"inputs": 0, "largest": 0} for f in FORMATS} for w in SC.WORDS}
    cases = []
    for i, (name, data) in enumerate(SC.inputs()):
        group = "base" if i < base else "constructed"
        libs = [hc9(data), zstd_level(data, 1), zstd_level(data, 3)]
        rec = {"name": name, "size": len(data), "libs": libs}
        for lib, size in zip(("hc9", "zstd1", "zstd3"), libs):
            totals[lib]["all"] += size
            totals[lib][group] += size
        for f in FORMATS:
            encoded = [lz4.host_encode(data, w)[0] if f == "lz4" else zstd.host_encode(data, int(f[4:]), w)[0]
                       for w in words]
            decoded = {verdict(f, data, enc) for enc in encoded}
            assert decoded == {len(data)}
            rec[f] = {"sizes": [len(enc) for enc in encoded], "sha256": hashlib.sha256(b"".join(encoded)).hexdigest(),
                      "decoded": len(data)}
            for w, enc in zip(words, encoded):
                totals[str(w)][f]["all"] += len(enc)
                totals[str(w)][f][group] += len(enc)
                if w and len(enc) > len(encoded[0]):
                    grew[str(w)][f]["inputs"] += 1
                    grew[str(w)][f]["largest"] = max(grew[str(w)][f]["largest"], len(enc) - len(encoded[0]))
        cases.append(rec)
    versions = {"lz4": L.LZ4_versionString().decode(), "zstd": Z.ZSTD_versionString().decode()}
    lines = ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases)
    (HERE / "search_kat.json").write_text(
        '{"versions":%s,\n"words":%s,\n"totals":%s,\n"grew":%s,\n"cases":[\n%s\n]}\n' %
        (json.dumps(versions, separators=(",", ":")), json.dumps(list(words)), json.dumps(totals, separators=(",", ":")),
         json.dumps(grew, separators=(",", ":")), lines))
    print(f"{len(cases)} cases, {versions}")
    for key, t in totals.items():
        print(key, t)
    print("grew", grew)


if __name__ == "__main__":
    main()
