"""Writes tests/golden/zstd_enc_adaptive_kat.json: what libzstd says about the frames that this project's
Zstandard encoder writes with its options word (1: per-block table modes, 2: repeat offsets, 3: both).

    python tests/golden/make_zstd_enc_adaptive_kat.py

Runs on the development machine only: it loads ``libzstd.so.1`` with ctypes (there are no headers) and needs the
built library.  The tests read the JSON and need neither.

"version": ZSTD_versionString().  "cases": per input of tests/zstd_enc_adaptive_cases.py its name, size and
SHA-256, the size of the options-0 frame ("size0"), and under "1", "2" and "3" the size and SHA-256 of
``rpp_zstd_host_encode_opt``'s frame and what ``ZSTD_decompress`` returned for it ("decompressed": the input's
size, and the bytes were compared with the input here).  "totals": per options word the frames' sizes added up,
over all inputs and ("base") over the inputs of tests/zstd_enc_cases.py alone.  "grew": per options word how many
inputs came out larger than with options 0, and the largest growth in bytes.  Totals and growth are recorded,
not asserted.
"""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))


def main():
    import zstd_enc_adaptive_cases as AC
    from dwarfs_amd import zstd

    Z = C.CDLL("libzstd.so.1")
    Z.ZSTD_versionString.restype = C.c_char_p
    Z.ZSTD_decompress.restype = C.c_size_t
    Z.ZSTD_decompress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    Z.ZSTD_isError.argtypes = [C.c_size_t]
    base = len(AC.EC.inputs())
    options = (0,) + AC.OPTIONS
    cases = []
    totals = {str(o): {"all": 0, "base": 0} for o in options}
    grew = {str(o): {"inputs": 0, "largest": 0} for o in AC.OPTIONS}
    for i, (name, data) in enumerate(AC.inputs()):
        size0 = len(zstd.host_encode(data)[0])
        rec = {"name": name, "size": len(data), "sha256": hashlib.sha256(data).hexdigest(), "size0": size0}
        for o in options:
            frame, _ = zstd.host_encode(data, o)
            totals[str(o)]["all"] += len(frame)
            if i < base:
                totals[str(o)]["base"] += len(frame)
            if o == 0:
                continue
            buf = C.create_string_buffer(max(len(data), 1))
            r = Z.ZSTD_decompress(buf, len(data), frame, len(frame))
            assert not Z.ZSTD_isError(r) and r == len(data) and buf.raw[:len(data)] == data, (name, o)
            rec[str(o)] = {"frame_size": len(frame), "frame_sha256": hashlib.sha256(frame).hexdigest(),
                           "decompressed": int(r)}
            if len(frame) > size0:
                grew[str(o)]["inputs"] += 1
                grew[str(o)]["largest"] = max(grew[str(o)]["largest"], len(frame) - size0)
        cases.append(rec)
    lines = ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases)
    (HERE / "zstd_enc_adaptive_kat.json").write_text(
        '{"version":%s,\n"totals":%s,\n"grew":%s,\n"cases":[\n%s\n]}\n' %
        (json.dumps(Z.ZSTD_versionString().decode()), json.dumps(totals, separators=(",", ":")),
         json.dumps(grew, separators=(",", ":")), lines))
    print(f"{len(cases)} cases, libzstd {Z.ZSTD_versionString().decode()}, totals {totals}, grew {grew}")


if __name__ == "__main__":
    main()
