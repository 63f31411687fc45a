"""Writes tests/golden/similarity_kat.json: known answers for the two similarity hashes of the inode scan.

    python tests/golden/make_similarity_kat.py

Pure Python, host only.  Both hashes are restated here from their description (include/ricepp_amd.h, the
similarity group); this model is the third restatement next to the host C++ and the HIP kernels.

"nilsimsa_reference": the reference's recorded answers (test/nilsimsa_test.cpp: the empty string, "abcdefgh",
    the incremental pair and the 26 prefixes of the alphabet), as the reference prints them (`hexdigest`: the 32
    digest bytes reversed).  `build` asserts that the model reproduces every one of them.
"messages": synthetic messages (kind, seed, length) with the model's nilsimsa hexdigest and 32-bit similarity
    value (8 hex digits).  The reference records no vector for the 32-bit hash: these come from the model alone.
"table": the first four and last two entries of the transition table.
"""
import json
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent

ZERO = "00" * 32
ABCDEFGH = "14c8118000000000030800000004042004189020001308014088003280000078"
ABCDEFGHIJK = "14c811840010000c0328200108040630041890200217582d4098103280000078"
ALPHABET = "abcdefghijklmnopqrstuvwxyz"
ALPHABET_PREFIXES = [
    ZERO,
    ZERO,
    "0040000000000000000000000000000000000000000000000000000000000000",
    "0440000000000000000000000000000000100000000000000008000000000000",
    "0440008000000000000000000000000000100020001200000008001200000050",
    "04c0018000000000000000000000000004188020001200000088001280000058",
    "04c8118000000000030000000000002004188020001208004088001280000078",
    "14c8118000000000030800000004042004189020001308014088003280000078",
    "14c8118400000000030800010804043004189020021318094098003280000078",
    "14c81184000000000308200108040430041890200217580d4098103280000078",
    "14c811840010000c0328200108040630041890200217582d4098103280000078",
    "14c811840010000ca328200108044630041890200a17586d4298103280000078",
    "14ca11850010000ca328200188044630041898200a17586dc2d8103284000078",
    "14ca11850030004ca3a8200188044630041898200a17586dc2d8107284000078",
    "14ca11850032004ca3a8284188044730041898200a17586dc2d8107384000078",
    "94ca11850432005ca3a828418804473004199c200a17586dc2d8107384004178",
    "94ca11850433005ca3a82841880447341419be200a17586dc2d8107384004178",
    "94ca11850433005ca3a82841a88457341419be201a17586dc6d8107384084178",
    "94ca11850533005ca3b82841a88657361419be201a17586dc6d8107384084178",
    "94ca11850533005ca3b82841aa8657371419be201a17587dc6d81077840c4178",
    "94ca15850533005ca3b92841aa8657371419be201a17587dd6d81077844cc178",
    "94ca15850533005ca3b92849aa8657371419be201a17587fd6d81077844cc978",
    "94ca15850533045cabb92869aa8657371419bea01a17587fd6f81077c44cc978",
    "94ca95850533045cabb93869aa8657371499beb01a17587fd6f8107fc44cc978",
    "94ca95850733045cabb93869aa8657373499beb01a17587fd6f9107fc54cc978",
    "94ca95850773045cabb93869ba8657373499beb81a17587fd6f9107fc54cc978",
]
INCREMENTAL = [{"pieces": ["a", "bc", "defgh"], "hexdigest": ABCDEFGH},
               {"pieces": ["i", "jk"], "hexdigest": ABCDEFGHIJK}]

LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 70001]
OTHER_KIND_LENGTHS = [5, 17, 64, 257, 4097, 70001]
TEXT = b"The quick brown fox jumps over the lazy dog; pack my box with five dozen liquor jugs.\n"


def transition_table():
    """The published Nilsimsa table: a recurrence with multiplier 53 whose values are bumped past those
    already taken (the search restarts after every bump)."""
    t, j = [], 0
    for _ in range(256):
        j = (53 * j + 1) & 255
        j += j
        if j > 255:
            j -= 255
        while j in t:
            j = (j + 1) & 255
        t.append(j)
    return t


T = transition_table()
# tran3(a, b, c, n) = (A[n][a] ^ B[n][b]) + C[n][c], truncated to 8 bits
_A = [[T[(a + n) & 255] for a in range(256)] for n in range(8)]
_B = [[T[b] * (2 * n + 1) for b in range(256)] for n in range(8)]
_C = [[T[c ^ T[n]] for c in range(256)] for n in range(8)]


def tran3(a, b, c, n):
    return ((_A[n][a] ^ _B[n][b]) + _C[n][c]) & 255


class Nilsimsa:
    def __init__(self):
        self.acc = [0] * 256
        self.size = 0
        self.w = [0, 0, 0, 0]  # the four bytes before the next one, latest first

    def update(self, data: bytes):
        acc, (w1, w2, w3, w4), p = self.acc, self.w, self.size
        for w0 in data:
            if p >= 2:
                acc[tran3(w0, w1, w2, 0)] += 1
            if p >= 3:
                acc[tran3(w0, w1, w3, 1)] += 1
                acc[tran3(w0, w2, w3, 2)] += 1
            if p >= 4:
                acc[tran3(w0, w1, w4, 3)] += 1
                acc[tran3(w0, w2, w4, 4)] += 1
                acc[tran3(w0, w3, w4, 5)] += 1
                acc[tran3(w4, w1, w0, 6)] += 1
                acc[tran3(w4, w3, w0, 7)] += 1
            w1, w2, w3, w4 = w0, w1, w2, w3
            p += 1
        self.w, self.size = [w1, w2, w3, w4], p
        return self

    def total(self):
        n = self.size
        return 0 if n < 3 else 1 if n == 3 else 4 if n == 4 else 8 * n - 28

    def digest(self) -> bytes:
        threshold = self.total() // 256
        out = bytearray(32)
        for i, c in enumerate(self.acc):
            if c > threshold:
                out[i >> 3] |= 1 << (i & 7)
        return bytes(out)

    def hexdigest(self) -> str:
        return self.digest()[::-1].hex()


def mix32(x):
    x ^= x >> 16
    x = (x * 0x21F0AAAD) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x735A2D97) & 0xFFFFFFFF
    x ^= x >> 15
    return x


class Similarity:
    def __init__(self):
        self.acc = [0] * 256
        self.val = 0
        self.size = 0

    def update(self, data: bytes):
        acc, val, p = self.acc, self.val, self.size
        for b in data:
            val = ((val << 8) | b) & 0xFFFFFFFF
            if p >= 3:
                i = mix32((val + 0x9E3779B9) & 0xFFFFFFFF) >> 24
                acc[i] = (acc[i] + 1) & 0xFFFFFFFF
            p += 1
        self.val, self.size = val, p
        return self

    def value(self) -> int:
        top = sorted(range(256), key=lambda i: (-self.acc[i], i))[:4]
        return top[0] << 24 | top[1] << 16 | top[2] << 8 | top[3]

    def digest(self) -> bytes:
        return self.value().to_bytes(4, "little")

    def hexdigest(self) -> str:
        return f"{self.value():08x}"


def message_specs():
    specs = [{"kind": "rng", "seed": 7000 + i, "length": n} for i, n in enumerate(LENGTHS)]
    for kind in ("zero", "period2", "text"):
        specs += [{"kind": kind, "seed": 0, "length": n} for n in OTHER_KIND_LENGTHS]
    return specs


def message_bytes(spec) -> bytes:
    n, kind = spec["length"], spec["kind"]
    if kind == "zero":
        return bytes(n)
    if kind == "period2":
        return (b"\xa5\x3c" * (n // 2 + 1))[:n]
    if kind == "text":
        return (TEXT * (n // len(TEXT) + 1))[:n]
    return np.random.default_rng(spec["seed"]).integers(0, 256, n, dtype=np.uint8).tobytes()


def build():
    assert sorted(T) == list(range(256)) and T[:4] == [0x02, 0xD6, 0x9E, 0x6F] and T[-2:] == [0x72, 0x4E]

    def nil(b):
        return Nilsimsa().update(b).hexdigest()

    assert nil(b"") == ZERO and nil(b"abcdefgh") == ABCDEFGH
    for i, want in enumerate(ALPHABET_PREFIXES):
        assert nil(ALPHABET[:i + 1].encode()) == want, i
    h = Nilsimsa()
    for step in INCREMENTAL:
        for piece in step["pieces"]:
            h.update(piece.encode())
        assert h.hexdigest() == step["hexdigest"]
    assert Similarity().value() == 0x00010203
    messages = []
    for spec in message_specs():
        m = message_bytes(spec)
        messages.append(dict(spec, nilsimsa=nil(m), similarity=Similarity().update(m).hexdigest()))
    return {
        "table": {"head": T[:4], "tail": T[-2:]},
        "nilsimsa_reference": {"empty": ZERO, "abcdefgh": ABCDEFGH, "incremental": INCREMENTAL,
                               "alphabet": ALPHABET, "alphabet_prefixes": ALPHABET_PREFIXES},
        "messages": messages,
    }


def main():
    kat = build()
    (HERE / "similarity_kat.json").write_text(json.dumps(kat, indent=0, separators=(",", ":")) + "\n")
    print(f"{len(kat['messages'])} messages")


if __name__ == "__main__":
    main()
