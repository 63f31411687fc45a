"""Writes tests/golden/digest_kat.json and digest_kat.bin: the yardstick of the named digests (rpp_digest_batch,
rpp_digest_host), from Python's hashlib, which shares no code with the library.

Messages are not stored.  Message i of ``specs()`` is ``random.Random(SEED + i).randbytes(length)`` (the Mersenne
Twister of the standard library); the tests regenerate it.  digest_kat.bin holds, algorithm after algorithm in the
order of ``ALGORITHMS``, the digests of all messages back to back (raw bytes); the JSON holds the layout, the message
lengths with the payload misalignment each one is meant to be placed at, and the published vectors of each standard
for "abc" and the empty message (RFC 1321, FIPS 180-4 and FIPS 202 example values, RFC 7693), which this script checks
hashlib against before it trusts it.

Run from the repository root:  python tests/golden/make_digest_kat.py
"""

import hashlib
import json
import random
from pathlib import Path

HERE = Path(__file__).resolve().parent
SEED = 20261

# canonical name -> (hashlib name, digest bytes)
ALGORITHMS = {
    "md5": ("md5", 16), "sha1": ("sha1", 20), "sha224": ("sha224", 28), "sha256": ("sha256", 32),
    "sha384": ("sha384", 48), "sha512": ("sha512", 64), "sha512-224": ("sha512_224", 28),
    "sha3-224": ("sha3_224", 28), "sha3-256": ("sha3_256", 32), "sha3-384": ("sha3_384", 48),
    "sha3-512": ("sha3_512", 64), "blake2b512": ("blake2b", 64), "blake2s256": ("blake2s", 32),
}

PUBLISHED = {
    "md5": ("900150983cd24fb0d6963f7d28e17f72", "d41d8cd98f00b204e9800998ecf8427e"),
    "sha1": ("a9993e364706816aba3e25717850c26c9cd0d89d", "da39a3ee5e6b4b0d3255bfef95601890afd80709"),
    "sha224": ("23097d223405d8228642a477bda255b32aadbce4bda0b3f7e36c9da7",
               "d14a028c2a3a2bc9476102bb288234c415a2b01f828ea62ac5b3e42f"),
    "sha256": ("ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad",
               "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"),
    "sha384": ("cb00753f45a35e8bb5a03d699ac65007272c32ab0eded1631a8b605a43ff5bed8086072ba1e7cc2358baeca134c825a7",
               "38b060a751ac96384cd9327eb1b1e36a21fdb71114be07434c0cc7bf63f6e1da274edebfe76f65fbd51ad2f14898b95b"),
    "sha512": ("ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a"
               "2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f",
               "cf83e1357eefb8bdf1542850d66d8007d620e4050b5715dc83f4a921d36ce9ce"
               "47d0d13c5d85f2b0ff8318d2877eec2f63b931bd47417a81a538327af927da3e"),
    "sha512-224": ("4634270f707b6a54daae7530460842e20e37ed265ceee9a43e8924aa",
                   "6ed0dd02806fa89e25de060c19d3ac86cabb87d6a0ddd05c333b84f4"),
    "sha3-224": ("e642824c3f8cf24ad09234ee7d3c766fc9a3a5168d0c94ad73b46fdf",
                 "6b4e03423667dbb73b6e15454f0eb1abd4597f9a1b078e3f5b5a6bc7"),
    "sha3-256": ("3a985da74fe225b2045c172d6bd390bd855f086e3e9d525b46bfe24511431532",
                 "a7ffc6f8bf1ed76651c14756a061d662f580ff4de43b49fa82d80a4b80f8434a"),
    "sha3-384": ("ec01498288516fc926459f58e2c6ad8df9b473cb0fc08c2596da7cf0e49be4b298d88cea927ac7f539f1edf228376d25",
                 "0c63a75b845e4f7d01107d852e4c2485c51a50aaaa94fc61995e71bbee983a2ac3713831264adb47fb6bd1e058d5f004"),
    "sha3-512": ("b751850b1a57168a5693cd924b6b096e08f621827444f70d884f5d0240d2712e"
                 "10e116e9192af3c91a7ec57647e3934057340b4cf408d5a56592f8274eec53f0",
                 "a69f73cca23a9ac5c8b567dc185a756e97c982164fe25859e0d1dcc1475c80a6"
                 "15b2123af1f5f94c11e3e9402c3ac558f500199d95b6d3e301758586281dcd26"),
    "blake2b512": ("ba80a53f981c4d0d6a2797b69f12f6e94c212f14685ac4b74b12bb6fdbffa2d1"
                   "7d87c5392aab792dc252d5de4533cc9518d38aa8dbf1925ab92386edd4009923",
                   "786a02f742015903c6c6fd852552d272912f4740e15847618a86e217f71f5419"
                   "d25e1031afee585313896444934eb04b903a685b1448b755d56f701afe9be2ce"),
    "blake2s256": ("508c5e8c327c14e2e1a72ba34eeb452f37458b209ed63a294d999b4c86675982",
                   "69217a3079908094e11121d042354a7c1f55b6482ca1a51e1b250dfd1ed0eef9"),
}

SWEEP = list(range(301)) + [4095, 4096, 4097, 65536 + 3]
# Where a kernel can go wrong: the padding spilling into one more block (55/56, 63/64; 111/112, 127/128), the SHA-3
# rates 72, 104, 136, 144 at rate - 1 (0x06 and 0x80 in one byte), rate, rate + 1 and two rates, and whole BLAKE2
# blocks (64, 128, 256: the last full block is the final one).  Each at every payload misalignment 0..15.
BOUNDARY = [0, 1, 55, 56, 63, 64, 65, 71, 72, 73, 103, 104, 105, 111, 112, 119, 120, 127, 128, 129, 135, 136, 137, 143,
            144, 145, 208, 256, 272, 288, 4096]


def specs():
    """[(length, misalign)]: the sweep on 16-byte boundaries, then every boundary length at every misalignment."""
    return [(n, 0) for n in SWEEP] + [(n, mis) for n in BOUNDARY for mis in range(16)]


def message_bytes(i: int, length: int) -> bytes:
    return random.Random(SEED + i).randbytes(length)


def build():
    """(json object, bin bytes)"""
    for name, (hname, nbytes) in ALGORITHMS.items():
        abc, empty = PUBLISHED[name]
        assert hashlib.new(hname, b"abc").hexdigest() == abc, name
        assert hashlib.new(hname, b"").hexdigest() == empty, name
        assert len(abc) == 2 * nbytes
    sp = specs()
    msgs = [message_bytes(i, n) for i, (n, _) in enumerate(sp)]
    blob = b"".join(hashlib.new(hname, m).digest() for hname, _ in ALGORITHMS.values() for m in msgs)
    obj = {
        "prng": "random.Random(seed + i).randbytes(length), Python standard library (MT19937)",
        "seed": SEED,
        "algorithms": [{"name": n, "bytes": b} for n, (_, b) in ALGORITHMS.items()],
        "messages": [[n, mis] for n, mis in sp],
        "bin": "digest_kat.bin: per algorithm in this order, the digests of all messages back to back",
        "bin_bytes": len(blob),
        "bin_sha256": hashlib.sha256(blob).hexdigest(),
        "published": {n: {"abc": PUBLISHED[n][0], "empty": PUBLISHED[n][1]} for n in ALGORITHMS},
    }
    return obj, blob


if __name__ == "__main__":
    obj, blob = build()
    (HERE / "digest_kat.json").write_text(json.dumps(obj, indent=1) + "\n")
    (HERE / "digest_kat.bin").write_bytes(blob)
    print(f"{len(obj['messages'])} messages, {len(blob)} digest bytes")
