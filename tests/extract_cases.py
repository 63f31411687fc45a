"""Shared inputs of the file-extraction tests (plain Python; no GPU, no native code).

A case is decoded blocks, files as chunk lists, and optionally rows that are overwritten after the destinations have
been laid out (so a chunk can claim more bytes than its place has).  Blocks are pseudo-random bytes from fixed seeds,
so a misplaced byte shows; their sizes are no multiples of 16 and they lie back to back in the buffer, so a block's
start has any phase.  A chunk is the tuple (block, offset, size); a hole is (HOLE, 0, size).  ``model`` is the
plain-Python restatement of the rules that the host call is tested against.
"""

import random
from typing import List, NamedTuple, Optional, Tuple

HOLE = 0xFFFFFFFF
BAD_CHUNK = -9
ALIGN_SIZES = (0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 48)


class Case(NamedTuple):
    name: str
    blocks: List[bytes]
    files: List[List[Tuple[int, int, int]]]
    patches: Tuple = ()     # ((chunk index, (block, offset, size)), ...): rows replaced after the layout is made
    bad_files: Tuple = ()   # the files that must come out RPP_BAD_CHUNK


def block_bytes(seed: int, n: int) -> bytes:
    return random.Random(seed).randbytes(n)


def hole(size: int):
    return (HOLE, 0, size)


def block_offsets(blocks) -> List[int]:
    """The blocks back to back: block b starts where block b - 1 ends."""
    out, at = [], 0
    for b in blocks:
        out.append(at)
        at += len(b)
    return out


def align_case() -> Case:
    """Every source phase x every destination phase x ALIGN_SIZES: one file per combination, a first chunk of
    0..15 bytes that gives the second chunk its destination phase (files start on 16-byte boundaries)."""
    blocks = [block_bytes(101, 1021), block_bytes(102, 777)]
    offs = block_offsets(blocks)
    files, k = [], 0
    for sp in range(16):
        for dp in range(16):
            for size in ALIGN_SIZES:
                b = k % 2
                start = (sp - offs[b]) % 16 + 16 * (k % 37)  # (start + offs[b]) % 16 == sp, inside the block
                assert (offs[b] + start) % 16 == sp and start + size <= len(blocks[b])
                files.append([(1 - b, 5 * (k % 100), dp), (b, start, size)])
                k += 1
    return Case("align", blocks, files)


def tile_edges_cases(tile: int, lead: int) -> List[Case]:
    """``lead`` is where the caller puts file 0 in the output; file 0's chunks are cut so that their ends and
    starts fall on tile - 1, tile and tile + 1 of the OUTPUT."""
    blocks = [block_bytes(201, 3 * tile + 101), block_bytes(202, 2 * tile + 37)]
    assert 0 <= lead < tile - 2
    first = [(0, 3, tile - 1 - lead),    # ends at tile - 1
             (1, 7, 1),                  # starts at tile - 1, ends at tile
             (0, 11, 1),                 # starts at tile, ends at tile + 1
             (1, 1, tile - 2),           # starts at tile + 1, ends at 2 * tile - 1
             (0, 5, 2),                  # straddles the edge 2 * tile
             (0, 9, 2 * tile + 5)]       # spans three tiles and more
    ones = [[(k % 2, 13 + 3 * k, 1) for k in range(200)]]           # 200 chunks of 1 byte inside one tile
    many = [[(k % 2, 17 + 5 * k, 1 + k % 3) for k in range(700)]]   # more chunks in a tile than one staged batch
    exact = [[(0, 0, tile)], [(1, 16, tile)], [(0, 1, 2 * tile)]]   # whole tiles, aligned and not
    return [Case("tile_edges", blocks, [first] + ones + many + exact + [[(1, 0, tile + 1)], [(0, 2, tile - 1)]])]


def block_edges_case() -> Case:
    blocks = [block_bytes(301, 333), block_bytes(302, 4099), block_bytes(303, 61)]
    shared = [[(1, 40 * f, 100 + f), (1, 7, 50)] for f in range(24)]  # the same block used by many files
    files = [[(0, 0, 333)],                  # a chunk that is a whole block
             [(0, 0, 1)],                    # starts at byte 0 of block 0
             [(2, 0, 61)],                   # the last block, whole: ends on the last byte of the buffer
             [(2, 60, 1)],                   # the last byte of the buffer alone
             [(2, 29, 32)],                  # ends on it, longer than a granule
             [(1, 4099 - 17, 17), (0, 332, 1), (1, 0, 4099)]] + shared
    return Case("block_edges", blocks, files)


def holes_cases(tile: int) -> List[Case]:
    blocks = [block_bytes(401, 2 * tile + 9), block_bytes(402, 999)]
    files = [[hole(100), (0, 5, 300)],                          # leading
             [(1, 0, 300), hole(77)],                           # trailing
             [(0, 1, 50), hole(33), (1, 2, 50), hole(1), (0, 3, 5)],  # between data
             [hole(4097)],                                      # only a hole
             [(0, 0, tile // 2 + 3), hole(tile + 100), (1, 9, 20)],   # a hole spanning two tiles
             [(1, 3, 10), hole(0), (1, 13, 10)],                # a hole of 0 bytes
             [hole(0)],
             [hole(15), hole(1), hole(16), (0, 7, 1)]]
    return [Case("holes", blocks, files)]


def empty_cases() -> List[Case]:
    blocks = [block_bytes(501, 500), block_bytes(502, 123)]
    files = [[(0, 0, 40)],
             [],                                                # a file with no chunks
             [(1, 3, 0), (0, 500, 0), hole(0), (1, 123, 0)],    # all chunks of size 0 (offset == size is allowed)
             [],
             [(1, 100, 23)],
             []]
    return [Case("empty_files", blocks, files), Case("empty_batch", blocks, []),
            Case("only_empty_files", blocks, [[], [], []]), Case("no_blocks", [], [[hole(5)], []])]


def bad_cases() -> List[Case]:
    blocks = [block_bytes(601, 700), block_bytes(602, 300)]
    good = lambda k: [(k % 2, 10 * k, 90 + k), hole(3), (1 - k % 2, k, 35)]  # noqa: E731

    def around(name, bad_file, patches=()):
        files = [good(1), good(2), bad_file, good(3), good(4)]
        at = len(files[0]) + len(files[1])
        return Case(name, blocks, files, tuple((at + i, row) for i, row in patches), (2,))

    return [around("bad_block_index", [(0, 0, 20), (2, 0, 50), (1, 5, 20)]),          # block == nblocks
            around("bad_one_past_block", [(1, 0, 30), (1, 251, 50), (0, 1, 30)]),     # offset + size == size + 1
            around("bad_offset_wraps", [(0, 0xFFFFFFFF, 2), (0, 8, 8)]),              # 32-bit sum would wrap
            around("bad_offset_past_block_size_0", [(0, 701, 0), (0, 8, 8)]),
            # the row claims more than its place: its destination runs past the output (and into its neighbour)
            around("bad_dst_past_out", [(0, 0, 16), (1, 3, 40), (0, 16, 16)], ((1, (1, 3, 1 << 40)),)),
            around("bad_hole_past_out", [hole(24), (0, 16, 16)], ((0, hole((1 << 64) - 1)),)),
            around("bad_runs_into_neighbour", [(0, 0, 16), (1, 3, 40), (0, 16, 16)], ((1, (1, 3, 41)),))]


def families(tile: int, lead: int = 0):
    return {"align": [align_case()], "tile_edges": tile_edges_cases(tile, lead), "block_edges": [block_edges_case()],
            "holes": holes_cases(tile), "empty": empty_cases(), "bad": bad_cases()}


def all_cases(tile: int, lead: int = 0) -> List[Case]:
    return [c for cs in families(tile, lead).values() for c in cs]


def model(blocks: List[bytes], rows, dst, first, out: bytearray) -> List[int]:
    """The rules, restated: writes the good chunks of every file into ``out`` and returns the statuses."""
    status = []
    for f in range(len(first) - 1):
        status.append(0)
        for c in range(first[f], first[f + 1]):
            b, off, size = rows[c]
            fits = dst[c] + size <= min(len(out), dst[c + 1])
            if fits and (b == HOLE or (b < len(blocks) and off + size <= len(blocks[b]))):
                out[dst[c]:dst[c] + size] = bytes(size) if b == HOLE else blocks[b][off:off + size]
            else:
                status[f] = BAD_CHUNK
    return status
