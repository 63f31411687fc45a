"""Writes tests/golden/order_kat.json: known answers for the nilsimsa fragment ordering (--order=nilsimsa).

    python tests/golden/make_order_kat.py

Pure Python, host only: the ordering restated with Python ints and lists from its description (include/ricepp_amd.h,
the order group; the reference's similarity_ordering.cpp and inode_element_view.cpp).  This model is the third
restatement next to the host C++ and the HIP kernels; the reference itself is not compiled (it needs fmt).

"tables" hold elements; a case names its table, so cases that differ in the index or the options share the rows.
A table's digests are one base64 string of its 32-byte rows (the four words w0..w3, little endian: the digest bytes
as the hash kernels write them), its sizes one digit per element into "size_choices", its rank a list.  Lists of
ids are packed: [start, count] stands for count ascending numbers (`unpack`).
"order": whole orderings with the model's permutation and statistics, and for the full-node and threshold cases
the root split's child of every visited element.
"split": one node's split at a given max_distance.  "chain": one chain over from/to id lists.
"params": the pass widths and the LDS capacity of the kernels that the sizes around them were built for.
"""
import base64
import json
import random
from pathlib import Path

HERE = Path(__file__).resolve().parent
MASK = (1 << 256) - 1
FLIPS = (0, 1, 2, 3, 8, 20, 60)
PARAMS = {"split_pass_children": 1024, "chain_threads": 256, "chain_stage_rows": 896}


def words(v):
    return [(v >> (64 * i)) & (2**64 - 1) for i in range(4)]


def to_hex(v):
    return "".join(f"{w:016x}" for w in words(v))


def from_hex(s):
    return sum(int(s[16 * i:16 * i + 16], 16) << (64 * i) for i in range(4))


def pack(values):
    """A list of ints with every ascending run of four or more written as [start, count]."""
    out, i, values = [], 0, list(values)
    while i < len(values):
        j = i
        while j + 1 < len(values) and values[j + 1] == values[j] + 1:
            j += 1
        if j - i >= 3:
            out.append([values[i], j - i + 1])
        else:
            out.extend(values[i:j + 1])
        i = j + 1
    return out


def unpack(packed):
    out = []
    for x in packed:
        out.extend(range(x[0], x[0] + x[1]) if isinstance(x, list) else [x])
    return out


def write_table(bits, sizes, rank):
    choices = sorted(set(sizes))
    assert len(choices) <= 10
    return {"digests": base64.b64encode(b"".join(v.to_bytes(32, "little") for v in bits)).decode(),
            "size_choices": choices, "sizes": "".join(str(choices.index(x)) for x in sizes), "rank": pack(rank)}


def read_table(t):
    """(digests as 256-bit ints, sizes, rank) of a table of the file."""
    raw = base64.b64decode(t["digests"])
    bits = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
    return bits, [t["size_choices"][int(c)] for c in t["sizes"]], unpack(t["rank"])


if hasattr(int, "bit_count"):
    def distance(a, b):
        return (a ^ b).bit_count()
else:
    def distance(a, b):
        return bin(a ^ b).count("1")


class Centroid:
    def __init__(self):
        self.value, self.counts, self.members = 0, [0] * 256, 0

    def add(self, v):
        self.members += 1
        value = 0
        for bit in range(256):
            self.counts[bit] += (v >> bit) & 1
            if self.counts[bit] > self.members // 2:
                value |= 1 << bit
        self.value = value


def split(bits, index, max_children, max_distance, stats=None):
    """One node: (child of every element of `index` in visiting order, the children's lists in creation order)."""
    cents, lists, child = [], [], []
    for e in index:
        v = bits[e]
        match, best, best_d, tie = None, None, None, False
        for c, cen in enumerate(cents):
            d = distance(cen.value, v)
            if d <= max_distance:
                match = c
                break
            if best_d is None or d < best_d:
                best, best_d, tie = c, d, False
            elif d == best_d:
                tie = True
        if match is None:
            if len(cents) < max_children:
                cents.append(Centroid())
                lists.append([])
                match = len(cents) - 1
            else:
                match = best
                if stats is not None:
                    stats["fallbacks"] += 1
                    stats["fallback_ties"] += tie
        cents[match].add(v)
        lists[match].append(e)
        child.append(match)
    return child, lists


def chain(count, frm, to, stats=None, rotate=False):
    """The permutation (entries by their original place) the chain leaves; frm(p) / to(p): the rows of entry p.
    rotate: what a rotate in place of the swap would give (only to show that a case tells them apart)."""
    perm = list(range(count))
    for i in range(count - 1):
        a = frm(perm[i])
        best_d, best_k = None, 0
        for k in range(i + 1, count):
            d = distance(a, to(perm[k]))
            if best_d is None or d < best_d:
                best_d, best_k = d, k
                if d <= 1:
                    if stats is not None:
                        stats["chain_early_stops"] += 1
                    break
        if rotate:
            perm.insert(i + 1, perm.pop(best_k))
        elif best_k > 0 and best_k != i + 1:
            perm[i + 1], perm[best_k] = perm[best_k], perm[i + 1]
    return perm


def order(bits, sizes, rank, index, max_children, max_cluster_size):
    """Steps 1-6: (the ordered ids, statistics, the root split's child per visited element)."""
    st = dict(fallbacks=0, fallback_ties=0, chain_early_stops=0, depth=0, leaves=0, largest_leaf=0,
              largest_final_leaf=0, largest_node=0, duplicate_groups=0, unique=0)
    if not index:
        return [], st, []
    order_key = lambda e: (-sizes[e], rank[e])  # noqa: E731
    srt = sorted(index, key=lambda e: (words(bits[e]), rank[e]))
    unique, dups = [], {}
    for e in srt:
        if unique and bits[unique[-1]] == bits[e]:
            dups.setdefault(unique[-1], []).append(e)
        else:
            unique.append(e)
    st["duplicate_groups"], st["unique"] = len(dups), len(unique)
    root_child = []

    def cluster(lst, max_distance, level):
        """-> the node as ("inner", [children]); a leaf is ("leaf", [ids])."""
        st["depth"] = max(st["depth"], level)
        child, lists = split(bits, lst, max_children, max_distance, st)
        if level == 1:
            root_child.extend(child)
        st["largest_node"] = max(st["largest_node"], len(lists))
        children = []
        for sub in lists:
            if max_distance > 1 and len(sub) > max_cluster_size:
                children.append(cluster(sub, max_distance // 2, level + 1))
                continue
            st["leaves"] += 1
            st["largest_leaf"] = max(st["largest_leaf"], len(sub))
            if max_distance == 1:
                st["largest_final_leaf"] = max(st["largest_final_leaf"], len(sub))
            if len(sub) > 1:
                sub = sorted(sub, key=order_key)
                sub = [sub[p] for p in chain(len(sub), lambda p: bits[sub[p]], lambda p: bits[sub[p]], st)]
            children.append(("leaf", sub))
        return ("inner", children)

    def order_tree(node):
        """-> (the node with its children ordered, first id, last id, weight)."""
        kind, body = node
        if kind == "leaf":
            return node, body[0], body[-1], sum(sizes[e] for e in body)
        entries = [order_tree(c) for c in body]
        entries.sort(key=lambda en: -en[3])  # (stable)
        perm = chain(len(entries), lambda p: bits[entries[p][2]], lambda p: bits[entries[p][1]], st)
        entries = [entries[p] for p in perm]
        return ("inner", [en[0] for en in entries]), entries[0][1], entries[-1][2], sum(en[3] for en in entries)

    def collect(node, out):
        kind, body = node
        if kind == "leaf":
            for e in body:
                out.append(e)
                out.extend(sorted(dups.get(e, []), key=order_key))
        else:
            for c in body:
                collect(c, out)

    out = []
    collect(order_tree(cluster(unique, 128, 1))[0], out)
    return out, st, root_child


def total_distance(bits, ids):
    return sum(distance(bits[a], bits[b]) for a, b in zip(ids, ids[1:]))


# ---- inputs ----

def flip(rng, v, f):
    for b in rng.sample(range(256), f):
        v ^= 1 << b
    return v


def families(rng, n, flips=FLIPS, max_members=12):
    """n digests: random bases, every member of a family its base with f random bits flipped."""
    out = []
    while len(out) < n:
        base, f = rng.getrandbits(256), rng.choice(flips)
        out.extend(flip(rng, base, f) for _ in range(min(rng.randint(1, max_members), n - len(out))))
    return out


def table(rng, digests):
    n = len(digests)
    rank = list(range(n))
    rng.shuffle(rank)
    return list(digests), [rng.choice((1, 4096, 4096, 65536)) for _ in range(n)], rank


def spread(rng, count, f=60, apart=64):
    """`count` digests, each a common base with f bits flipped, every pair more than `apart` bits apart."""
    base, out = rng.getrandbits(256), []
    while len(out) < count:
        v = flip(rng, base, f)
        if all(distance(v, o) > apart for o in out):
            out.append(v)
    return out


def build():
    rng = random.Random(20261020)
    B, T, S = PARAMS["split_pass_children"], PARAMS["chain_threads"], PARAMS["chain_stage_rows"]
    tables, orders, splits, chains = {}, [], [], []

    def add_order(name, tab, index, max_children, max_cluster_size, why, keep_root=False):
        bits, sizes, rank = tables[tab]
        out, st, root_child = order(bits, sizes, rank, list(index), max_children, max_cluster_size)
        assert sorted(out) == sorted(index)
        orders.append({"name": name, "why": why, "table": tab, "index": pack(index), "max_children": max_children,
                       "max_cluster_size": max_cluster_size, "order": pack(out), "stats": st,
                       "root_child": root_child if keep_root else None,
                       "total_distance": [total_distance(bits, list(index)), total_distance(bits, out)]})
        return st

    def add_split(name, tab, index, max_children, max_distance, why):
        child, lists = split(tables[tab][0], index, max_children, max_distance)
        splits.append({"name": name, "why": why, "table": tab, "index": pack(index), "max_children": max_children,
                       "max_distance": max_distance, "child": pack(child), "nchildren": len(lists)})
        return child, lists

    def add_chain(name, tab, frm, to, why):
        bits, frm, to = tables[tab][0], list(frm), list(to)
        perm = chain(len(frm), lambda p: bits[frm[p]], lambda p: bits[to[p]])
        chains.append({"name": name, "why": why, "table": tab, "from": pack(frm), "to": None if to == frm else pack(to),
                       "perm": pack(perm)})
        return perm

    # whole orderings
    tables["mix"] = table(rng, families(rng, 300))
    add_order("empty", "mix", [], 16384, 16384, "empty index")
    add_order("one", "mix", [7], 16384, 16384, "n = 1")
    add_order("two", "mix", [11, 3], 16384, 16384, "n = 2")
    add_order("mix_default", "mix", range(300), 16384, 16384, "family mix, default options")
    sub = rng.sample(range(300), 120)
    add_order("subset", "mix", sub, 8, 16, "a proper subset of a larger table, in no order")
    tables["equal"] = table(rng, [rng.getrandbits(256)] * 9)
    st = add_order("all_equal", "equal", range(9), 16384, 16384, "one unique element and a duplicate list")
    assert st["unique"] == 1 and st["duplicate_groups"] == 1
    for mc in (1, 2, 4):
        st = add_order(f"max_children_{mc}", "mix", range(300), mc, 8, "the full-node rule", keep_root=True)
        # (one child cannot tie with another: the tie is asked of 2 and 4)
        assert st["fallbacks"] > 0 and (mc == 1 or st["fallback_ties"] > 0), st
    tight = []
    for _ in range(10):
        base = rng.getrandbits(256)
        tight.extend(flip(rng, base, f) for f in [0] + [1] * 9 + [2] * 3 + [3] * 2)
    tables["tight"] = table(rng, tight)
    st = add_order("depth8", "tight", range(len(tight)), 256, 4, "clusters survive to max_distance 1")
    assert st["depth"] == 8 and st["largest_final_leaf"] > 4, st
    far, near_of = spread(rng, B + 1), (0, 1, B // 2, B - 3, B - 2, B - 1, B)
    tables["spread"] = table(rng, far + [flip(rng, far[i], 1) for i in near_of])
    for delta in (-1, 0, 1):
        idx = list(range(B + delta)) + [B + 1 + j for j, i in enumerate(near_of) if i < B + delta]
        st = add_order(f"children_B{delta:+d}", "spread", idx, 16384, 512,
                       "a node with B - 1, B, B + 1 children; its tree chain is longer than the LDS holds")
        assert st["largest_node"] == B + delta, st

    # threshold: a one-member child and an element at exactly max_distance and max_distance + 1
    a = rng.getrandbits(256)
    thr = [a] + [flip(rng, a, d) for d in (128, 129, 64, 65, 1, 2)] + [rng.getrandbits(256)]
    tables["threshold"] = table(rng, thr)
    for md, at, over in ((128, 1, 2), (64, 3, 4), (1, 5, 6)):
        child, _ = add_split(f"at_{md}", "threshold", [0, at, 7], 16, md, "distance == max_distance joins")
        assert child[1] == 0
        child, _ = add_split(f"over_{md}", "threshold", [0, over, 7], 16, md, "distance == max_distance + 1 does not")
        assert child[1] == 1
    tables["threshold_order"] = ([0, MASK >> 128 << 128, MASK >> 127 << 127, 2**64 - 1], [1, 2, 3, 4], [2, 0, 3, 1])
    add_order("root_at_128", "threshold_order", [0, 1, 3], 16, 16, "three elements, one at exactly 128 from the first",
              keep_root=True)
    add_order("root_at_129", "threshold_order", [0, 2, 3], 16, 16, "three elements, one at exactly 129 from the first",
              keep_root=True)
    assert orders[-2]["root_child"][:2] == [0, 0] and orders[-1]["root_child"][:2] == [0, 1]

    # majority: members that disagree on bits 0..3, then a probe that only count > members / 2 places right
    bit = lambda *bs: sum(1 << b for b in bs)  # noqa: E731
    maj = [0, bit(0, 1, 2, 3), bit(0, 1, 2, 3, 7), bit(0, 1, 8, 9, 10),          # the members
           bit(0, 1, 2, 3, 4, 5), bit(0, 1, 2, 3, 4, 5, 6, 8, 9), bit(0, 1, 4, 5, 6), bit(2, 3, 4, 5, 6)]  # probes
    tables["majority"] = table(rng, maj)
    c2, _ = add_split("majority_2", "majority", [0, 1, 4], 16, 5, "2 members: a bit held by one is clear")
    c3, _ = add_split("majority_3", "majority", [0, 1, 2, 5], 16, 5, "3 members: a bit held by two is set")
    c4, _ = add_split("majority_4", "majority", [0, 1, 2, 3, 6, 7], 16, 5, "4 members: a bit held by two is clear")
    assert c2 == [0, 0, 1] and c3 == [0, 0, 0, 0] and c4 == [0, 0, 0, 0, 0, 1], (c2, c3, c4)

    # splits of B - 1, B, B + 1 children, with elements that join the last ones
    for delta in (-1, 0, 1):
        idx = list(range(B + delta)) + [B + 1 + j for j, i in enumerate(near_of) if i < B + delta]
        child, lists = add_split(f"wide_B{delta:+d}", "spread", idx, 16384, 64, "children per pass - 1, =, + 1")
        assert len(lists) == B + delta and child[-1] == B + delta - 1
    add_split("wide_full", "spread", list(range(B + 1)) + [B + 7, B + 1], B, 64,
              "a full node of B children: the elements past it go to the nearest")

    # chains
    x = rng.getrandbits(256)
    edge = [x, flip(rng, x, 9), flip(rng, x, 1), x, flip(rng, x, 5), flip(rng, x, 5), flip(rng, x, 3),
            x ^ 1, x ^ (7 << 10), x ^ (7 << 20)]
    tables["chain_edges"] = table(rng, edge)
    p = add_chain("d1_before_d0", "chain_edges", [0, 1, 2, 3], [0, 1, 2, 3], "the d == 1 entry comes first and wins")
    assert p[:2] == [0, 2]
    p = add_chain("tie_lowest_k", "chain_edges", [0, 4, 5], [0, 4, 5], "two entries at the minimum: the lowest k")
    assert p == [0, 1, 2]
    ids = [0, 8, 9, 7]  # 7 is nearest to 0; 8 and 9 are equally far from 7
    p = add_chain("swap_not_rotate", "chain_edges", ids, ids, "the swap leaves 9 before 8, a rotate 8 before 9")
    ebits = tables["chain_edges"][0]
    assert p == [0, 3, 2, 1] and chain(4, lambda q: ebits[ids[q]], lambda q: ebits[ids[q]], rotate=True) == [0, 3, 1, 2]
    # lengths around the pass width and the LDS capacity, over the spread table's last rows: far rows and, from 11
    # rows on, the near copies of four of them, so that steps end early on a d == 1 beyond the first pass
    n_spread = len(tables["spread"][0])
    assert n_spread >= S + 1
    for length in sorted({1, 2, 3, T - 1, T, T + 1, S - 1, S, S + 1}):
        ids = range(n_spread - length, n_spread)
        add_chain(f"leaf_{length}", "spread", ids, ids, "segment length")
    for length in (3, T + 1, S + 1):
        add_chain(f"tree_{length}", "spread", range(n_spread - length, n_spread), range(length), "to != from")
    tables = {name: write_table(*t) for name, t in tables.items()}
    return {"params": PARAMS, "tables": tables, "order": orders, "split": splits, "chain": chains}


def dumps(kat):
    """One table or case a line."""
    one = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    lines = ['{"params":' + one(kat["params"]) + ',', '"tables":{']
    lines += [",\n".join(one(k) + ":" + one(v) for k, v in kat["tables"].items()) + "}"]
    for group in ("order", "split", "chain"):
        lines[-1] += ","
        lines += ['"%s":[' % group, ",\n".join(one(c) for c in kat[group]) + "]"]
    return "\n".join(lines) + "}\n"


if __name__ == "__main__":
    kat = build()
    path = HERE / "order_kat.json"
    path.write_text(dumps(kat))
    print(path, path.stat().st_size, "bytes;", len(kat["order"]), "orderings,", len(kat["split"]), "splits,",
          len(kat["chain"]), "chains")
