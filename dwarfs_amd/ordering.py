"""The nilsimsa fragment order (``--order=nilsimsa``, the reference's default) over the MI355X kernels.

``similarity_hashes(files)`` -> ``order_nilsimsa(digests, sizes)`` goes from file bytes to the order in which the
files are segmented: the permutation of the reference's ``similarity_ordering::order_nilsimsa``
(src/writer/internal/similarity_ordering.cpp), element for element.  The popcount-of-XOR work -- every split of
the cluster tree and every nearest-neighbour chain -- runs in the two kernels of the order group of
``include/ricepp_amd.h``; the sorts, the regrouping of a level by (node, child), the tree bookkeeping and the
collect are numpy on the host.  ``host_order_nilsimsa`` is the same order from the library's sequential host code.
"""

from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _native as N
from .codec import _raise_status, _stream_ptr
from .section import _ptr

U32_MAX = 0xFFFFFFFF


def pass_children() -> int:
    """Children one pass of the split kernel compares an element with."""
    return int(N.lib().rpp_order_split_pass_children())


def chain_threads() -> int:
    """Entries one pass of the chain kernel covers."""
    return int(N.lib().rpp_order_chain_threads())


def chain_stage_rows() -> int:
    """The longest segment the chain kernel keeps in LDS."""
    return int(N.lib().rpp_order_chain_stage_rows())


def check_options(max_children: int, max_cluster_size: int) -> None:
    if not (0 <= int(max_children) <= U32_MAX and 0 <= int(max_cluster_size) <= U32_MAX):
        raise ValueError("max_children and max_cluster_size are 32-bit counts")
    _raise_status(N.lib().rpp_order_check_options(int(max_children), int(max_cluster_size)))


def as_words(digests) -> np.ndarray:
    """Digest rows (uint8 [n, 32] as ``similarity_hash_batch`` returns them, or uint64 [n, 4]) as uint64 [n, 4]:
    the four little-endian words of the reference's ``std::array<uint64_t, 4>``."""
    if isinstance(digests, torch.Tensor):
        digests = digests.cpu().numpy()
    a = np.ascontiguousarray(digests)
    if a.dtype == np.uint8:
        a = a.reshape(-1, 32).view("<u8")
    elif a.dtype != np.uint64:
        raise ValueError("digests are uint8 [n, 32] or uint64 [n, 4]")
    return np.ascontiguousarray(a.reshape(-1, 4).astype(np.uint64, copy=False))


def _inputs(digests, sizes, rank, index) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    bits = as_words(digests)
    n = bits.shape[0]
    if n >= U32_MAX:
        raise ValueError("too many elements")
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1)
    rank = np.arange(n, dtype=np.uint32) if rank is None else np.ascontiguousarray(rank, dtype=np.uint32).reshape(-1)
    index = np.arange(n, dtype=np.uint32) if index is None else np.ascontiguousarray(index, dtype=np.uint32).reshape(-1)
    if sizes.size != n or rank.size != n:
        raise ValueError("one size and one rank per digest")
    if index.size and int(index.max()) >= n:
        raise ValueError("index names an element that is not there")
    if np.unique(index).size != index.size:
        raise ValueError("index names an element twice")
    return bits, sizes, rank, index


def _hp(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def total_distance(digests, order) -> int:
    """Sum of the distances of neighbours in ``order`` (what the reference logs before and after ordering)."""
    bits = as_words(digests)
    order = np.asarray(order, dtype=np.int64)
    if order.size < 2:
        return 0
    x = bits[order[:-1]] ^ bits[order[1:]]
    return int(np.unpackbits(x.view(np.uint8)).sum(dtype=np.int64))


def host_order_nilsimsa(digests, sizes, rank=None, index=None, max_children: int = 16384,
                        max_cluster_size: int = 16384, device=None, return_stats: bool = False):
    """The order on the host (``rpp_order_host_nilsimsa``, one thread); with ``return_stats`` also the run's
    statistics (``rpp_order_stats`` as a dict).  ``device`` is accepted for symmetry and not used."""
    check_options(max_children, max_cluster_size)
    bits, sizes, rank, index = _inputs(digests, sizes, rank, index)
    out = np.zeros(index.size, dtype=np.uint32)
    st = N.RppOrderStats()
    _raise_status(N.lib().rpp_order_host_nilsimsa(_hp(bits), _hp(sizes), _hp(rank), bits.shape[0], _hp(index), index.size,
                                                  int(max_children), int(max_cluster_size), _hp(out), C.byref(st)))
    if return_stats:
        return out, {name: int(getattr(st, name)) for name, _ in st._fields_ if name != "reserved"}
    return out


def host_split(digests, index, max_children: int, max_distance: int) -> Tuple[np.ndarray, int]:
    """One node's split on the host: (child per element of ``index``, child count)."""
    bits = as_words(digests)
    index = np.ascontiguousarray(index, dtype=np.uint32)
    child, nch = np.zeros(index.size, dtype=np.uint32), C.c_uint32(0)
    _raise_status(N.lib().rpp_order_host_split(_hp(bits), bits.shape[0], _hp(index), index.size, int(max_children),
                                               int(max_distance), _hp(child), C.byref(nch)))
    return child, int(nch.value)


def host_chain(digests, from_ids, to_ids=None) -> np.ndarray:
    """One chain on the host: the entry (by its place in the lists) left at every place."""
    bits = as_words(digests)
    frm = np.ascontiguousarray(from_ids, dtype=np.uint32)
    to = frm if to_ids is None else np.ascontiguousarray(to_ids, dtype=np.uint32)
    if to.size != frm.size:
        raise ValueError("one `to` id per `from` id")
    perm = np.zeros(frm.size, dtype=np.uint32)
    _raise_status(N.lib().rpp_order_host_chain(_hp(bits), bits.shape[0], _hp(frm), _hp(to), frm.size, _hp(perm)))
    return perm


# ---- device ----

def _dev_u32(a, device) -> torch.Tensor:
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32).copy()).to(device)


def _to_u32(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def device_bits(digests, device="cuda") -> torch.Tensor:
    """The digest rows on the device as int64 [n, 4] (the words' bit patterns)."""
    return torch.from_numpy(as_words(digests).view(np.int64).copy()).to(device)


def split_batch(d_bits: torch.Tensor, index, node_start, max_children: int, max_distance: int,
                stream: Optional[torch.cuda.Stream] = None) -> Tuple[np.ndarray, np.ndarray]:
    """``rpp_order_split_batch`` for the nodes ``index[node_start[j] : node_start[j + 1]]``: (child per slot,
    child count per node) on the host (synchronises)."""
    dev = d_bits.device
    index = np.ascontiguousarray(index, dtype=np.uint32)
    node_start = np.ascontiguousarray(node_start, dtype=np.uint32)
    n_nodes = node_start.size - 1
    if n_nodes < 0 or (n_nodes >= 0 and int(node_start[-1]) != index.size):
        raise ValueError("node_start has one entry per node and one more, the last the length of index")
    if n_nodes == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    m = np.diff(node_start.astype(np.int64))
    if m.min() < 0:
        raise ValueError("node_start descends")
    slots_of = np.minimum(m, int(max_children))
    base = np.zeros(n_nodes, dtype=np.uint64)
    base[1:] = np.cumsum(slots_of[:-1])
    slots = int(slots_of.sum())
    L = N.lib()
    ws_bytes = int(L.rpp_order_split_workspace_bytes(slots))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    d_index, d_start = _dev_u32(index if index.size else np.zeros(1, np.uint32), dev), _dev_u32(node_start, dev)
    d_base = torch.from_numpy(base.view(np.int64).copy()).to(dev)
    d_child = torch.zeros(max(index.size, 1), dtype=torch.int32, device=dev)
    d_nch = torch.zeros(n_nodes, dtype=torch.int32, device=dev)
    _raise_status(L.rpp_order_split_batch(_ptr(d_bits), d_bits.shape[0], _ptr(d_index), _ptr(d_start), _ptr(d_base),
                                          n_nodes, slots, int(max_children), int(max_distance), _ptr(d_child),
                                          _ptr(d_nch), _ptr(ws), ws_bytes, _stream_ptr(stream)))
    if stream is not None:
        stream.synchronize()
    child, nch = _to_u32(d_child)[:index.size], _to_u32(d_nch)
    if (nch == U32_MAX).any():
        raise RuntimeError("rpp_order_split_batch refused a node (an id out of range or a workspace too small)")
    return child, nch


def chain_batch(d_bits: torch.Tensor, from_ids, to_ids, seg_start,
                stream: Optional[torch.cuda.Stream] = None) -> np.ndarray:
    """``rpp_order_chain_batch``: for every segment the entry, counted from the segment's start, left at every
    place (host array, synchronises).  ``to_ids=None``: the `from` rows (a leaf)."""
    dev = d_bits.device
    seg_start = np.ascontiguousarray(seg_start, dtype=np.uint32)
    from_ids = np.ascontiguousarray(from_ids, dtype=np.uint32)
    n_seg = seg_start.size - 1
    if n_seg < 0 or int(seg_start[-1]) != from_ids.size or (to_ids is not None and len(to_ids) != from_ids.size):
        raise ValueError("seg_start has one entry per segment and one more, the last the length of the id lists")
    if n_seg == 0 or from_ids.size == 0:
        return np.zeros(0, np.uint32)
    d_from = _dev_u32(from_ids, dev)
    d_to = d_from if to_ids is None else _dev_u32(to_ids, dev)
    d_start = _dev_u32(seg_start, dev)
    d_perm = torch.zeros(from_ids.size, dtype=torch.int32, device=dev)
    _raise_status(N.lib().rpp_order_chain_batch(_ptr(d_bits), d_bits.shape[0], _ptr(d_from), _ptr(d_to), _ptr(d_start),
                                                n_seg, _ptr(d_perm), _stream_ptr(stream)))
    if stream is not None:
        stream.synchronize()
    perm = _to_u32(d_perm)
    if (perm == U32_MAX).any():
        raise RuntimeError("rpp_order_chain_batch refused a segment (an id out of range)")
    return perm


@dataclass
class _Level:
    """The clusters one tree level's splits made, grouped by parent in creation order."""

    parent: np.ndarray           # the cluster of the level above each one came from (level 1: all 0, the root)
    count: np.ndarray            # its elements
    start: np.ndarray            # where they begin in `elems`
    elems: np.ndarray            # the level's elements, cluster by cluster, in insertion order
    is_split: np.ndarray         # split again on the next level (else a leaf)
    first: np.ndarray = field(default=None)
    last: np.ndarray = field(default=None)
    weight: np.ndarray = field(default=None)
    pos: np.ndarray = field(default=None)    # where the cluster's elements begin in the final unique order


def _group_starts(keys: np.ndarray) -> np.ndarray:
    """Starts (and the end) of the runs of equal values in a sorted array."""
    if keys.size == 0:
        return np.zeros(1, np.int64)
    return np.concatenate(([0], np.flatnonzero(keys[1:] != keys[:-1]) + 1, [keys.size])).astype(np.int64)


def order_nilsimsa(digests, sizes, rank=None, index=None, max_children: int = 16384, max_cluster_size: int = 16384,
                   device="cuda", timings: Optional[Dict[str, float]] = None) -> np.ndarray:
    """The nilsimsa order of the elements ``index`` (default: all) as uint32 ids.  ``digests``: the rows of
    ``similarity_hash_batch(kind="nilsimsa")``; ``sizes``: the weights; ``rank``: distinct numbers standing for the
    reference's path order (default: the element's own number).  ``timings`` (a dict) receives the seconds spent
    in the split launches, the leaf chains, the tree chains and the host plumbing."""
    check_options(max_children, max_cluster_size)
    bits, sizes, rank, index = _inputs(digests, sizes, rank, index)
    tm = {"split": 0.0, "leaf_chain": 0.0, "tree_chain": 0.0, "levels": 0}
    t_begin = time.perf_counter()

    def timed(key, fn, *args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn(*args)
        torch.cuda.synchronize()
        tm[key] += time.perf_counter() - t0
        return r

    def finish(out):
        if timings is not None:
            total = time.perf_counter() - t_begin
            timings.update(tm, total=total, plumbing=total - tm["split"] - tm["leaf_chain"] - tm["tree_chain"])
        return out

    if index.size == 0:
        return finish(np.zeros(0, np.uint32))
    d_bits = device_bits(bits, device)

    # 1. duplicates: sort by (w0, w1, w2, w3, rank); the first of every run of equal rows stays, in this order
    b = bits[index]
    srt = index[np.lexsort((rank[index], b[:, 3], b[:, 2], b[:, 1], b[:, 0]))]
    sb = bits[srt]
    new_run = np.ones(srt.size, dtype=bool)
    new_run[1:] = (sb[1:] != sb[:-1]).any(axis=1)
    run_of = np.cumsum(new_run) - 1          # per sorted element: its run = its unique element's number
    unique = srt[new_run]

    # 2. the cluster tree, one split launch per level
    levels = []
    node_elems, node_start = unique, np.array([0, unique.size], dtype=np.int64)
    node_cluster = np.zeros(1, dtype=np.int64)  # the cluster (of the level above) every node of this launch is
    max_distance = 128
    while node_start.size > 1:
        child, _ = timed("split", split_batch, d_bits, node_elems, node_start, max_children, max_distance)
        tm["levels"] += 1
        node_of = np.repeat(np.arange(node_start.size - 1, dtype=np.int64), np.diff(node_start))
        key = node_of * (int(child.max()) + 1) + child.astype(np.int64)
        o = np.argsort(key, kind="stable")
        gs = _group_starts(key[o])
        count = np.diff(gs)
        is_split = (count > int(max_cluster_size)) if max_distance > 1 else np.zeros(count.size, dtype=bool)
        lv = _Level(parent=node_cluster[node_of[o][gs[:-1]]], count=count, start=gs[:-1], elems=node_elems[o],
                    is_split=is_split)
        levels.append(lv)
        which = np.flatnonzero(is_split)
        sel = np.repeat(is_split, count)
        node_elems = lv.elems[sel]
        node_start = np.concatenate(([0], np.cumsum(count[which]))).astype(np.int64)
        node_cluster = which
        max_distance //= 2

    # 3. leaves: sort by (size descending, rank), chain every leaf in one launch
    for lv in levels:
        leaf = ~lv.is_split
        sel = np.repeat(leaf, lv.count)
        e = lv.elems[sel]
        leaf_of = np.repeat(np.arange(lv.count.size, dtype=np.int64), lv.count)[sel]
        o = np.lexsort((rank[e], ~sizes[e], leaf_of))
        e = e[o]
        seg = np.concatenate(([0], np.cumsum(lv.count[leaf]))).astype(np.int64)
        perm = timed("leaf_chain", chain_batch, d_bits, e, None, seg)
        e = e[np.repeat(seg[:-1], lv.count[leaf]) + perm.astype(np.int64)]
        lv.elems = lv.elems.copy()
        lv.elems[sel] = e                     # (a leaf's slots are contiguous: its chained order in place)
        lv.first, lv.last = lv.elems[lv.start], lv.elems[lv.start + lv.count - 1]
        csum = np.concatenate(([np.uint64(0)], np.cumsum(sizes[lv.elems], dtype=np.uint64)))
        lv.weight = csum[lv.start + lv.count] - csum[lv.start]   # (only the leaves' entries are used)

    # 5. tree order, deepest level first: the children of every parent, heaviest first, chained last -> first
    child_order = [None] * len(levels)
    for depth in range(len(levels) - 1, -1, -1):
        lv = levels[depth]
        o = np.lexsort((~lv.weight, lv.parent))    # (stable: equal weights keep creation order)
        seg = _group_starts(lv.parent[o])
        perm = timed("tree_chain", chain_batch, d_bits, lv.last[o], lv.first[o], seg)
        o = o[np.repeat(seg[:-1], np.diff(seg)) + perm.astype(np.int64)]
        child_order[depth] = (o, seg)
        if depth:
            up, parents = levels[depth - 1], lv.parent[o][seg[:-1]]
            up.first[parents], up.last[parents] = lv.first[o][seg[:-1]], lv.last[o][seg[1:] - 1]
            wsum = np.concatenate(([np.uint64(0)], np.cumsum(lv.weight[o], dtype=np.uint64)))
            up.weight[parents] = wsum[seg[1:]] - wsum[seg[:-1]]

    # 6. collect: every cluster's place in the final order, top down; then the duplicates behind their element
    place = np.zeros(unique.size, dtype=np.int64)
    up_pos = np.zeros(1, dtype=np.int64)
    for depth, lv in enumerate(levels):
        o, seg = child_order[depth]
        c = lv.count[o]
        before = np.cumsum(c) - c
        lv.pos = np.zeros(lv.count.size, dtype=np.int64)
        lv.pos[o] = up_pos[lv.parent[o]] + before - np.repeat(before[seg[:-1]], np.diff(seg))
        leaf = ~lv.is_split
        sel = np.repeat(leaf, lv.count)
        within = np.arange(lv.elems.size, dtype=np.int64) - np.repeat(lv.start, lv.count)
        place[(np.repeat(lv.pos, lv.count) + within)[sel]] = lv.elems[sel]
        up_pos = lv.pos
    # place[p] = the unique element at position p; order the sorted elements by (their unique's position,
    # the unique itself first, then size descending and rank)
    pos_of_elem = np.zeros(bits.shape[0], dtype=np.int64)
    pos_of_elem[place] = np.arange(place.size)
    upos = pos_of_elem[unique][run_of]
    out = srt[np.lexsort((rank[srt], ~sizes[srt], ~new_run, upos))]
    return finish(out.astype(np.uint32))
