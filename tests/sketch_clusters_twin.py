"""The single-linkage clusters of a sketch matrix, restated from the text of include/bsq.h ("sketch clusters") alone: the upper pair list of
tests/sketch_pairs_twin.py fed to a plain sequential union-find that hooks the larger root under the smaller, and the inputs the cluster
tests share -- a path through scrambled rows, groups of identical rows.  The split of `cluster_split` is restated in Python integers.
Nothing of the library is called here."""
import numpy as np

import minhash_twin
import sketch_pairs_twin


def labels_of_pairs(row, col, n):
    """labels (int64, n) of the edge list: an entry with row == col or an index outside 0 .. n - 1 is ignored"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for i, j in zip(np.asarray(row).tolist(), np.asarray(col).tolist()):
        if i == j or not (0 <= i < n and 0 <= j < n):
            continue
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)
    return np.array([find(x) for x in range(n)], dtype=np.int64).reshape(n)


def labels(a, min_match=1, T=32768, compared=None):
    """labels of the rule: the links are the upper pairs of the pair twin"""
    row, col = sketch_pairs_twin.pairs(a, None, min_match, T, compared)[:2]
    return labels_of_pairs(row, col, len(a))


def _as(values, dtype):
    """uint32 bucket values (EMPTY = 0xFFFFFFFF) as the element type stores them"""
    values = np.asarray(values, np.uint64)
    if dtype == np.int32:
        return values.astype(np.uint32).view(np.int32)
    out = values.copy()
    out[values == 0xFFFFFFFF] = np.uint64(2 ** 64 - 1)
    return out.view(np.int64)


def chain(B, S, seed, dtype, cut=False):
    """(B, S) rows, S even: the row at chain position p holds p // 2 in its even buckets and (p + 1) // 2 + 2^20 in its odd ones, the
    positions laid out through a seeded permutation of the rows.  Consecutive positions agree in exactly S / 2 of S filled buckets,
    positions two apart in none: at min_match 1, T = q16(0.5) the graph is ONE path of B - 1 links that hops between strips and tiles in a
    scrambled order, at T + 1 it has no link.  cut: the row of every 50th position (49, 99, ...) is EMPTY throughout, which cuts the path
    into pieces and leaves singletons."""
    assert S % 2 == 0
    p = np.arange(B, dtype=np.uint64)
    rows = np.empty((B, S), np.uint64)
    rows[:, 0::2] = (p // np.uint64(2))[:, None]
    rows[:, 1::2] = ((p + np.uint64(1)) // np.uint64(2) + np.uint64(1 << 20))[:, None]
    if cut:
        rows[49::50] = 0xFFFFFFFF
    out = np.empty_like(rows)
    out[np.random.default_rng(seed).permutation(B)] = rows
    return _as(out, dtype)


def cliques(B, S, sizes, seed, dtype=np.int32):
    """(B, S) rows in groups of identical rows of the given sizes (they sum to B), the rows permuted; the groups differ in every bucket,
    so at T = 65536 every pair inside a group passes and no other"""
    assert sum(sizes) == B
    group = np.repeat(np.arange(len(sizes), dtype=np.uint64), sizes)
    rows = group[:, None] * np.uint64(1000) + np.arange(S, dtype=np.uint64)[None, :]
    out = np.empty_like(rows)
    out[np.random.default_rng(seed).permutation(B)] = rows
    return _as(out, dtype)


def table(lab):
    """(representatives, sizes, dense_id) of a label array, one row at a time"""
    reps = [i for i, v in enumerate(lab.tolist()) if v == i]
    sizes = [int((lab == r).sum()) for r in reps]
    rank = {r: k for k, r in enumerate(reps)}
    return np.array(reps, np.int64), np.array(sizes, np.int64), np.array([rank[v] for v in lab.tolist()], np.int64)


def split(lab, fractions, seed=0):
    """the split of every row in Python integers: h = mix64((seed + label + 0x9E3779B97F4A7C15) mod 2^64), u = h >> 32, the first s with
    u < floor((f_0 + ... + f_s) * 2^32), the last split taking the rest"""
    bounds, run = [], 0.0
    for f in fractions[:-1]:
        run += float(f)
        bounds.append(int(run * 4294967296.0))
    out = []
    for v in lab.tolist():
        u = minhash_twin.mix64_int(seed + v + 0x9E3779B97F4A7C15) >> 32
        out.append(next((s for s, b in enumerate(bounds) if u < b), len(bounds)))
    return np.array(out, np.int64).reshape(len(lab))
