"""The LSH candidates of a sketch matrix in plain Python, written from the rule of include/bsq.h ("LSH candidates of a sketch matrix")
alone: Python integers for mix64, `sorted` for the runs, bucket counting of its own.  Nothing of the library is called.  The tests of
the CPU twins and of the kernels compare against it and share the matrices made here; the header's known answers come from it
(`python tests/lsh_twin.py` prints them)."""
import numpy as np

MASK = (1 << 64) - 1
EMPTY = 0xFFFFFFFF
DOMAIN = 0x4C53485F42414E44  # "LSH_BAND"
GOLDEN = 0x9E3779B97F4A7C15


def mix64(z):
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def values(a):
    """the 32-bit unsigned values of a sketch matrix of int32, int64 or uint64, as lists of Python integers"""
    return [[int(v) & EMPTY for v in row] for row in np.asarray(a)]


def keys(a, rows_per_band, seed=0):
    """(T, N) int64: key[t][i]"""
    rows, r = values(a), int(rows_per_band)
    S = np.asarray(a).shape[1]
    T = S // r
    salt = mix64((int(seed) & MASK) ^ DOMAIN)
    out = np.empty((T, len(rows)), np.int64)
    for t in range(T):
        start = mix64(salt + GOLDEN * (t + 1))
        for i, row in enumerate(rows):
            band = row[t * r:(t + 1) * r]
            h = start
            for v in band:
                h = mix64(h ^ v)
            out[t, i] = -1 if all(v == EMPTY for v in band) else h >> 1
    return out


def candidates(a, b=None, *, rows_per_band, max_bucket=32, seed=0):
    """(sorted list of the candidates (i, j), their number before the union): over one matrix the pairs i < j, over two the pairs
    (i, j - Ba) with i < Ba <= j of the concatenation"""
    a = np.asarray(a)
    Ba = a.shape[0]
    whole = a if b is None else np.concatenate([a, np.asarray(b)])
    found, total = set(), 0
    for band in keys(whole, rows_per_band, seed):
        order = sorted(range(len(band)), key=lambda i: (int(band[i]), i))
        runs, at = [], 0
        while at < len(order):
            end = at
            while end < len(order) and band[order[end]] == band[order[at]]:
                end += 1
            if band[order[at]] != -1:
                runs.append(order[at:end])
            at = end
        for run in runs:
            if len(run) <= max_bucket:
                pairs = [(run[x], run[y]) for y in range(len(run)) for x in range(y)]
            else:
                pairs = [(run[0], j) for j in run[1:]]
            assert all(i < j for i, j in pairs)
            total += len(pairs)
            found.update(pairs)
    if b is not None:
        found = {(i, j - Ba) for i, j in found if i < Ba <= j}
    return sorted(found), total


def counts(x, y):
    """(match, either) of two rows of 32-bit values"""
    match = sum(1 for p, q in zip(x, y) if p == q and p != EMPTY)
    either = sum(1 for p, q in zip(x, y) if p != EMPTY or q != EMPTY)
    return match, either


def compare_list(a, row, col, b=None):
    """(match, either) int32 arrays of listed pairs; an index outside its matrix gives -1, -1"""
    va = values(a)
    vb = va if b is None else values(b)
    out = [counts(va[i], vb[j]) if 0 <= i < len(va) and 0 <= j < len(vb) else (-1, -1) for i, j in zip(map(int, row), map(int, col))]
    return np.array([m for m, _ in out], np.int32), np.array([e for _, e in out], np.int32)


def passes(match, either, min_jaccard, min_match):
    return match >= min_match and match * 65536 >= int(float(min_jaccard) * 65536 + 0.5) * either


def lsh_pairs(a, b=None, *, rows_per_band, min_jaccard=0.5, min_match=1, max_bucket=32, seed=0):
    """(row, col, match, either, pair_offsets) as numpy arrays"""
    a = np.asarray(a)
    va = values(a)
    vb = va if b is None else values(b)
    cand, _ = candidates(a, b, rows_per_band=rows_per_band, max_bucket=max_bucket, seed=seed)
    rows = []
    for i, j in cand:
        m, e = counts(va[i], vb[j])
        if passes(m, e, min_jaccard, min_match):
            rows.append((i, j, m, e))
    row = np.array([x[0] for x in rows], np.int64)
    offs = np.searchsorted(row, np.arange(a.shape[0] + 1)).astype(np.int64)
    return (row, np.array([x[1] for x in rows], np.int64), np.array([x[2] for x in rows], np.int32), np.array([x[3] for x in rows], np.int32), offs)


# ---- shared inputs ----
def random_sketches(seed, N, S, dtype=np.int32, *, fill=1.0, groups=()):
    """(N, S) sketches of random 32-bit values below EMPTY, each bucket filled with probability `fill`; groups: lists of row indices,
    the rows of a list made identical to its first row"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 0xFFFFFFFE, (N, S), dtype=np.uint64, endpoint=True)
    v[rng.random((N, S)) >= fill] = EMPTY
    for g in groups:
        v[list(g)] = v[g[0]]
    return as_dtype(v, dtype)


def as_dtype(v, dtype):
    """32-bit values as a sketch matrix of `dtype`: int32 holds the bits, int64 / uint64 the value, EMPTY as all bits set"""
    v = np.asarray(v, np.uint64)
    if np.dtype(dtype) == np.int32:
        return v.astype(np.uint32).view(np.int32)
    wide = np.where(v == EMPTY, np.uint64(MASK), v)
    return wide.view(np.int64) if np.dtype(dtype) == np.int64 else wide


def near_duplicates(seed, N, S, dtype=np.int32, *, share=0.1, keep=0.8, fill=1.0):
    """random sketches in which `share` of the rows copy an earlier row and keep each bucket with probability `keep`"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 0xFFFFFFFE, (N, S), dtype=np.uint64, endpoint=True)
    v[rng.random((N, S)) >= fill] = EMPTY
    for j in rng.choice(np.arange(1, N), max(1, int(N * share)), replace=False):
        src = int(rng.integers(0, j))
        mask = rng.random(S) < keep
        v[j, mask] = v[src, mask]
    return as_dtype(v, dtype)


def header_batch():
    """the plain sketches of the MinHash section's batch (ACGTAC, ACGNACGT, AC, "", TTTTTTT: DNA4, k = 3, S = 4, seed 0) are rows 0 and 1
    equal with two filled buckets, rows 2 and 3 EMPTY throughout, row 4 with one filled bucket of its own; the known answers below use a
    matrix of that shape written out in full, so that they depend on this section's rule alone"""
    E = EMPTY
    return as_dtype([[7, E, 9, E], [7, E, 9, E], [E, E, E, E], [E, E, E, E], [E, 5, E, E], [7, E, 3, E]], np.int32)


if __name__ == "__main__":
    m = header_batch()
    for r in (1, 2, 3, 4):
        print("r", r, "keys", keys(m, r).tolist())
    for r, mb in ((1, 32), (2, 32), (4, 32), (1, 2)):
        c, total = candidates(m, rows_per_band=r, max_bucket=mb)
        print("r", r, "max_bucket", mb, "candidates", c, "before the union", total)
        print("   pairs at 0.5:", [x.tolist() for x in lsh_pairs(m, rows_per_band=r, max_bucket=mb)])
    print("two:", candidates(m[:2], m[2:], rows_per_band=1), [x.tolist() for x in lsh_pairs(m[:2], m[2:], rows_per_band=1)])
    print("seed 1 r 2:", keys(m, 2, 1).tolist())
