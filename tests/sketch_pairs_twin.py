"""The thresholded pair list of two sketch matrices, restated from the text of include/bsq.h ("sketch pairs") alone: the comparison of
tests/minhash_twin.py, the threshold in numpy integers, `np.nonzero` for the (i, j) order.  Nothing of the library is called here."""
import numpy as np

import minhash_twin

VALUES = np.array([0xFFFFFFFF, 0, 1, 2, 3, 4, 5, 2 ** 31, 2 ** 32 - 2], dtype=np.uint64)


def sketch_like(rng, B, S, dtype, values=VALUES.size):
    """(B, S) values drawn from the first `values` of {EMPTY, 0 .. 5, 2^31, 2^32 - 2}, as the element type stores them"""
    v = VALUES[rng.integers(0, values, (B, S))]
    if dtype == np.int32:
        return v.astype(np.uint32).view(np.int32)
    v[v == 0xFFFFFFFF] = np.uint64(2 ** 64 - 1)
    return v.view(np.int64)


def case(seed, Ba, Bb, S, dtype, upper=False):
    """(a, b) of a test case, b None for `upper`: rows drawn by sketch_like -- a pair of them agrees in about a tenth of its buckets --
    and, from three rows on, row 1 of a EMPTY throughout (a row that pairs with nothing at min_match >= 1) and three identical rows
    planted: the last row of a, the first and the last of b (upper: rows 0, B // 2 and B - 1 of a).  The planted row has an EMPTY bucket
    in front (S >= 2), so that not even it reaches match == S."""
    rng = np.random.default_rng(seed)
    a = sketch_like(rng, Ba, S, dtype)
    b = None if upper else sketch_like(rng, Bb, S, dtype)
    if Ba >= 3:
        a[1] = -1
        plant = sketch_like(rng, 1, S, dtype)[0]
        plant[-1] = 3
        if S >= 2:
            plant[0] = -1
        if upper:
            a[0] = a[Ba // 2] = a[Ba - 1] = plant
        else:
            a[Ba - 1] = b[0] = b[Bb - 1] = plant
    return a, b


# the middle threshold of a case by its width: min_jaccard a little above the 8 / 80 two drawn rows score on average
MID_JACCARD = {1: 0.5, 7: 0.25, 33: 0.2, 64: 0.14, 100: 0.13, 1024: 0.105, 16384: 0.1005}


def thresholds(S):
    """(name, min_match, jaccard_q16): every pair; a middle one; identical rows only; one nothing of `case` passes"""
    return [("all", 0, 0), ("mid", min(2, S), q16(MID_JACCARD[S])), ("equal", 1, 65536), ("none", S, 65536)]


def q16(min_jaccard):
    """jaccard_q16 of a threshold"""
    return int(np.floor(min_jaccard * 65536 + 0.5))


def pairs(a, b=None, min_match=1, T=32768, compared=None):
    """(row, col, match, either, pair_offsets) of the rule: b None = upper; compared: minhash_twin.compare(a, b) when it is at hand"""
    upper = b is None
    b = a if upper else b
    match, either = minhash_twin.compare(a, b) if compared is None else compared
    m, e = match.astype(np.int64), either.astype(np.int64)
    ok = (m >= min_match) & (m * 65536 >= T * e)
    if upper:
        ok = np.triu(ok, k=1)
    row, col = np.nonzero(ok)  # (row-major: ascending (i, j))
    offsets = np.zeros(len(a) + 1, np.int64)
    np.cumsum(ok.sum(1), out=offsets[1:])
    return row.astype(np.int64), col.astype(np.int64), match[row, col].astype(np.int32), either[row, col].astype(np.int32), offsets


def duplicates(B, row, col):
    """(keep, first) from the upper pair list of a matrix of B rows"""
    first = np.arange(B, dtype=np.int64)
    for i, j in zip(row, col):
        first[j] = min(first[j], i)
    return first == np.arange(B), first
