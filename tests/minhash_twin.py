"""The MinHash sketch and the sketch comparison, restated from the text of include/bsq.h ("MinHash sketch") alone: numpy uint64 arrays
(whose products and sums wrap modulo 2^64, which is the arithmetic the rule asks for) and Python integers.  Nothing of the library is
called here."""
import numpy as np

M64 = (1 << 64) - 1
DOMAIN = 0x534B455443485F5F
EMPTY = 0xFFFFFFFF
NP_DTYPES = {2: np.int32, 3: np.uint64}


def mix64_int(z):
    """splitmix64's finalizer on a Python integer"""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix64(z):
    """the same on a uint64 array"""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def salt(seed):
    return mix64_int((seed & M64) ^ DOMAIN)


def row_hashes(lut, A, row, k, canonical, seed):
    """h of every window of the row that has no unmapped character, in window order (uint64)"""
    n = min(max(row.size - k + 1, 0), 1 << 30)
    if n == 0:
        return np.zeros(0, np.uint64)
    ids = lut[row].astype(np.int64)
    bad = np.concatenate([[0], np.cumsum(ids < 0)])
    whole = (bad[k:k + n] - bad[:n]) == 0
    dig = np.where(ids < 0, 0, ids).astype(np.uint64)
    word = np.zeros(n, np.uint64)
    for i in range(k):  # the lexicographic Horner sum: first character most significant
        word = word * np.uint64(A) + dig[i:i + n]
    if canonical:
        rc = np.zeros(n, np.uint64)
        for i in range(k):  # rc(w)[i] = 3 - w[k - 1 - i]
            rc = rc * np.uint64(4) + (np.uint64(3) - dig[k - 1 - i:k - 1 - i + n])
        word = np.minimum(word, rc)
    return mix64(word[whole] ^ np.uint64(salt(seed)))


def batch_hashes(lut, A, chars, offs, k, canonical=False, seed=0):
    """row_hashes of every row of a packed batch: what sketches of several widths S share"""
    return [row_hashes(lut, A, chars[max(int(offs[b]), 0):max(int(offs[b + 1]), int(offs[b]), 0)], k, canonical, seed) for b in range(len(offs) - 1)]


def sketch_row(lut, A, row, k, S, canonical=False, seed=0, hashes=None):
    """the S buckets of one row as uint32"""
    h = row_hashes(lut, A, row, k, canonical, seed) if hashes is None else hashes
    bucket = ((h >> np.uint64(32)) * np.uint64(S)) >> np.uint64(32)
    value = np.minimum(h & np.uint64(0xFFFFFFFF), np.uint64(0xFFFFFFFE))
    tab = np.full(S, EMPTY, np.uint64)
    np.minimum.at(tab, bucket.astype(np.int64), value)
    return tab.astype(np.uint32)


def sketch(lut, A, chars, offs, k, S, dtype, canonical=False, seed=0, hashes=None):
    """the (B, S) matrix as the library's element type `dtype` (2: BSQ_I32, 3: BSQ_U64); hashes: batch_hashes of the same arguments"""
    hashes = batch_hashes(lut, A, chars, offs, k, canonical, seed) if hashes is None else hashes
    B = len(offs) - 1
    tab = np.empty((B, S), np.uint32)
    for b in range(B):
        tab[b] = sketch_row(None, A, None, k, S, hashes=hashes[b])
    if dtype == 2:
        return tab.view(np.int32)
    out = tab.astype(np.uint64)
    out[tab == EMPTY] = np.uint64(M64)
    return out


def merge(a, b):
    """bucket-wise unsigned minimum of two uint32 sketches"""
    return np.minimum(a, b)


def compare(a, b):
    """(match, either) of two sketch matrices of any integer type: the low 32 bits of an element are read"""
    ua = a.astype(np.uint64) & np.uint64(0xFFFFFFFF)
    ub = b.astype(np.uint64) & np.uint64(0xFFFFFFFF)
    match, either = np.empty((len(ua), len(ub)), np.int32), np.empty((len(ua), len(ub)), np.int32)
    for i in range(len(ua)):  # (a row of `a` against all of b: the broadcast of the header, one slice at a time)
        row = ua[i][None, :]
        match[i] = ((row == ub) & (row != EMPTY)).sum(-1)
        either[i] = ((row != EMPTY) | (ub != EMPTY)).sum(-1)
    return match, either


def revcomp(row):
    """the reverse complement of an ACGT row (other bytes are kept, reversed)"""
    table = np.arange(256, dtype=np.uint8)
    for x, y in zip(b"ACGTacgt", b"TGCAtgca"):
        table[x] = y
    return table[row[::-1]]
