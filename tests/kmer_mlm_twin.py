"""numpy twin of the span-masked k-mer masked-LM draw of include/bsq.h ("k-mer masked-LM", `bsq_kmer_mlm`), shared by
tests/test_kmer_mlm_host.py and tests/test_kmer_mlm_gpu.py: an independent restatement of the rule, not a port of the library's code --
per row, the anchors over range(n), the coverage by a plain loop over every anchor's span, then the replacement.  The plain ids come
from tests/kmer_twin.py."""
import math

import numpy as np

import kmer_twin

U64 = np.uint64
NP_DTYPES = kmer_twin.NP_DTYPES
K_SEED, GOLDEN, STEP = 0x4B4D45524D4C4D53, 0x9E3779B97F4A7C15, 0xD1342543DE82EF95
M64 = 2 ** 64 - 1


def mix64(z):
    """splitmix64's finalizer on Python integers."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def threshold(p):
    return int(math.floor(float(p) * 65536.0 + 0.5))


def row_key(seed, row):
    return mix64(((int(seed) ^ K_SEED) & M64) + GOLDEN * (row + 1))


def anchors(h_row, n, anchor_prob):
    """bool[n]: anchor(a) for the window indices 0 .. n - 1 of a row."""
    T = threshold(anchor_prob)
    out = np.zeros(n, dtype=bool)
    for a in range(n):
        w = mix64(h_row + STEP * ((a >> 2) + 1))
        out[a] = ((w >> (16 * (a & 3))) & 0xFFFF) < T
    return out


def coverage(anch, span):
    """bool[n]: the union of [a, a + span) over the anchors, cut at n."""
    n = len(anch)
    cov = np.zeros(n, dtype=bool)
    for a in np.flatnonzero(anch):
        cov[a:min(n, a + span)] = True
    return cov


def span_anchor_prob(frac, span):
    return 1.0 - (1.0 - float(frac)) ** (1.0 / span)


def mlm(lut, A, chars, offsets, k, s, P, bos=False, eos=False, padchar=False, *, anchor_prob, span, mask_prob=0.8, random_prob=0.1,
        mask_token=None, ignore_index=-100, seed=0, first_row=0, details=None, fast=False):
    """(inputs, labels) as int64 (B, P).  details: a list that receives (n, anchors, covered, selected) per row.  fast: the plain ids
    from kmer_twin.rows_fast (the vectorised form, for the larger GPU cases)."""
    plain = (kmer_twin.rows_fast if fast else kmer_twin.rows)(lut, A, chars, offsets, k, s, P, bos, eos, padchar)
    sp = kmer_twin.specials(A, k, bos, eos, padchar)
    V = A ** k
    mask_token = sp["vocab"] if mask_token is None else mask_token
    tm, tr = threshold(mask_prob), threshold(mask_prob) + threshold(random_prob)
    inputs, labels = plain.copy(), np.full_like(plain, ignore_index)
    b0 = int(bool(bos))
    room = max(P - b0 - int(bool(eos)), 0)
    for i in range(len(offsets) - 1):
        n = min(kmer_twin.count(int(offsets[i + 1] - offsets[i]), k, s), room)
        h = row_key(seed, first_row + i)
        anch = anchors(h, n, anchor_prob)
        cov = coverage(anch, span)
        ids = plain[i, b0:b0 + n]
        sel = cov & (ids != V)
        for j in np.flatnonzero(sel):
            j = int(j)
            v = mix64((~h & M64) + STEP * (j + 1))
            cat, rnd = v & 0xFFFF, (v >> 16) & 0xFFFFFFFF
            labels[i, b0 + j] = ids[j]
            inputs[i, b0 + j] = mask_token if cat < tm else ((rnd * V) >> 32 if cat < tr else ids[j])
        if details is not None:
            details.append((n, anch, cov, sel))
    return inputs, labels


def fates(seed, row, sel, mask_prob, random_prob):
    """int8[n] per window of batch row `row` (first_row included): 0 not selected, 1 mask token, 2 random id, 3 keeps its id -- the
    category of the replacement word, for the tests that look at one branch (sel: the row's `selected` of mlm()'s details)."""
    h = row_key(seed, row)
    tm, tr = threshold(mask_prob), threshold(mask_prob) + threshold(random_prob)
    out = np.zeros(len(sel), dtype=np.int8)
    for j in np.flatnonzero(sel):
        cat = mix64((~h & M64) + STEP * (int(j) + 1)) & 0xFFFF
        out[j] = 1 if cat < tm else (2 if cat < tr else 3)
    return out


def matrices(*a, batch_first=True, in_dtype=np.int64, label_dtype=np.int64, **kw):
    """What bsq_kmer_mlm_tokenize_* writes: (B, P) or (P, B), C-contiguous, in the element types (int64 -> uint64 keeps the bits)."""
    inputs, labels = mlm(*a, **kw)

    def cast(m, t):
        m = np.ascontiguousarray(m if batch_first else m.T)
        return m.view(np.uint64) if np.dtype(t) == np.uint64 else m.astype(t)

    return cast(inputs, in_dtype), cast(labels, label_dtype)
