"""numpy restatement of the k-mer spectrum (include/bsq.h, "k-mer spectrum"): per row and per window a Horner sum or a skip, np.add.at,
and the division in np.float32 / np.float64.  Written from the rule, not from the library's code."""
import numpy as np

MAX_WINDOWS = 1 << 23
NP_DTYPES = {2: np.int32, 3: np.int64, 4: np.float32, 5: np.float64}  # bsq_dtype code -> element type (BSQ_U64: int64 bits)


def n_windows(L, k, s):
    L = max(int(L), 0)
    return min(0 if L < k else (L - k) // s + 1, MAX_WINDOWS)


def rc_ids(V, k):
    """rc(v) for every v of the 4 ** k vocabulary: id(rc(w)) = sum_j (3 - c_j) * 4 ** j with c_0 the window's first character."""
    out = np.zeros(V, dtype=np.int64)
    for v in range(V):
        digits = [(v // 4 ** (k - 1 - j)) % 4 for j in range(k)]  # c_0 .. c_{k-1}
        out[v] = sum((3 - c) * 4 ** j for j, c in enumerate(digits))
    return out


def window_ids(lut, A, seq, k, s):
    """Ids of the row's counted windows (those without an unmapped character), in order."""
    n = n_windows(len(seq), k, s)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    cls = lut[np.asarray(seq, dtype=np.uint8)].astype(np.int64)
    w = cls[np.arange(n)[:, None] * s + np.arange(k)[None, :]]  # (n, k): window j is characters [j * s, j * s + k)
    v = np.zeros(n, dtype=np.int64)
    for i in range(k):  # Horner, first character most significant
        v = v * A + w[:, i]
    return v[(w >= 0).all(axis=1)]


def counts(lut, A, chars, offs, k, s, both_strands=False):
    """(B, A ** k) int64 counts."""
    V = A ** k
    B = len(offs) - 1
    out = np.zeros((B, V), dtype=np.int64)
    rc = rc_ids(V, k) if both_strands else None
    for i in range(B):
        ids = window_ids(lut, A, np.asarray(chars[offs[i]:max(offs[i + 1], offs[i])]), k, s)
        np.add.at(out[i], ids, 1)
        if both_strands:
            np.add.at(out[i], rc[ids], 1)
    return out


def spectrum(lut, A, chars, offs, k, s, dt, both_strands=False, normalize=False):
    """The matrix the library writes for element type code `dt`, bit for bit."""
    c = counts(lut, A, chars, offs, k, s, both_strands)
    T = NP_DTYPES[dt]
    if not normalize:
        return c.astype(T)
    S = c.sum(axis=1, keepdims=True)
    out = np.zeros(c.shape, dtype=T)
    rows = S[:, 0] > 0
    out[rows] = c[rows].astype(T) / S[rows].astype(T)
    return out
