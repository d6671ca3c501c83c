"""numpy twin of the crop / strand draw of include/bsq.h (`bsq_crop`), written from the header text; shared by tests/test_views_host.py
and tests/test_views_gpu.py.  It does not call the library."""
import math

import numpy as np

U64 = np.uint64
K_SEED, GOLDEN = 0x43524F5056494557, 0x9E3779B97F4A7C15
MODES = {"random": 0, "head": 1, "center": 2}
PAIRS = "AT CG RY KM BV DH"


def _comp():
    t = np.arange(256, dtype=np.uint8)
    for a, b in PAIRS.split():
        for x, y in ((a, b), (a.lower(), b.lower())):
            t[ord(x)], t[ord(y)] = ord(y), ord(x)
    return t


COMP = _comp()


def mix64(z):
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def threshold(p):
    return int(math.floor(float(p) * 65536.0 + 0.5))


def row_keys(seed, first_row, n):
    rows = np.arange(n, dtype=U64) + U64(first_row + 1)
    with np.errstate(over="ignore"):
        return mix64(U64((int(seed) ^ K_SEED) & (2 ** 64 - 1)) + U64(GOLDEN) * rows)


def plan(offsets, window, index=None, mode="random", revcomp_frac=0.0, seed=0, first_row=0):
    """(starts, lengths, strand) of the views of rows index[0 .. n) (None: every sequence) of a store with these offsets."""
    offsets = np.asarray(offsets, dtype=np.int64)
    L = np.maximum(np.diff(offsets), 0)
    idx = np.arange(L.size, dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
    Ls = L[idx]
    n = Ls.size
    h = row_keys(seed, first_row, n)
    crop = (window > 0) & (Ls > window)
    length = np.where(crop, window, Ls)
    starts = np.zeros(n, dtype=np.int64)
    for i in np.nonzero(crop)[0]:
        span = int(Ls[i]) - window
        if mode == "random":
            starts[i] = (int(h[i]) * (span + 1)) >> 64
        elif mode == "center":
            starts[i] = span // 2
    rc = (mix64(~h) >> U64(48)).astype(np.int64) < threshold(revcomp_frac)
    return starts, length.astype(np.int64), rc.astype(np.uint8)


def apply(chars, offsets, seq, starts, lengths, strand):
    """The packed batch (chars, offsets) of the views (seq[i], starts[i], lengths[i], strand[i]) of a host store."""
    chars = np.asarray(chars, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.int64)
    pieces = []
    for j, s, n, r in zip(seq, starts, lengths, strand):
        piece = chars[offsets[j] + s: offsets[j] + s + n]
        pieces.append(COMP[piece[::-1]] if r else piece)
    out_offs = np.zeros(len(pieces) + 1, dtype=np.int64)
    np.cumsum([p.size for p in pieces], out=out_offs[1:])
    out = np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)
    return out.astype(np.uint8), out_offs


def crop(chars, offsets, window, index=None, **kw):
    """The twin's crop_packed on a host store: (chars, offsets, starts, strand)."""
    starts, lengths, strand = plan(offsets, window, index, **kw)
    seq = np.arange(len(offsets) - 1) if index is None else np.asarray(index, dtype=np.int64)
    out, offs = apply(chars, offsets, seq, starts, lengths, strand)
    return out, offs, starts, strand
