"""numpy twin of the masked-LM draw of include/bsq.h (`bsq_mlm`), shared by tests/test_masking_host.py and tests/test_masking_gpu.py."""
import math

import numpy as np

U64 = np.uint64
K_SEED, GOLDEN, STEP = 0x4D4C4D5F4D41534B, 0x9E3779B97F4A7C15, 0xD1342543DE82EF95


def mix64(z):
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def threshold(p):
    return int(math.floor(float(p) * 65536.0 + 0.5))


def row_keys(seed, first_row, B):
    rows = np.arange(B, dtype=U64) + U64(first_row + 1)
    with np.errstate(over="ignore"):
        return mix64(U64((int(seed) ^ K_SEED) & (2 ** 64 - 1)) + U64(GOLDEN) * rows)


def draw(lut, chars, offsets, frac, seed, first_row=0):
    """Per character of the packed batch (index k - offsets[0]): row, j, selected, cat16, rnd16."""
    offsets = np.asarray(offsets, dtype=np.int64)
    B = len(offsets) - 1
    lens = np.diff(offsets)
    total = int(offsets[-1] - offsets[0])
    row = np.repeat(np.arange(B, dtype=np.int64), lens)
    j = np.arange(total, dtype=np.int64) + offsets[0] - offsets[row] if total else np.zeros(0, np.int64)
    h = row_keys(seed, first_row, B)[row] if total else np.zeros(0, U64)
    ju = j.astype(U64)
    with np.errstate(over="ignore"):
        w = mix64(h + U64(STEP) * ((ju >> U64(2)) + U64(1)))
        v = mix64(~h + U64(STEP) * (ju + U64(1)))
    sel16 = ((w >> (U64(16) * (ju & U64(3)))) & U64(0xFFFF)).astype(np.int64)
    c = np.asarray(chars, dtype=np.uint8)[offsets[0]:offsets[-1]]
    mapped = np.asarray(lut, dtype=np.int8)[c] >= 0
    selected = (sel16 < threshold(frac)) & mapped
    cat = (v & U64(0xFFFF)).astype(np.int64)
    rnd = ((v >> U64(16)) & U64(0xFFFF)).astype(np.int64)
    return row, j, selected, cat, rnd, sel16


def mask(lut, chars, offsets, frac, seed, first_row=0):
    """The byte mask of bsq_random_mask_*: 0 = selected, 1 elsewhere (bytes outside the sequences: 1)."""
    out = np.ones(len(chars), dtype=np.uint8)
    _, _, selected, _, _, _ = draw(lut, chars, offsets, frac, seed, first_row)
    out[offsets[0]:offsets[-1]] = np.where(selected, 0, 1)
    return out


def mlm(plain_bp, lut, nchars, bos, eos, chars, offsets, frac, mask_prob, random_prob, mask_token, ignore_index, seed, first_row=0):
    """Expected (inputs, labels) as int64 (B, P) from the plain (B, P) tokens: the draw applied at the selected characters that fit."""
    plain = np.asarray(plain_bp, dtype=np.int64)
    B, P = plain.shape
    inputs, labels = plain.copy(), np.full_like(plain, ignore_index)
    row, j, selected, cat, rnd, _ = draw(lut, chars, offsets, frac, seed, first_row)
    t = j + int(bos)
    keep = selected & (j < P - int(bos) - int(eos))  # (characters past the room of an over-long sequence are clamped away)
    r, t, cat, rnd = row[keep], t[keep], cat[keep], rnd[keep]
    tm, tr = threshold(mask_prob), threshold(mask_prob) + threshold(random_prob)
    repl = np.where(cat < tm, mask_token, np.where(cat < tr, (rnd * nchars) >> 16, plain[r, t]))
    labels[r, t] = plain[r, t]
    inputs[r, t] = repl
    return inputs, labels
