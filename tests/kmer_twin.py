"""numpy twin of the k-mer ids of include/bsq.h (`bsq_kmer`), shared by tests/test_kmers_host.py and tests/test_kmers_gpu.py: an
independent restatement of the rules -- per row, per window, a Horner sum or UNK -- not a port of the library's code."""
import numpy as np

NP_DTYPES = {0: np.int8, 1: np.int16, 2: np.int32, 3: np.uint64, 4: np.float32, 5: np.float64}  # bsq_dtype code -> numpy type


def specials(A, k, bos, eos, padchar):
    """{"unk", "bos", "eos", "pad", "vocab"}: bos / eos are -1 where the flag is off, pad is the id whether or not it is stored."""
    V = A ** k
    return {"unk": V, "bos": V + 1 if bos else -1, "eos": V + 1 + bool(bos) if eos else -1, "pad": V + 1 + bool(bos) + bool(eos),
            "vocab": V + 1 + bool(bos) + bool(eos) + bool(padchar)}


def count(L, k, s):
    return 0 if L < k else (L - k) // s + 1


def rows(lut, A, chars, offsets, k, s, P, bos=False, eos=False, padchar=False):
    """The (B, P) int64 matrix of the rules."""
    lut = np.asarray(lut, dtype=np.int64)
    sp = specials(A, k, bos, eos, padchar)
    weights = A ** np.arange(k - 1, -1, -1, dtype=np.int64)
    B = len(offsets) - 1
    out = np.full((B, P), sp["pad"] if padchar else 0, dtype=np.int64)
    for b in range(B):
        seq = lut[np.asarray(chars[offsets[b]:offsets[b + 1]], dtype=np.uint8)]
        n = min(count(len(seq), k, s), max(P - bool(bos) - bool(eos), 0))
        row = [sp["bos"]] if bos else []
        for j in range(n):
            w = seq[j * s:j * s + k]
            row.append(sp["unk"] if (w < 0).any() else int((w * weights).sum()))
        if eos:
            row.append(sp["eos"])
        row = row[:P]
        out[b, :len(row)] = row
    return out


def matrix(lut, A, chars, offsets, k, s, P, bos=False, eos=False, padchar=False, batch_first=True, dtype=np.int64):
    """What bsq_kmer_tokenize_* writes: (B, P) or (P, B), C-contiguous, in the element type."""
    m = rows(lut, A, chars, offsets, k, s, P, bos, eos, padchar)
    return np.ascontiguousarray(m if batch_first else m.T).astype(dtype)


def rows_fast(lut, A, chars, offsets, k, s, P, bos=False, eos=False, padchar=False):
    """The same matrix, vectorised over the batch for the large GPU cases (checked against rows() in the host tests)."""
    lut = np.asarray(lut, dtype=np.int64)
    sp = specials(A, k, bos, eos, padchar)
    offsets = np.asarray(offsets, dtype=np.int64)
    B = len(offsets) - 1
    room = max(P - bool(bos) - bool(eos), 0)
    L = np.diff(offsets)
    n = np.minimum(np.where(L < k, 0, (L - k) // s + 1), room)
    ids = lut[np.asarray(chars, dtype=np.uint8)]
    j = np.arange(room, dtype=np.int64)[None, :]
    live = j < n[:, None]
    val = np.zeros((B, room), dtype=np.int64)
    unk = np.zeros((B, room), dtype=bool)
    for i in range(k):
        at = np.where(live, offsets[:-1, None] + j * s + i, 0)
        c = ids[at] if ids.size else np.zeros_like(at)
        unk |= c < 0
        val = val * A + np.maximum(c, 0)
    body = np.where(unk, sp["unk"], val)
    out = np.full((B, P), sp["pad"] if padchar else 0, dtype=np.int64)
    b0 = int(bool(bos))
    if bos:
        out[:, 0] = sp["bos"]
    width = min(room, P - b0)
    out[:, b0:b0 + width] = np.where(live, body, out[:, b0:b0 + width])[:, :width]
    if eos:
        at = n + b0
        ok = at < P
        out[np.arange(B)[ok], at[ok]] = sp["eos"]
    return out


# What an element type holds (include/bsq.h, "what an element type holds"), restated as a table: bsq_dtype code -> [lo, hi], the integers
# that survive the conversion to the type and back.  The host tests check the table itself by doing that conversion with numpy.
HOLDS = {0: (-2 ** 7, 2 ** 7 - 1), 1: (-2 ** 15, 2 ** 15 - 1), 2: (-2 ** 31, 2 ** 31 - 1), 3: (-2 ** 63, 2 ** 63 - 1), 4: (-2 ** 24, 2 ** 24),
         5: (-2 ** 53, 2 ** 53)}


def holds(dt, lo, hi):
    r = HOLDS.get(dt)
    return r is not None and r[0] <= lo and hi <= r[1]


def back(a):
    """A matrix the library wrote, as int64 values (uint64 holds an int64's bits): the comparison that does not pass through the
    element type on the expected side."""
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.uint64 else a.astype(np.int64)


def edge_bytes(lut, A, k):
    """(first, last, unmapped, top): a byte of class 0, a byte of the highest class the table maps, an unmapped byte, and the id of k
    copies of `last` -- V - 1, except under BYTES, whose int8 table maps the bytes below 0x80 only (its top id is 127 * (V - 1) / 255)."""
    lut = np.asarray(lut, dtype=np.int64)
    A_top = int(lut.max())
    first, last = int(np.flatnonzero(lut == 0)[0]), int(np.flatnonzero(lut == A_top)[0])
    return first, last, int(np.flatnonzero(lut < 0)[-1]), sum(A_top * A ** i for i in range(k))


def edge_pool(lut):
    """Bytes to draw random sequences from: the first byte of every mapped class, about one unmapped byte in 25."""
    lut = np.asarray(lut, dtype=np.int64)
    firsts = np.array([np.flatnonzero(lut == c)[0] for c in range(int(lut.max()) + 1)], dtype=np.uint8)
    unmapped = np.flatnonzero(lut < 0).astype(np.uint8)
    body = np.tile(firsts, -(-48 // firsts.size))
    return np.concatenate([body, unmapped[[0, -1] * max(1, body.size // 48)]])
