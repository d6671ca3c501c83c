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
