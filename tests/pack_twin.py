"""numpy twin of the sequence packing of include/bsq.h ("sequence packing"), shared by tests/test_packing_host.py and
tests/test_packing_gpu.py: written from the header, not from the kernels -- the plan is the plain sequential loop, a run is the head of
the row the existing oracle writes for its sequence, and segment / position ids come from a per-position cover array."""
import numpy as np

from oracle import oracle as O

NP_DTYPES = {0: np.int8, 1: np.int16, 2: np.int32, 3: np.uint64, 4: np.float32, 5: np.float64}  # bsq_dtype code -> numpy type


def plan(offsets, P, bos, eos, mode, rows=None):
    """(starts int64[B + 1], n_rows, n_placed) by the sequential loop of the header."""
    offsets = [int(x) for x in offsets]
    B = len(offsets) - 1
    be = int(bool(bos)) + int(bool(eos))
    w = [offsets[i + 1] - offsets[i] + be for i in range(B)]
    starts = []
    row = col = total = 0
    for i in range(B):
        if mode == "nextfit":
            if i > 0 and col + w[i] > P:
                row, col = row + 1, 0
            starts.append(row * P + col)
            col += w[i]
        else:
            starts.append(total)
        total += w[i]
    n_rows = 0 if B == 0 else (row + 1 if mode == "nextfit" else max(1, -(-total // P)))
    took = [min(x, P) if mode == "nextfit" else x for x in w]
    limit = None if rows is None else rows * P
    n_placed, end = 0, 0
    for i in range(B):
        if n_placed == i and (limit is None or starts[i] + took[i] <= limit):
            n_placed, end = i + 1, starts[i] + took[i]
        else:
            starts[i] = -1
    return np.array(starts + [end], dtype=np.int64), n_rows, n_placed


def runs(key, flags, chars, offsets):
    """The runs [BOS] t .. [EOS] of every sequence, int64 arrays: the heads of the oracle's one-sequence-per-row matrix."""
    bos, eos, pad = flags
    offsets = np.asarray(offsets, dtype=np.int64)
    B = len(offsets) - 1
    if B == 0:
        return []
    w = np.diff(offsets) + int(bool(bos)) + int(bool(eos))
    tok = O.OracleTokenizer(key, eos=eos, bos=bos, padchar=pad)
    width = max(int(w.max()), 1)
    out = []
    step = max(1, (1 << 24) // width)  # the padded oracle matrix in slabs
    for b0 in range(0, B, step):
        o = offsets[b0:b0 + step + 1]
        m = tok.tokenize_packed(np.asarray(chars, dtype=np.uint8), o, width, "i", batch_first=True)
        out += [m[k, :w[b0 + k]].astype(np.int64) for k in range(len(o) - 1)]
    return out


def pad_value(key, flags):
    bos, eos, pad = flags
    return O.OracleTokenizer(key, eos=eos, bos=bos, padchar=pad).pad() if pad else 0


def pack(key, flags, chars, offsets, P, mode, rows=None, dtype=np.int64):
    """(tokens, segment_ids, position_ids, starts, n_rows, n_placed): the three (R, P) matrices of the header's rules."""
    bos, eos, _ = flags
    starts, n_rows, n_placed = plan(offsets, P, bos, eos, mode, rows)
    R = n_rows if rows is None else rows
    flat = np.full(R * P, pad_value(key, flags), dtype=np.int64)
    cover = np.full(R * P, -1, dtype=np.int64)
    pos = np.zeros(R * P, dtype=np.int64)
    for i, run in enumerate(runs(key, flags, chars, offsets)):
        s = int(starts[i])
        if s < 0:
            continue
        n = min(len(run), P) if mode == "nextfit" else len(run)
        flat[s:s + n] = run[:n]
        cover[s:s + n] = i
        pos[s:s + n] = np.arange(n)
    cover2 = cover.reshape(R, P)
    seg = np.where(cover2 >= 0, 1 + cover2 - cover2[:, :1], 0) if R else cover2
    return (flat.reshape(R, P).astype(dtype), seg.astype(np.int32), pos.reshape(R, P).astype(np.int32), starts, n_rows, n_placed)
