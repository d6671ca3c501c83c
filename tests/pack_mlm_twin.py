"""numpy twin of the masked-LM batches over sequence-packed rows of include/bsq.h ("sequence packing", bsq_pack_mlm_tokenize_device),
shared by tests/test_pack_mlm_host.py and tests/test_pack_mlm_gpu.py: written from the header, not from the kernel -- it composes the
two existing twins.  pack_twin gives the plan and the plain packed matrices, mlm_twin.draw the fate of every character of the batch,
and every selected character of a placed sequence that survives the next-fit cut scatters to q = starts[i] + bos + j."""
import numpy as np

import mlm_twin
import pack_twin

NP_DTYPES = pack_twin.NP_DTYPES


def pack_mlm(key, flags, lut, nchars, chars, offsets, P, mode, *, rows=None, frac=0.15, mask_prob=0.8, random_prob=0.1, mask_token=None,
             ignore_index=-100, seed=0, first_row=0):
    """(inputs, labels, segment_ids, position_ids, starts, n_rows, n_placed): inputs and labels int64 (R, P), the ids int32.
    lut: int8[256] of the alphabet, nchars its size; mask_token=None: one past the tokenizer's last id."""
    bos, eos, pad = (int(bool(f)) for f in flags)
    offsets = np.asarray(offsets, dtype=np.int64)
    tokens, seg, pos, starts, n_rows, n_placed = pack_twin.pack(key, flags, chars, offsets, P, mode, rows)
    if mask_token is None:
        mask_token = nchars + bos + eos + pad
    R = tokens.shape[0]
    inputs = tokens.reshape(-1).astype(np.int64)
    labels = np.full(R * P, ignore_index, dtype=np.int64)
    row, j, selected, cat, rnd, _ = mlm_twin.draw(lut, chars, offsets, frac, seed, first_row)
    if row.size:
        s = starts[row]
        keep = selected & (s >= 0)
        if mode == "nextfit":
            keep &= bos + j < P  # the cut of a run wider than the row
        q = (s + bos + j)[keep]
        plain = inputs[q]
        tm = mlm_twin.threshold(mask_prob)
        tr = tm + mlm_twin.threshold(random_prob)
        c, r = cat[keep], rnd[keep]
        labels[q] = plain
        inputs[q] = np.where(c < tm, mask_token, np.where(c < tr, (r * nchars) >> 16, plain))
    return inputs.reshape(R, P), labels.reshape(R, P), seg, pos, starts, n_rows, n_placed


def as_dtype(a, dt):
    """int64 values as the element type `dt` (bsq_dtype code), converted as the library converts them."""
    t = NP_DTYPES[dt]
    return a.astype(t) if np.dtype(t).kind == "f" else a.astype(np.int64).astype(t)
