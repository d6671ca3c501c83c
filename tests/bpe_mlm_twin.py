"""An independent statement of the BPE masked-LM draw of include/bsq.h ("BPE masked-LM") in Python integers and numpy, over the ids of
bpe_twin (the one-merge-at-a-time programme).  It calls nothing of the library: the tests hold bsq_bpe_mlm_tokenize_host to it byte for
byte, and the kernels to that."""
import numpy as np

import bpe_twin

MASK64 = (1 << 64) - 1
ROW_DOMAIN = 0x4250454D4C4D534B  # "BPEMLMSK"
GOLDEN = 0x9E3779B97F4A7C15
STEP = 0xD1342543DE82EF95


def mix64(z):
    """splitmix64's finalizer"""
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def threshold(p):
    return int(np.floor(p * 65536.0 + 0.5))


def row_key(seed, row):
    return mix64(((seed & MASK64) ^ ROW_DOMAIN) + GOLDEN * (row + 1))


def draw_row(ids, V, row, frac, mask_prob, random_prob, mask_token, ignore_index, seed):
    """(inputs, labels) of the ids of one row, as Python lists: the row as it would stand without BOS / EOS / PAD and without a cut."""
    h = row_key(seed, row)
    t_frac, t_mask, t_rand = threshold(frac), threshold(mask_prob), threshold(random_prob)
    inputs, labels = [], []
    for j, tok in enumerate(ids):
        w = mix64(h + STEP * ((j >> 2) + 1))
        sel16 = (w >> (16 * (j & 3))) & 0xFFFF
        if tok == V or sel16 >= t_frac:
            inputs.append(tok)
            labels.append(ignore_index)
            continue
        v = mix64((~h & MASK64) + STEP * (j + 1))
        cat16, rnd32 = v & 0xFFFF, (v >> 16) & 0xFFFFFFFF
        inputs.append(mask_token if cat16 < t_mask else ((rnd32 * V) >> 32 if cat16 < t_mask + t_rand else tok))
        labels.append(tok)
    return inputs, labels


def _as(matrix, destchar):
    """int64 values as the element type: two's complement bits for the 64-bit type, the value for every other"""
    dt = bpe_twin.DTYPES[destchar]
    return np.ascontiguousarray(matrix.view(np.uint64) if dt is np.uint64 else matrix.astype(dt))


def tokenize(lut, C, merges, flags, chars, offs, P, destchar="q", batch_first=True, *, label_destchar="q", frac=0.15, mask_prob=0.8,
             random_prob=0.1, mask_token=None, ignore_index=-100, seed=0, first_row=0, max_chars=8192):
    """(inputs, labels, lengths) as the header states them; flags = (eos, bos, padchar) as the Tokenizer constructor orders them."""
    eos, bos, padchar = (int(bool(f)) for f in flags)
    V = C + len(merges)
    bos_id, eos_id, pad_id = V + 1, V + 1 + bos, V + 1 + bos + eos
    mask_token = V + 1 + bos + eos + padchar if mask_token is None else mask_token
    B = len(offs) - 1
    inputs = np.zeros((B, P), np.int64)
    labels = np.full((B, P), ignore_index, np.int64)
    lengths = np.zeros(B, np.int32)
    for b in range(B):
        L = max(int(offs[b + 1] - offs[b]), 0)
        if L > max_chars:
            ids, lengths[b] = [], -1
        else:
            ids = bpe_twin.row_ids(lut, C, merges, chars[offs[b]:offs[b] + L])
            lengths[b] = len(ids)
        ins, labs = draw_row(ids, V, first_row + b, frac, mask_prob, random_prob, mask_token, ignore_index, seed)
        room = max(P - bos - eos, 0)
        ins, labs = ins[:room], labs[:room]
        row = ([bos_id] if bos else []) + ins + ([eos_id] if eos else [])
        inputs[b] = (row + [pad_id if padchar else 0] * P)[:P]
        lab_row = ([ignore_index] if bos else []) + labs
        labels[b] = (lab_row + [ignore_index] * P)[:P]
    if not batch_first:
        inputs, labels = np.ascontiguousarray(inputs.T), np.ascontiguousarray(labels.T)
    return _as(inputs, destchar), _as(labels, label_destchar), lengths
