"""An independent restatement of the span-corruption rule of include/bsq.h ("span corruption"), from the header's text: a loop over a
row's positions in plain Python integers -- no tiles, no lanes, no masks, no scans.  The host and GPU tests compare the library's C twin
and kernel with it bit for bit, and read from its `details` whether a batch really holds the case a test is named for."""
import math

import numpy as np

M64 = (1 << 64) - 1


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def threshold(p):
    return int(math.floor(p * 65536 + 0.5))


def corrupt_row(lut, seq, row, *, anchor_prob, span, max_sentinels, sentinel_first, sentinel_step, seed):
    """(input body, target body, details) of one row.  lut: 256 ids (negative: unmapped); seq: the row's bytes.
    details: runs = [(first position, length)] of every maximal run of cand positions, selected or not; cand and anchors per position."""
    t_anchor = threshold(anchor_prob)
    h_row = mix64(((seed ^ 0x5350414E43525054) + 0x9E3779B97F4A7C15 * (row + 1)) & M64)
    words = {}

    def anchor(a):
        if a < 0:
            return False
        q = a >> 2
        if q not in words:
            words[q] = mix64((h_row + 0xD1342543DE82EF95 * (q + 1)) & M64)
        return ((words[q] >> (16 * (a & 3))) & 0xFFFF) < t_anchor

    L = len(seq)
    cand = [any(anchor(a) for a in range(max(0, j - span + 1), j + 1)) and lut[seq[j]] >= 0 for j in range(L)]
    body_in, body_tgt, runs = [], [], []
    g = -1
    for j in range(L):
        tok = lut[seq[j]] if lut[seq[j]] >= 0 else 0  # (bsq_tokenize_device stores 0 for an unmapped byte)
        if cand[j]:
            opens = j == 0 or not cand[j - 1]
            if opens:
                g += 1
                runs.append([j, 0])
            runs[-1][1] += 1
            if g < max_sentinels:
                if opens:
                    s = sentinel_first + g * sentinel_step
                    body_in.append(s)
                    body_tgt.append(s)
                body_tgt.append(tok)
                continue
        body_in.append(tok)
    return body_in, body_tgt, {"runs": [tuple(r) for r in runs], "cand": cand, "anchors": [anchor(a) for a in range(L)]}


def corrupt_batch(desc, chars, offsets, P_in, P_tgt, *, anchor_prob, span=3, max_sentinels=100, sentinel_first=None, sentinel_step=1,
                  ignore_index=-100, seed=0, first_row=0):
    """(inputs int64 (B, P_in), labels int64 (B, P_tgt), in_len, tgt_len, details per row).  desc: a capi.Desc (table and flags)."""
    lut = [int(v) for v in desc.lut]
    bos, eos = int(bool(desc.bos)), int(bool(desc.eos))
    bos_id, eos_id = desc.nchars, desc.nchars + bos
    pad = desc.nchars + bos + eos if desc.padchar else 0  # (what bsq_tokenize_device stores at a pad position)
    if sentinel_first is None:
        sentinel_first = desc.nchars + bos + eos + int(bool(desc.padchar))
    chars = np.asarray(chars, dtype=np.uint8)
    B = len(offsets) - 1
    inputs, labels = np.empty((B, P_in), np.int64), np.empty((B, P_tgt), np.int64)
    in_len, tgt_len, details = np.empty(B, np.int32), np.empty(B, np.int32), []
    for b in range(B):
        seq = chars[int(offsets[b]):max(int(offsets[b + 1]), int(offsets[b]))].tolist()
        bi, bt, det = corrupt_row(lut, seq, first_row + b, anchor_prob=anchor_prob, span=span, max_sentinels=max_sentinels,
                                  sentinel_first=sentinel_first, sentinel_step=sentinel_step, seed=seed)
        in_len[b], tgt_len[b] = len(bi), len(bt)
        row = [bos_id] * bos + bi[:min(len(bi), max(P_in - bos - eos, 0))] + [eos_id] * eos
        inputs[b] = (row + [pad] * P_in)[:P_in]
        row = bt[:min(len(bt), max(P_tgt - eos, 0))] + [eos_id] * eos
        labels[b] = (row + [ignore_index] * P_tgt)[:P_tgt]
        det["in_body"], det["tgt_body"] = bi, bt
        details.append(det)
    return inputs, labels, in_len, tgt_len, details


def as_int64(a):
    """A result matrix as int64 values: 'q' results are uint64 in numpy (the bits of the int64), the float types hold exact integers."""
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.uint64 else a.astype(np.int64)
