"""Masked-LM batches on the device (`bsq_mlm_tokenize_device`, `bsq_random_mask_device`).

The reference's pretraining step (training/cnnpretrain.py:119-124) draws a keep-mask with `torch.rand(...) > maskfrac` and hands it to
`batch_onehot_encode(..., mask=mask)`, which honours only a list there (tokenize.h:294): its "masked" batch is the unmasked one.  Here the
mask is drawn on the device from (seed, row, character index) -- never from padlen, layout, element type, batch size or how a batch is
cut into shards -- and comes in three forms:

* `mlm_tokenize_packed`   BERT's token form: masked inputs (80 % mask token, 10 % a uniform alphabet id, 10 % kept, by default) and the
                          labels for `F.cross_entropy(..., ignore_index=-100)`, one launch;
* `random_mask_packed`    the selection alone as the byte mask `onehot_packed(mask=...)` takes (0 = selected);
* `onehot_masked_packed`  the cnnpretrain.py step done right: the masked one-hot and the labels of the same draw.

and, for encoder-decoder models, T5's span corruption (`bsq_span_corrupt_device`; include/bsq.h, "span corruption"):

* `span_corrupt_packed`   encoder inputs with each cut-out run replaced by a sentinel, decoder labels, and both body lengths, one launch;
* `span_corrupt_host`, `span_corrupt_kernel_name`, `span_restore`  its CPU twin, the kernel taken, and the host helper that splices the
                          targets back into the inputs.

The draw is documented in include/bsq.h (`bsq_mlm`).  Every call runs on torch's current stream; inputs are packed batches on the device
(chars uint8[total], offsets int64[B + 1]).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi
from .multi import validate_packed_multi

_lib = capi.load()


def _check_packed(chars, offsets):
    return capi.packed_on_device(chars, offsets, "the masked-LM calls work on packed batches resident on the device (chars, offsets tensors)")


def _params(frac, mask_prob, random_prob, mask_token, ignore_index, seed, first_row):
    """The bsq_mlm struct, with the library's argument rules checked here first (no device is touched for a bad argument)."""
    for name, p in (("frac", frac), ("mask_prob", mask_prob), ("random_prob", random_prob)):
        p = float(p)
        if not 0.0 <= p <= 1.0:
            raise ValueError("%s must lie in [0, 1], got %r" % (name, p))
    if float(mask_prob) + float(random_prob) > 1.0 + 1e-12:
        raise ValueError("mask_prob + random_prob must not exceed 1")
    if int(first_row) < 0:
        raise ValueError("first_row must be >= 0")
    return capi.Mlm(float(frac), float(mask_prob), float(random_prob), int(mask_token), int(ignore_index), int(seed) & (2 ** 64 - 1),
                    int(first_row))


def _launch_mlm(tok, chars, offsets, B, padlen, batch_first, m, in_dt, inputs, label_dt, labels):
    desc = capi.desc_of(tok)
    if B == 0:
        return
    chars = capi.readable_chars(chars, offsets.device)  # (every sequence may be empty)
    with capi.launching(chars.device) as stream:
        capi.check(_lib.bsq_mlm_tokenize_device(ctypes.byref(desc), chars.data_ptr(), offsets.data_ptr(), B, int(padlen), int(bool(batch_first)),
                                                ctypes.byref(m), in_dt, inputs.data_ptr() if inputs is not None else None, label_dt,
                                                labels.data_ptr() if labels is not None else None, stream))


def mlm_tokenize_packed(tok, chars, offsets, padlen, destchar="b", batch_first=True, *, frac=0.15, mask_prob=0.8, random_prob=0.1,
                        mask_token=None, ignore_index=-100, label_dtype="q", seed=0, first_row=0, validate=True):
    """(inputs, labels) of BERT's masked-LM objective for a packed batch on the device, both (B, padlen) when batch_first else (padlen, B).

    A mapped character is selected with probability `frac`; a selected one becomes `mask_token` with probability `mask_prob`, a uniform
    alphabet id with `random_prob`, else stays.  labels = the plain token at selected positions, `ignore_index` elsewhere (BOS / EOS / PAD
    and unmapped characters are never selected).  mask_token=None: `tok.alphabet_size()`, one past the last id (an extra embedding row).
    `destchar` / `label_dtype`: element types as in `tokenize_packed`.  Sequence i is row `first_row + i` of the draw: two halves of a batch
    encoded with first_row = 0 and = their split give the whole batch's result.  validate: the over-long-sequence check of tokenize_packed."""
    import torch
    m = _params(frac, mask_prob, random_prob, tok.alphabet_size() if mask_token is None else mask_token, ignore_index, seed, first_row)
    if int(padlen) <= 0:
        raise ValueError("padlen must be positive")
    (in_dt, in_tdt), (label_dt, label_tdt) = capi.dtype_of(destchar), capi.dtype_of(label_dtype)
    B = _check_packed(chars, offsets)
    if validate and B > 0:
        validate_packed_multi(tok, [(chars, offsets)], int(padlen))
    shape = (B, int(padlen)) if batch_first else (int(padlen), B)
    inputs = torch.empty(shape, dtype=in_tdt, device=chars.device)
    labels = torch.empty(shape, dtype=label_tdt, device=chars.device)
    _launch_mlm(tok, chars, offsets, B, padlen, batch_first, m, in_dt, inputs, label_dt, labels)
    return inputs, labels


def random_mask_packed(tok, chars, offsets, *, frac, seed, first_row=0):
    """uint8[total] device tensor in the packed layout of `chars`: 0 where a character is selected (the draw of `mlm_tokenize_packed`
    with the same tokenizer, frac, seed and first_row), 1 elsewhere -- the `mask=` of `tok.onehot_packed`."""
    import torch
    m = _params(frac, 0.0, 0.0, 0, 0, seed, first_row)
    B = _check_packed(chars, offsets)
    mask = torch.ones(chars.numel(), dtype=torch.uint8, device=chars.device)
    if B > 0 and chars.numel() > 0:
        desc = capi.desc_of(tok)
        with capi.launching(chars.device) as stream:
            capi.check(_lib.bsq_random_mask_device(ctypes.byref(desc), chars.data_ptr(), offsets.data_ptr(), B, ctypes.byref(m), mask.data_ptr(), stream))
    return mask


def onehot_masked_packed(tok, chars, offsets, padlen, destchar="f", layout="bcl", *, frac, seed, first_row=0, label_dtype="q", ignore_index=-100,
                         validate=True):
    """(masked one-hot, labels): `tok.onehot_packed(..., mask=random_mask_packed(...), layout=layout)` -- a selected character's one-hot row
    is all zero -- and the (B, padlen) labels of the same draw (the plain token where the row was zeroed, `ignore_index` elsewhere).  The
    masked-LM step of training/cnnpretrain.py:119-124 with the mask the reference meant to apply."""
    import torch
    m = _params(frac, 0.0, 0.0, 0, ignore_index, seed, first_row)
    if int(padlen) <= 0:
        raise ValueError("padlen must be positive")
    label_dt, label_tdt = capi.dtype_of(label_dtype)
    B = _check_packed(chars, offsets)
    mask = random_mask_packed(tok, chars, offsets, frac=frac, seed=seed, first_row=first_row)
    onehot = tok.onehot_packed(chars, offsets, int(padlen), destchar, mask=mask, validate=validate, layout=layout)
    labels = torch.empty((B, int(padlen)), dtype=label_tdt, device=chars.device)
    _launch_mlm(tok, chars, offsets, B, padlen, True, m, label_dt, None, label_dt, labels)
    return onehot, labels


_NUMPY = {capi.I8: np.int8, capi.I16: np.int16, capi.I32: np.int32, capi.U64: np.uint64, capi.F32: np.float32, capi.F64: np.float64}


def _span_params(tok, destchar, label_dtype, frac, span, anchor_prob, sentinel_first, sentinel_step, max_sentinels, ignore_index, seed, first_row):
    """(desc, bsq_span_corrupt, input dtype, label dtype, torch dtypes) with the library's argument rules applied as ValueError: no
    device is touched for a bad argument."""
    desc = capi.desc_of(tok)
    span = capi.int_arg("span", span, 1, 16)
    max_sentinels = capi.int_arg("max_sentinels", max_sentinels, 1, 65535)
    if sentinel_step not in (1, -1) or isinstance(sentinel_step, bool):
        raise ValueError("sentinel_step must be +1 or -1, got %r" % (sentinel_step,))
    if anchor_prob is None:
        anchor_prob = float(_lib.bsq_kmer_mlm_anchor_prob(float(frac), span))
        if anchor_prob < 0:
            raise ValueError("frac must lie in [0, 1], got %r" % (frac,))
    elif frac != 0.15:
        raise ValueError("give frac or anchor_prob, not both")
    if not 0.0 <= float(anchor_prob) <= 1.0:  # (a NaN fails both comparisons)
        raise ValueError("anchor_prob must lie in [0, 1], got %r" % (anchor_prob,))
    asize = tok.alphabet_size()
    first = asize if sentinel_first is None else capi.int_arg("sentinel_first", sentinel_first)
    last = first + int(sentinel_step) * (max_sentinels - 1)
    lo, hi = min(first, last), max(first, last)
    if lo < 0 or hi >= 2 ** 31:
        raise ValueError("the sentinels %d .. %d leave [0, 2^31)" % (first, last))
    if lo < asize:
        raise ValueError("the sentinels %d .. %d meet the tokenizer's ids [0, %d)" % (first, last, asize))
    if int(first_row) < 0:
        raise ValueError("first_row must be >= 0")
    ignore_index = int(ignore_index)
    try:
        (dt, tdt), (ldt, ltdt) = capi.dtype_of(destchar), capi.dtype_of(label_dtype)
    except RuntimeError as e:
        raise ValueError("bad destchar or label_dtype: %s" % e) from None
    if not _lib.bsq_dtype_holds(dt, 0, hi):
        raise ValueError("destchar %r cannot hold ids up to the largest sentinel %d" % (destchar, hi))
    if not _lib.bsq_dtype_holds(ldt, min(ignore_index, 0), max(ignore_index, hi)):
        raise ValueError("label_dtype %r cannot hold ids up to the largest sentinel %d and ignore_index %d" % (label_dtype, hi, ignore_index))
    m = capi.SpanCorrupt(float(anchor_prob), span, max_sentinels, first, int(sentinel_step), ignore_index, int(seed) & (2 ** 64 - 1), int(first_row))
    return desc, m, dt, ldt, tdt, ltdt


def _span_widths(padlen, target_padlen):
    padlen, target_padlen = int(padlen), int(target_padlen)
    if padlen <= 0 or target_padlen <= 0:
        raise ValueError("padlen and target_padlen must be positive")
    return padlen, target_padlen


def span_corrupt_kernel_name(tok, B, padlen, target_padlen, destchar="q", *, label_dtype="q", sentinel_first=None, sentinel_step=1, max_sentinels=100,
                             ignore_index=-100):
    """The kernel `span_corrupt_packed` takes (host only: profiling labels, tests); a call it would refuse is a ValueError here too."""
    desc, m, dt, ldt, _, _ = _span_params(tok, destchar, label_dtype, 0.15, 3, None, sentinel_first, sentinel_step, max_sentinels, ignore_index, 0, 0)
    padlen, target_padlen = _span_widths(padlen, target_padlen)
    return _lib.bsq_span_corrupt_kernel_name(ctypes.byref(desc), ctypes.byref(m), int(B), padlen, target_padlen, dt, ldt).decode()


def span_corrupt_host(tok, chars, offsets, padlen, target_padlen, destchar="q", *, label_dtype="q", frac=0.15, span=3, anchor_prob=None,
                      sentinel_first=None, sentinel_step=1, max_sentinels=100, ignore_index=-100, seed=0, first_row=0):
    """The library's CPU twin (`bsq_span_corrupt_host`, the lane code of the kernel) on numpy arrays: (inputs, labels, in_len, tgt_len)."""
    desc, m, dt, ldt, _, _ = _span_params(tok, destchar, label_dtype, frac, span, anchor_prob, sentinel_first, sentinel_step, max_sentinels,
                                          ignore_index, seed, first_row)
    padlen, target_padlen = _span_widths(padlen, target_padlen)
    chars, offsets = capi.host_batch(chars, offsets)
    B = offsets.size - 1
    inputs, labels = np.empty((B, padlen), dtype=_NUMPY[dt]), np.empty((B, target_padlen), dtype=_NUMPY[ldt])
    in_len, tgt_len = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
    if B > 0:
        capi.check(_lib.bsq_span_corrupt_host(ctypes.byref(desc), chars.ctypes.data, offsets.ctypes.data, B, padlen, target_padlen, ctypes.byref(m),
                                              dt, inputs.ctypes.data, ldt, labels.ctypes.data, in_len.ctypes.data, tgt_len.ctypes.data))
    return inputs, labels, in_len, tgt_len


def span_corrupt_packed(tok, chars, offsets, padlen, target_padlen, destchar="q", *, label_dtype="q", frac=0.15, span=3, anchor_prob=None,
                        sentinel_first=None, sentinel_step=1, max_sentinels=100, ignore_index=-100, seed=0, first_row=0, validate=True):
    """(inputs, labels, in_len, tgt_len) of T5's span-corruption objective for a packed batch on the device, one launch on torch's current
    stream (`bsq_span_corrupt_device`; include/bsq.h, "span corruption", has the rule).

    Anchors open spans of `span` characters; every maximal run of covered, mapped characters is cut out of the encoder inputs (B, padlen)
    and replaced by one sentinel -- sentinel_first (None: `tok.alphabet_size()`), then sentinel_first + sentinel_step, ... -- and the
    decoder labels (B, target_padlen) hold each sentinel followed by the tokens it stands for, [EOS] when the tokenizer has one, then
    ignore_index.  Only the first `max_sentinels` runs of a row are cut out.  `frac` is the share of a long row that is covered
    (`anchor_prob` = 1 - (1 - frac) ** (1 / span)); give `anchor_prob` to set the anchor rate itself -- both is a ValueError.  in_len,
    tgt_len: int32 (B), the body lengths BEFORE the cut at the widths, which the call never reads back: in_len > padlen - bos - eos or
    tgt_len > target_padlen - eos marks a cut row.  validate: the over-long check of `tokenize_packed` on the UNCORRUPTED rows against
    padlen -- sufficient for the inputs (a corrupted row is never longer), silent about the labels.  A character's fate depends on
    (seed, first_row + its row, its index, span, the rate, max_sentinels) and its row's characters only."""
    import torch
    desc, m, dt, ldt, tdt, ltdt = _span_params(tok, destchar, label_dtype, frac, span, anchor_prob, sentinel_first, sentinel_step, max_sentinels,
                                               ignore_index, seed, first_row)
    padlen, target_padlen = _span_widths(padlen, target_padlen)
    B = capi.packed_on_device(chars, offsets, "span_corrupt_packed works on packed batches resident on the device (chars, offsets tensors)")
    if validate and B > 0:
        validate_packed_multi(tok, [(chars, offsets)], padlen)
    dev = chars.device
    inputs = torch.empty((B, padlen), dtype=tdt, device=dev)
    labels = torch.empty((B, target_padlen), dtype=ltdt, device=dev)
    in_len = torch.empty(B, dtype=torch.int32, device=dev)
    tgt_len = torch.empty(B, dtype=torch.int32, device=dev)
    if B > 0:
        src = capi.readable_chars(chars, offsets.device)  # (every sequence may be empty)
        with capi.launching(src.device) as stream:
            capi.check(_lib.bsq_span_corrupt_device(ctypes.byref(desc), src.data_ptr(), offsets.data_ptr(), B, padlen, target_padlen, ctypes.byref(m),
                                                    dt, inputs.data_ptr(), ldt, labels.data_ptr(), in_len.data_ptr(), tgt_len.data_ptr(), stream))
    return inputs, labels, in_len, tgt_len


def span_restore(inputs, labels, tok, *, in_len=None, sentinel_first=None, sentinel_step=1, max_sentinels=100, ignore_index=-100):
    """The plain bodies of UNCUT span-corruption rows, as a list of int64 numpy arrays: the targets spliced back into the inputs at their
    sentinels, BOS / EOS / PAD taken off.  inputs, labels: (B, padlen), (B, target_padlen) numpy arrays (or anything `np.asarray`
    takes); a small host helper for tests and for looking at a data pipeline, not a device call.  A row whose inputs or labels were cut
    at their width cannot be restored: ValueError when an input sentinel has no target.  in_len (the call's third result) ends the
    input body where it is given; without it the body ends at [EOS], or, for a tokenizer without one, in front of the trailing pad ids."""
    inputs, labels = np.asarray(inputs).astype(np.int64), np.asarray(labels).astype(np.int64)
    first = tok.alphabet_size() if sentinel_first is None else int(sentinel_first)
    step = int(sentinel_step)
    index = {first + g * step: g for g in range(int(max_sentinels))}
    desc = capi.desc_of(tok)
    bos, eos = int(bool(desc.bos)), int(bool(desc.eos))
    eos_id = desc.nchars + bos if eos else None
    pad_id = desc.nchars + bos + eos if desc.padchar else 0  # (what bsq_tokenize_device stores at a pad position)
    out = []
    for r, (row, lab) in enumerate(zip(inputs, labels)):
        gaps, cur = {}, None
        for v in lab.tolist():
            if v == ignore_index or (eos and v == eos_id):
                break
            if v in index:
                cur = gaps.setdefault(index[v], [])
            elif cur is None:
                raise ValueError("a label row does not open with a sentinel")
            else:
                cur.append(v)
        body = row.tolist()[bos:]
        if in_len is not None:
            if int(in_len[r]) > len(body) - eos:
                raise ValueError("in_len says that an input row was cut")
            body = body[:int(in_len[r])]
        elif eos:
            if eos_id not in body:
                raise ValueError("an input row has no EOS: it was cut")
            body = body[:body.index(eos_id)]
        else:  # (without EOS the pad tail is told from the body only by its value: trailing pad ids are taken off)
            while body and body[-1] == pad_id:
                body.pop()
        plain = []
        for v in body:
            if v in index:
                if index[v] not in gaps:
                    raise ValueError("an input sentinel has no target: the label row was cut")
                plain.extend(gaps[index[v]])
            else:
                plain.append(v)
        out.append(np.asarray(plain, dtype=np.int64))
    return out


__all__ = ["mlm_tokenize_packed", "random_mask_packed", "onehot_masked_packed", "span_corrupt_packed", "span_corrupt_host",
           "span_corrupt_kernel_name", "span_restore"]
