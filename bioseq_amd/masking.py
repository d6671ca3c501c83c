"""Masked-LM batches on the device (`bsq_mlm_tokenize_device`, `bsq_random_mask_device`).

The reference's pretraining step (training/cnnpretrain.py:119-124) draws a keep-mask with `torch.rand(...) > maskfrac` and hands it to
`batch_onehot_encode(..., mask=mask)`, which honours only a list there (tokenize.h:294): its "masked" batch is the unmasked one.  Here the
mask is drawn on the device from (seed, row, character index) -- never from padlen, layout, element type, batch size or how a batch is
cut into shards -- and comes in three forms:

* `mlm_tokenize_packed`   BERT's token form: masked inputs (80 % mask token, 10 % a uniform alphabet id, 10 % kept, by default) and the
                          labels for `F.cross_entropy(..., ignore_index=-100)`, one launch;
* `random_mask_packed`    the selection alone as the byte mask `onehot_packed(mask=...)` takes (0 = selected);
* `onehot_masked_packed`  the cnnpretrain.py step done right: the masked one-hot and the labels of the same draw.

The draw is documented in include/bsq.h (`bsq_mlm`).  Every call runs on torch's current stream; inputs are packed batches on the device
(chars uint8[total], offsets int64[B + 1]).
"""
from __future__ import annotations

import ctypes

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


__all__ = ["mlm_tokenize_packed", "random_mask_packed", "onehot_masked_packed"]
