"""Several independent packed batches per call (round 6; `bsq_tokenize_device_multi`, `bsq_augment_tokenize_device_multi`, `bsq_onehot_device_multi`).

The reference encodes one batch per call and its training loop issues the calls back to back (/root/reference/bioseq/loaders.py:76-104;
`Tokenizer::transencode`, src/tokenize.h:451-479, is one OpenMP region per batch).  On the GPU a 16-40-us token launch pays its own ramp-up
and drain, and on one in-order stream the next batch cannot start under the tail of this one; a caller that has its next batches at hand
passes them together and gets ONE launch (two with augmentation) for up to eight of them.  Results are bit for bit those of the per-batch
calls `tok.tokenize_packed(...)` / `blosum.augment_tokenize_packed(...)` with the same seeds.  `onehot_packed_multi` does the same for the
one-hot: the batches whose single calls take the chunk-owner kernel share one launch, the one-piece two-pass batches one raw-id launch and
one expansion launch, the (B,C,P) chunk-stream batches one launch; every other batch is its single call."""
from __future__ import annotations

import ctypes

from . import capi

_RESIDENT = "the multi-batch calls work on packed batches resident on the device (chars, offsets tensors)"
_ONE_DEVICE = "every batch of a multi-batch call lives on one device"


def _convert(batches):
    """The batches as the C ABI reads them -- contiguous uint8 characters and contiguous int64 offsets on one device -- converted ONCE, before
    both the validation and the launch read them (validating int32 or strided offsets as raw int64 words would check garbage)."""
    import torch
    out, dev = [], None
    for chars, offsets in batches:
        capi.packed_on_device(chars, offsets, _RESIDENT, exact=False, apart=_ONE_DEVICE)
        if dev is None:
            dev = chars.device
        if chars.device != dev:
            raise ValueError(_ONE_DEVICE)
        out.append((chars.contiguous(), offsets.to(torch.int64).contiguous()))
    return out


def _prepare(tokenizer, batches, padlen, destchar, batch_first, outs, onehot=False):
    """batches: the output of _convert.  onehot: the table is of bsq_onehot_batch and the results are (padlen, B, C) / (B, C, padlen)."""
    import torch
    lib = capi.load()
    desc = capi.desc_of(tokenizer)
    dt, tdt = capi.dtype_of(destchar)
    n = len(batches)
    arr = ((capi.OnehotBatch if onehot else capi.Batch) * max(n, 1))()
    results, keep = [], []
    dev = batches[0][0].device if batches else None
    C = lib.bsq_alphabet_size(ctypes.byref(desc))
    for i, (chars, offsets) in enumerate(batches):
        B = int(offsets.shape[0]) - 1
        if onehot:
            shape = (B, C, padlen) if batch_first else (padlen, B, C)
        else:
            shape = (B, padlen) if batch_first else (padlen, B)
        if outs is not None:
            out = outs[i]
            if tuple(out.shape) != shape or out.dtype != tdt or not out.is_contiguous() or out.device != dev:
                raise ValueError("outs[%d] must be a contiguous %s tensor of shape %r on %s" % (i, tdt, shape, dev))
        else:
            out = torch.empty(shape, dtype=tdt, device=dev)
        if B > 0:
            chars = capi.readable_chars(chars, dev)  # (every sequence of this batch may be empty)
        keep.append((chars, offsets))
        results.append(out)
        arr[i].chars, arr[i].offsets, arr[i].B, arr[i].out = chars.data_ptr(), offsets.data_ptr(), B, out.data_ptr()
    return lib, desc, dt, arr, results, keep, dev


def validate_packed_multi(tokenizer, batches, padlen):
    """The reference's over-long-sequence error for every batch (one synchronising check per batch: `tokenize_packed(validate=True)`'s).
    batches: the output of _convert (the offsets are read as contiguous int64)."""
    lib = capi.load()
    desc = capi.desc_of(tokenizer)
    for chars, offsets in batches:
        B = int(offsets.shape[0]) - 1
        if B <= 0:
            continue
        bad = ctypes.c_int64(-1)
        with capi.launching(chars.device) as stream:
            st = lib.bsq_validate_packed_device(offsets.data_ptr(), B, padlen, desc.bos, desc.eos, chars.numel(), ctypes.byref(bad), stream)
        if st == capi.ERR_SEQ_TOO_LONG:  # the reference's error of batch_tokenize (tokenize.h:456-459), as tokenize_packed raises it
            i = int(bad.value)
            capi.raise_too_long(tokenizer, int(offsets[i + 1] - offsets[i]), padlen, False)
        capi.check(st)


def tokenize_packed_multi(tokenizer, batches, padlen, destchar="B", batch_first=False, outs=None, validate=True):
    """`[tokenizer.tokenize_packed(c, o, padlen, destchar, batch_first) for c, o in batches]` in ceil(n / 8) launches.
    batches: list of (chars uint8, offsets int64) device tensors; returns the list of token matrices ((B_i, padlen) or (padlen, B_i))."""
    batches = _convert(batches)
    if validate:
        validate_packed_multi(tokenizer, batches, padlen)
    lib, desc, dt, arr, results, keep, dev = _prepare(tokenizer, batches, padlen, destchar, batch_first, outs)
    if batches:
        with capi.launching(dev) as stream:
            capi.check(lib.bsq_tokenize_device_multi(ctypes.byref(desc), len(batches), arr, padlen, int(batch_first), dt, stream))
    return results


def augment_tokenize_packed_multi(tokenizer, batches, padlen, destchar="b", batch_first=True, chain_len=1, augment_frac=1.0, seeds=None, outs=None,
                                  validate=True):
    """`[blosum.augment_tokenize_packed(tokenizer, c, o, padlen, destchar, batch_first, chain_len, augment_frac, seed) for ...]`: every batch's
    characters are mutated in place (BLOSUM62 point substitutions, `seeds[i]` is batch i's seed), the token matrices of the mutated batches
    come back -- two launches for up to eight batches instead of one or two per batch."""
    n = len(batches)
    seeds = list(range(n)) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != n:
        raise ValueError("one seed per batch")
    batches = _convert(batches)
    if validate:
        validate_packed_multi(tokenizer, batches, padlen)
    lib, desc, dt, arr, results, keep, dev = _prepare(tokenizer, batches, padlen, destchar, batch_first, outs)
    if batches:
        sd = (ctypes.c_uint64 * n)(*[s & ((1 << 64) - 1) for s in seeds])
        with capi.launching(dev) as stream:
            capi.check(lib.bsq_augment_tokenize_device_multi(ctypes.byref(desc), n, arr, padlen, int(batch_first), dt, int(chain_len), float(augment_frac),
                                                             sd, stream))
    return results


def onehot_packed_multi(tokenizer, batches, padlen, destchar="B", layout="tbc", masks=None, outs=None, validate=True):
    """`[tokenizer.onehot_packed(c, o, padlen, destchar, mask=m, layout=layout) for (c, o), m in zip(batches, masks)]` in a bounded number of
    launches (`bsq_onehot_device_multi`).  batches: list of (chars uint8, offsets) device tensors; masks: None, or a list of None / uint8 device
    tensors of chars_i.numel() bytes (0 = masked, as `onehot_packed(mask=...)`); layout "tbc" -> (padlen, B_i, C), "bcl" -> (B_i, C, padlen)."""
    import torch
    bcl = capi.parse_layout(layout)
    n = len(batches)
    masks = [None] * n if masks is None else list(masks)
    if len(masks) != n:
        raise ValueError("one mask (or None) per batch")
    batches = _convert(batches)
    for i, m in enumerate(masks):
        if m is None:
            continue
        chars = batches[i][0]
        if not (isinstance(m, torch.Tensor) and m.dtype == torch.uint8 and m.numel() == chars.numel() and m.device == chars.device):
            raise ValueError("masks[%d] must be a uint8 tensor of %d bytes on %s" % (i, chars.numel(), chars.device))
        masks[i] = m.contiguous()
    if validate:
        validate_packed_multi(tokenizer, batches, padlen)
    lib, desc, dt, arr, results, keep, dev = _prepare(tokenizer, batches, padlen, destchar, bcl, outs, onehot=True)
    for i, m in enumerate(masks):
        arr[i].mask = m.data_ptr() if m is not None and m.numel() > 0 else None
    if batches:
        with capi.launching(dev) as stream:
            capi.check(lib.bsq_onehot_device_multi(ctypes.byref(desc), n, arr, padlen, int(bcl), dt, stream))
    return results
