"""Sequence packing on the device (`bsq_pack_plan_device`, `bsq_pack_tokenize_device`): several sequences per token row.

Every other encode path of the package writes one sequence per row and fills the rest with PAD.  A transformer pays for every
position of the matrix; at protein-like or read-like length distributions most of them are PAD.  Here the runs `[BOS] tokens [EOS]`
of a packed batch are laid out back to back in a (rows, padlen) matrix, with the segment ids and position ids that keep attention
and position embeddings per sequence -- the plan on the device, the encode in ONE launch, instead of a padded `tokenize_packed`, a
boolean-mask gather, a scatter and `cumsum` / `repeat_interleave` in torch over a matrix 2-6x larger than the result.

mode "nextfit": whole sequences share a row (the plain sequential loop: a run goes into the current row if it still fits, else it
opens the next one); mode "stream": the GPT-style concatenation of all runs, cut every `padlen` tokens.  include/bsq.h ("sequence
packing") has the full rules.

* `pack_tokenize_packed`  tokens, segment_ids, position_ids, starts and n_rows of a packed batch resident on the device;
* `pack_plan`             starts and row count alone;
* `pack_rows_bound`       a safe `rows=` from the sizes of a batch, with no device work;
* `pack_cu_seqlens`       int32 sequence boundaries for varlen attention (stream mode);
* `pack_mlm_tokenize_packed`  the masked-LM form of a packed batch (`bsq_pack_mlm_tokenize_device`): masked inputs, labels, segment_ids,
                          position_ids in one launch, the draw of `masking.mlm_tokenize_packed` per sequence;
* `pack_plan_host`, `pack_tokenize_host`, `pack_mlm_tokenize_host`  the library's CPU twins (numpy in, numpy out; no device).

The crops and reverse-complement views of `views` hand this module packed batches as they are.
"""
from __future__ import annotations

import collections
import ctypes

import numpy as np

from . import capi
from .masking import _params as _mlm_params

_lib = capi.load()

_NUMPY = {capi.I8: np.int8, capi.I16: np.int16, capi.I32: np.int32, capi.U64: np.uint64, capi.F32: np.float32, capi.F64: np.float64}
_MODES = {"stream": capi.PACK_STREAM, "nextfit": capi.PACK_NEXTFIT}

Packed = collections.namedtuple("Packed", "tokens segment_ids position_ids starts n_rows")
Packed.__doc__ = """Result of `pack_tokenize_packed`: tokens (rows, padlen); segment_ids, position_ids int32 of the same shape (None when
not requested); starts int64[B + 1]; n_rows (0-d int64 tensor on the device, an int from the host twin)."""
PackedRows = collections.namedtuple("PackedRows", "tokens segment_ids position_ids starts n_rows n_placed")
PackedRows.__doc__ = """`Packed` of a call with `rows=N`, plus n_placed: how many sequences of the batch were placed."""

PackedMlm = collections.namedtuple("PackedMlm", "inputs labels segment_ids position_ids starts n_rows")
PackedMlm.__doc__ = """Result of `pack_mlm_tokenize_packed`: masked inputs and labels (rows, padlen); segment_ids, position_ids int32 of the same
shape (None when not requested); starts int64[B + 1]; n_rows (0-d int64 tensor on the device, an int from the host twin)."""
PackedMlmRows = collections.namedtuple("PackedMlmRows", "inputs labels segment_ids position_ids starts n_rows n_placed")
PackedMlmRows.__doc__ = """`PackedMlm` of a call with `rows=N`, plus n_placed: how many sequences of the batch were placed."""


def _args(tok, padlen, mode, rows=None):
    """(desc, mode code, padlen, rows) with the argument rules applied: ValueError before any device work."""
    if mode not in _MODES:
        raise ValueError("mode must be 'nextfit' or 'stream', got %r" % (mode,))
    padlen = int(padlen)
    if padlen <= 0:
        raise ValueError("padlen must be positive")
    if padlen > 2 ** 30:
        raise ValueError("padlen > 2**30 is not supported")
    if rows is not None:
        rows = int(rows)
        if rows <= 0 or rows > 2 ** 31:
            raise ValueError("rows must be a positive number of rows (at most 2**31), got %r" % (rows,))
    return capi.desc_of(tok), _MODES[mode], padlen, rows


def pack_rows_bound(total_chars, B, padlen, tok, mode="nextfit"):
    """Rows that hold ANY batch of `B` sequences with `total_chars` characters in all, whose runs each fit a row: a safe `rows=` with no
    device work.  stream: ceil(tokens / padlen).  nextfit: two consecutive rows together hold more than `padlen` tokens (the run that
    opened the second did not fit the first), so rows <= 2 * tokens / padlen + 1; never more than B."""
    _, code, padlen, _ = _args(tok, padlen, mode)
    B, total_chars = int(B), int(total_chars)
    if B < 0 or total_chars < 0:
        raise ValueError("B and total_chars must not be negative")
    if B == 0:
        return 0
    tokens = total_chars + B * (int(tok.includes_bos()) + int(tok.includes_eos()))
    if code == capi.PACK_STREAM:
        return max(1, -(-tokens // padlen))
    return max(1, min(B, 2 * tokens // padlen + 1))


def pack_cu_seqlens(starts):
    """int32 boundaries of the sequences in the flat token stream, as varlen attention kernels take them (`cu_seqlens`): starts[0 .. B]
    of a stream-mode plan as int32.  (Next-fit rows have PAD gaps between rows: use the segment ids there.)"""
    import torch
    if isinstance(starts, torch.Tensor):
        return starts.to(torch.int32)
    return np.asarray(starts).astype(np.int32)


def pack_kernel_name(tok, B, rows, padlen, destchar="q"):
    """The kernel `pack_tokenize_packed` takes (host only: profiling labels, tests)."""
    dt, _ = capi.dtype_of(destchar)
    desc = capi.desc_of(tok)
    return _lib.bsq_pack_kernel_name(ctypes.byref(desc), int(B), int(rows), int(padlen), dt).decode()


def pack_mlm_kernel_name(tok, B, rows, padlen, destchar="q"):
    """The kernel `pack_mlm_tokenize_packed` takes (host only: profiling labels, tests)."""
    dt, _ = capi.dtype_of(destchar)
    desc = capi.desc_of(tok)
    return _lib.bsq_pack_mlm_kernel_name(ctypes.byref(desc), int(B), int(rows), int(padlen), dt).decode()


def _host_offsets(offsets):
    offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    if offsets.ndim != 1 or offsets.size < 1:
        raise ValueError("offsets must hold B + 1 entries")
    return offsets


def pack_plan_host(tok, offsets, padlen, mode="nextfit", rows=None, *, parallel=False):
    """The plan on the CPU (`bsq_pack_plan_host`: the plain sequential loop): (starts int64[B + 1], n_rows, n_placed).
    parallel=True runs the device plan's own arithmetic round by round instead (`bsq_pack_plan_parallel_host`)."""
    desc, code, padlen, rows = _args(tok, padlen, mode, rows)
    offsets = _host_offsets(offsets)
    B = offsets.size - 1
    starts = np.empty(B + 1, dtype=np.int64)
    n_rows, n_placed = ctypes.c_int64(0), ctypes.c_int64(0)
    fn = _lib.bsq_pack_plan_parallel_host if parallel else _lib.bsq_pack_plan_host
    capi.check(fn(offsets.ctypes.data, B, padlen, desc.bos, desc.eos, code, rows or 0, starts.ctypes.data, ctypes.addressof(n_rows),
                  ctypes.addressof(n_placed)))
    return starts, int(n_rows.value), int(n_placed.value)


def pack_tokenize_host(tok, chars, offsets, padlen, destchar="q", *, mode="nextfit", rows=None, segment_ids=True, position_ids=True):
    """The library's CPU twin of `pack_tokenize_packed` on numpy arrays: the same named tuple, of numpy arrays and Python ints."""
    desc, code, padlen, rows = _args(tok, padlen, mode, rows)
    dt, _ = capi.dtype_of(destchar)
    chars, offsets = capi.host_batch(chars, _host_offsets(offsets))
    B = offsets.size - 1
    starts, n_rows, n_placed = pack_plan_host(tok, offsets, padlen, mode, rows)
    R = n_rows if rows is None else rows
    tokens = np.empty((R, padlen), dtype=_NUMPY[dt])
    seg = np.empty((R, padlen), dtype=np.int32) if segment_ids else None
    pos = np.empty((R, padlen), dtype=np.int32) if position_ids else None
    if R > 0:
        capi.check(_lib.bsq_pack_tokenize_host(ctypes.byref(desc), chars.ctypes.data, offsets.ctypes.data, B, starts.ctypes.data, R, padlen, dt,
                                               tokens.ctypes.data, seg.ctypes.data if segment_ids else None,
                                               pos.ctypes.data if position_ids else None))
    if rows is None:
        return Packed(tokens, seg, pos, starts, n_rows)
    return PackedRows(tokens, seg, pos, starts, n_rows, n_placed)


def pack_mlm_tokenize_host(tok, chars, offsets, padlen, destchar="q", *, mode="nextfit", rows=None, frac=0.15, mask_prob=0.8, random_prob=0.1,
                           mask_token=None, ignore_index=-100, label_dtype="q", seed=0, first_row=0, segment_ids=True, position_ids=True):
    """The library's CPU twin of `pack_mlm_tokenize_packed` on numpy arrays: the same named tuple, of numpy arrays and Python ints."""
    desc, code, padlen, rows = _args(tok, padlen, mode, rows)
    m = _mlm_params(frac, mask_prob, random_prob, tok.alphabet_size() if mask_token is None else mask_token, ignore_index, seed, first_row)
    (dt, _), (ldt, _) = capi.dtype_of(destchar), capi.dtype_of(label_dtype)
    chars, offsets = capi.host_batch(chars, _host_offsets(offsets))
    B = offsets.size - 1
    starts, n_rows, n_placed = pack_plan_host(tok, offsets, padlen, mode, rows)
    R = n_rows if rows is None else rows
    pad = tok.pad() if tok.is_padded() else 0
    # (the entry writes nothing for a batch without sequences: such a matrix is all PAD / ignore_index / 0 / 0)
    inputs = np.full((R, padlen), pad, dtype=_NUMPY[dt])
    labels = np.full((R, padlen), np.int64(ignore_index)).astype(_NUMPY[ldt])
    seg = np.zeros((R, padlen), dtype=np.int32) if segment_ids else None
    pos = np.zeros((R, padlen), dtype=np.int32) if position_ids else None
    if R > 0 and B > 0:
        capi.check(_lib.bsq_pack_mlm_tokenize_host(ctypes.byref(desc), chars.ctypes.data, offsets.ctypes.data, B, starts.ctypes.data, R, padlen,
                                                   ctypes.byref(m), dt, inputs.ctypes.data, ldt, labels.ctypes.data,
                                                   seg.ctypes.data if segment_ids else None, pos.ctypes.data if position_ids else None))
    if rows is None:
        return PackedMlm(inputs, labels, seg, pos, starts, n_rows)
    return PackedMlmRows(inputs, labels, seg, pos, starts, n_rows, n_placed)


def _validate(chars, offsets, B, desc, code, padlen):
    """Well-formed offsets in both modes; in next-fit mode also every run within a row (`bsq_validate_packed_device`, one read-back)."""
    bad = ctypes.c_int64(-1)
    nextfit = code == capi.PACK_NEXTFIT
    with capi.launching(chars.device) as stream:
        st = _lib.bsq_validate_packed_device(offsets.data_ptr(), B, padlen if nextfit else 2 ** 62, desc.bos if nextfit else 0,
                                             desc.eos if nextfit else 0, chars.numel(), ctypes.byref(bad), stream)
    if st == capi.ERR_SEQ_TOO_LONG:
        i = int(bad.value)
        raise RuntimeError("sequence %d: seq len + bos + eos > padlen: %d, vs padlen %d (a next-fit row holds whole sequences)"
                           % (i, int(offsets[i + 1] - offsets[i]) + desc.bos + desc.eos, padlen))
    if st == capi.ERR_INVALID_ARG:
        raise RuntimeError("malformed offsets at entry %d: %s" % (int(bad.value), _lib.bsq_last_error().decode()))
    capi.check(st)


def _plan(offsets, B, desc, code, padlen, rows):
    import torch
    starts = torch.empty(B + 1, dtype=torch.int64, device=offsets.device)
    counts = torch.empty(2, dtype=torch.int64, device=offsets.device)  # n_rows, n_placed
    with capi.launching(offsets.device) as stream:
        capi.check(_lib.bsq_pack_plan_device(offsets.data_ptr(), B, padlen, desc.bos, desc.eos, code, rows or 0, starts.data_ptr(),
                                             counts.data_ptr(), counts.data_ptr() + 8, stream))
    return starts, counts[0], counts[1]


def pack_plan(tok, chars, offsets, padlen, *, mode="nextfit", rows=None, validate=True):
    """The plan of a packed batch resident on the device, without encoding: (starts int64[B + 1], n_rows, n_placed), device tensors
    (the two counts are 0-d).  Stream-ordered; nothing is read back unless `validate` (its check reads 8 bytes back)."""
    desc, code, padlen, rows = _args(tok, padlen, mode, rows)
    B = capi.packed_on_device(chars, offsets, "pack_plan works on packed batches resident on the device (chars, offsets tensors)")
    if validate and B > 0:
        _validate(chars, offsets, B, desc, code, padlen)
    return _plan(offsets, B, desc, code, padlen, rows)


def pack_tokenize_packed(tok, chars, offsets, padlen, destchar="q", *, mode="nextfit", rows=None, segment_ids=True, position_ids=True,
                         validate=True):
    """Pack a batch resident on the device (chars uint8[total], offsets int64[B + 1]) into a (rows, padlen) token matrix with several
    sequences per row: the named tuple (tokens, segment_ids, position_ids, starts, n_rows), all on the device, on torch's current stream.

    tokens        flat[starts[i] : starts[i] + w_i] = [BOS] tokens [EOS] of sequence i; PAD (0 for an unpadded tokenizer) elsewhere
    segment_ids   int32, 0 at PAD, else 1 + (sequence index - index of the sequence at column 0 of the row); None if not requested
    position_ids  int32, the index of the token inside its sequence's run (continues across a row cut in stream mode), 0 at PAD
    starts        int64[B + 1], the flat position of every run; starts[B] = the end of the last run
    n_rows        0-d int64 tensor: the rows the batch needs

    rows=None: the call reads the 8 bytes of n_rows back to size the outputs -- the ONE synchronisation of the call (besides the
    read-back of `validate`, as everywhere in the package).  rows=N: nothing is read back; the outputs have N rows, rows from n_rows on
    are all PAD; if the batch needs more than N rows only the prefix of sequences whose runs end inside the matrix is placed, the
    result carries a sixth field `n_placed` (0-d device tensor: resume there) and `starts` of the others is -1.  `pack_rows_bound`
    gives an N that always suffices.

    validate: malformed offsets raise; in next-fit mode a sequence whose run is wider than padlen raises, naming the sequence
    (without validation it gets a row of its own and is cut at padlen, memory-safe).  Argument errors raise ValueError before any
    device work."""
    import torch
    desc, code, padlen, rows = _args(tok, padlen, mode, rows)
    dt, tdt = capi.dtype_of(destchar)
    B = capi.packed_on_device(chars, offsets, "pack_tokenize_packed works on packed batches resident on the device (chars, offsets tensors)")
    if validate and B > 0:
        _validate(chars, offsets, B, desc, code, padlen)
    starts, n_rows, n_placed = _plan(offsets, B, desc, code, padlen, rows)
    R = int(n_rows) if rows is None else rows  # (rows=None: the one read-back)
    dev = offsets.device
    tokens = torch.empty((R, padlen), dtype=tdt, device=dev)
    seg = torch.empty((R, padlen), dtype=torch.int32, device=dev) if segment_ids else None
    pos = torch.empty((R, padlen), dtype=torch.int32, device=dev) if position_ids else None
    if R > 0:
        src = capi.readable_chars(chars, dev)
        with capi.launching(dev) as stream:
            capi.check(_lib.bsq_pack_tokenize_device(ctypes.byref(desc), src.data_ptr(), offsets.data_ptr(), B, starts.data_ptr(), R, padlen, dt,
                                                     tokens.data_ptr(), seg.data_ptr() if segment_ids else None,
                                                     pos.data_ptr() if position_ids else None, stream))
    if rows is None:
        return Packed(tokens, seg, pos, starts, n_rows)
    return PackedRows(tokens, seg, pos, starts, n_rows, n_placed)


def pack_mlm_tokenize_packed(tok, chars, offsets, padlen, destchar="q", *, mode="nextfit", rows=None, frac=0.15, mask_prob=0.8, random_prob=0.1,
                             mask_token=None, ignore_index=-100, label_dtype="q", seed=0, first_row=0, segment_ids=True, position_ids=True,
                             validate=True):
    """The masked-LM batch of a packed batch resident on the device, sequence-packed: the named tuple (inputs, labels, segment_ids,
    position_ids, starts, n_rows) -- `pack_tokenize_packed` with its tokens replaced by the masked inputs and the labels of
    `masking.mlm_tokenize_packed`, in ONE encode launch.

    A character's fate depends on (seed, first_row + its sequence's index in the batch, its index in the sequence) only -- never on the
    layout: the run of sequence i at `starts[i]` equals the head of row i of `mlm_tokenize_packed` with the same arguments, in either
    mode and at any padlen; a batch packed in pieces (`rows=N`, resumed at `n_placed` with `first_row` advanced by as much) or in
    shards gives every sequence the same run.  Positions outside every run hold PAD (0 for an unpadded tokenizer) and `ignore_index`;
    BOS / EOS are never selected.  `frac`, `mask_prob`, `random_prob`, `mask_token`, `ignore_index`, `label_dtype`, `seed`, `first_row`
    as in `mlm_tokenize_packed`; everything else -- `rows`, the one read-back of rows=None, `validate`, ValueError before any device
    work -- as in `pack_tokenize_packed`."""
    import torch
    desc, code, padlen, rows = _args(tok, padlen, mode, rows)
    m = _mlm_params(frac, mask_prob, random_prob, tok.alphabet_size() if mask_token is None else mask_token, ignore_index, seed, first_row)
    (dt, tdt), (ldt, ltdt) = capi.dtype_of(destchar), capi.dtype_of(label_dtype)
    B = capi.packed_on_device(chars, offsets, "pack_mlm_tokenize_packed works on packed batches resident on the device (chars, offsets tensors)")
    if validate and B > 0:
        _validate(chars, offsets, B, desc, code, padlen)
    starts, n_rows, n_placed = _plan(offsets, B, desc, code, padlen, rows)
    R = int(n_rows) if rows is None else rows  # (rows=None: the one read-back)
    dev = offsets.device
    if B > 0:
        inputs = torch.empty((R, padlen), dtype=tdt, device=dev)
        labels = torch.empty((R, padlen), dtype=ltdt, device=dev)
        seg = torch.empty((R, padlen), dtype=torch.int32, device=dev) if segment_ids else None
        pos = torch.empty((R, padlen), dtype=torch.int32, device=dev) if position_ids else None
    else:  # (the entry writes nothing for a batch without sequences: such a matrix is all PAD / ignore_index / 0 / 0)
        inputs = torch.full((R, padlen), tok.pad() if tok.is_padded() else 0, dtype=tdt, device=dev)
        labels = torch.full((R, padlen), int(ignore_index), dtype=ltdt, device=dev)
        seg = torch.zeros((R, padlen), dtype=torch.int32, device=dev) if segment_ids else None
        pos = torch.zeros((R, padlen), dtype=torch.int32, device=dev) if position_ids else None
    if R > 0 and B > 0:
        src = capi.readable_chars(chars, dev)
        with capi.launching(dev) as stream:
            capi.check(_lib.bsq_pack_mlm_tokenize_device(ctypes.byref(desc), src.data_ptr(), offsets.data_ptr(), B, starts.data_ptr(), R, padlen,
                                                         ctypes.byref(m), dt, inputs.data_ptr(), ldt, labels.data_ptr(),
                                                         seg.data_ptr() if segment_ids else None, pos.data_ptr() if position_ids else None,
                                                         stream))
    if rows is None:
        return PackedMlm(inputs, labels, seg, pos, starts, n_rows)
    return PackedMlmRows(inputs, labels, seg, pos, starts, n_rows, n_placed)


__all__ = ["pack_tokenize_packed", "pack_plan", "pack_plan_host", "pack_tokenize_host", "pack_rows_bound", "pack_cu_seqlens",
           "pack_kernel_name", "Packed", "PackedRows", "pack_mlm_tokenize_packed", "pack_mlm_tokenize_host", "pack_mlm_kernel_name",
           "PackedMlm", "PackedMlmRows"]
