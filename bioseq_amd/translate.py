"""Codon translation on the device: protein views of nucleotide batches (`bsq_translate_packed_device`).

A store of reads, contigs or CDS records resident on the GPU becomes a packed batch (chars, offsets) of amino-acid letters -- one
reading frame of every row, a frame per row, or all six frames of every row -- that tokenize, the reduced alphabets, one-hot, the
masked-LM calls, sequence packing and BLOSUM augmentation take as they are: six-frame translation in front of a protein encoder
without a host loop and without padding a ragged store to its longest row.

* `translate_packed`    the device call: rows index[i] (or every row) of a store, translated;
* `translate_host`      the same on numpy arrays through the library's CPU twin (the same rule text the kernels compile);
* `codon_table`         NCBI tables 1, 2, 4 and 11 as uint8[64], or a caller's own 64 bytes checked;
* `translated_length`   residues of a row of L characters under a frame code;
* `six_frame_origin`    (source row, frame code) of every output row of frame="six".

The rule is documented in include/bsq.h ("codon translation"): frame codes 0, 1, 2 forward and 3, 4, 5 reverse, phase = code % 3,
m = max(0, L - phase) // 3 residues, a trailing partial codon dropped; A C G T U in either case are bases (U reads as T), a codon with
any other byte becomes `unknown`; stops stay in the row as the table's `*` (or `stop`).  Every call runs on torch's current stream.
A returned `chars` tensor may be longer than the batch: only its first offsets[-1] bytes belong to it.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi

_lib = capi.load()

SIX = "six"


def codon_table(table=1):
    """uint8[64] genetic code, entry 16 * b0 + 4 * b1 + b2 with bases in NCBI's order T, C, A, G: NCBI table `table` (1, 2, 4 or 11),
    or 64 bytes / a 64-character string of the caller's own."""
    if isinstance(table, (int, np.integer)) and not isinstance(table, bool):
        out = np.empty(64, dtype=np.uint8)
        if _lib.bsq_codon_table(int(table), out.ctypes.data) != capi.OK:
            raise ValueError("codon table must be 1, 2, 4 or 11 (or 64 bytes), got %r" % (table,))
        return out
    if isinstance(table, str):
        table = table.encode("latin-1")
    out = np.frombuffer(bytes(table), dtype=np.uint8) if isinstance(table, (bytes, bytearray)) else np.asarray(table, dtype=np.uint8).ravel()
    if out.size != 64:
        raise ValueError("a codon table holds 64 letters, got %d" % out.size)
    return out.copy()


def _byte(value, name):
    if isinstance(value, str):
        value = value.encode("latin-1")
    if isinstance(value, (bytes, bytearray)):
        if len(value) != 1:
            raise ValueError("%s must be one character, got %r" % (name, value))
        return value[0]
    if not 0 <= int(value) <= 255:
        raise ValueError("%s must be one byte, got %r" % (name, value))
    return int(value)


def _rule(frame, table, unknown, stop):
    """(bsq_translate struct, per-row frames or None): the library's argument rules checked here first (no device is touched for a
    bad argument).  `stop` rewrites the table's '*' entries."""
    code = codon_table(table)
    s = _byte(stop, "stop")
    if s != ord("*"):
        code[code == ord("*")] = s
    t = capi.Translate()
    ctypes.memmove(t.code, code.ctypes.data, 64)
    t.unknown = _byte(unknown, "unknown")
    rows = None
    if isinstance(frame, str):
        if frame != SIX:
            raise ValueError("frame must be 0 .. 5, 'six' or one code per row, got %r" % (frame,))
        t.frame = capi.FRAME_SIX
    elif isinstance(frame, (int, np.integer)) and not isinstance(frame, bool):
        if not 0 <= int(frame) <= 5:
            raise ValueError("frame must be 0 .. 5, 'six' or one code per row, got %r" % (frame,))
        t.frame = int(frame)
    else:
        t.frame, rows = 0, frame
    return t, rows


def _host_frames(rows, n):
    host = np.asarray(rows)
    if host.ndim != 1 or host.size != n:
        raise ValueError("per-row frames must have one code per row (%d), got shape %r" % (n, host.shape))
    if host.size and (host.min() < 0 or host.max() > 5):
        raise ValueError("frame codes must be 0 .. 5")
    return np.ascontiguousarray(host, dtype=np.uint8)


def translated_length(L, frame):
    """Residues of a row of L characters (a number or an array) under frame code 0 .. 5: max(0, L - frame % 3) // 3."""
    if not 0 <= int(frame) <= 5:
        raise ValueError("frame must be 0 .. 5, got %r" % (frame,))
    if np.ndim(L) == 0:
        m = int(_lib.bsq_translate_length(int(L), int(frame)))
        if m < 0:
            raise ValueError("L must be >= 0, got %r" % (L,))
        return m
    L = np.asarray(L, dtype=np.int64)
    if (L < 0).any():
        raise ValueError("L must be >= 0")
    return np.maximum(L - int(frame) % 3, 0) // 3


def six_frame_origin(n):
    """(source row, frame code) int64 arrays of the 6 * n output rows of frame="six": row r comes from source row r // 6, frame r % 6."""
    n = int(n)
    if n < 0:
        raise ValueError("n must be >= 0")
    return np.repeat(np.arange(n, dtype=np.int64), 6), np.tile(np.arange(6, dtype=np.int64), n)


def _total_residues(lens, t, rows):
    """Residues of source rows with these lengths (host arrays): the exact size of the output."""
    lens = np.maximum(np.asarray(lens, dtype=np.int64), 0)
    if t.frame == capi.FRAME_SIX:
        return int(sum(translated_length(lens, c).sum() for c in range(3)) * 2)
    if rows is not None:
        return int((np.maximum(lens - rows.astype(np.int64) % 3, 0) // 3).sum())
    return int(translated_length(lens, t.frame).sum())


def _raise_status(bad, n_out, what):
    if bad < 0:
        return
    if bad >= n_out:
        raise RuntimeError("%s: row %d did not fit into the output buffer" % (what, bad - n_out))
    raise IndexError("%s: row %d has an index out of range or a frame code above 5" % (what, bad))


def translate_packed(chars, offsets, *, index=None, frame=0, table=1, unknown="X", stop="*", validate=True, capacity=None):
    """Packed batch (chars, offsets) of amino-acid letters: store sequence index[i] (index None: every sequence, in order) translated
    in `frame`.

    frame: a code 0 .. 5 for every row; "six" -- source row i gives the output rows 6 * i + c, c = 0 .. 5 (`six_frame_origin`); or one
    code per row as a host array (checked and uploaded) or a uint8 device tensor (taken as it is).  table: an NCBI id (1, 2, 4, 11) or
    64 bytes; `stop` replaces the table's '*' letters, `unknown` is the letter of a codon with a byte that is no base.  `index`: an
    int64 device tensor (nothing crosses PCIe) or a host list (range-checked and uploaded).  validate=True with a device index or
    device frames reads the status back once and raises IndexError for a bad row; validate=False never synchronises (a bad row is
    empty).  capacity: bytes of the output buffer (default: exact for a host index list -- the store's offsets are read back once --,
    else a bound from one read-back of the store's total or longest length)."""
    import torch
    t, rows = _rule(frame, table, unknown, stop)
    n_store = capi.packed_on_device(chars, offsets, "translation reads packed stores resident on the device (chars, offsets tensors)")
    dev = chars.device
    host = None
    if index is None:
        idx, n = None, n_store
    else:
        from .views import _index_arg
        idx, host = _index_arg(index, n_store, dev)
        n = int(idx.numel())
    frames, host_rows = None, None
    if rows is not None:
        if isinstance(rows, torch.Tensor) and rows.is_cuda:
            if rows.device != dev:
                raise ValueError("frames live on %s, the store on %s" % (rows.device, dev))
            if rows.dim() != 1 or rows.numel() != n:
                raise ValueError("per-row frames must have one code per row (%d)" % n)
            frames = rows.to(torch.uint8).contiguous()
        else:
            host_rows = _host_frames(rows.cpu().numpy() if isinstance(rows, torch.Tensor) else rows, n)
            frames = torch.from_numpy(host_rows).to(dev)
    six = t.frame == capi.FRAME_SIX
    n_out = 6 * n if six else n
    if capacity is None:
        if not n or not n_store:
            capacity = 0
        elif host is not None and (rows is None or host_rows is not None):
            lens = (offsets[1:] - offsets[:-1]).cpu().numpy()
            capacity = _total_residues(lens[host], t, host_rows)
        elif index is None:  # a frame holds at most a third of the characters, the six frames twice their number
            total = int((offsets[-1] - offsets[0]).item())
            capacity = 2 * total if six else total // 3
        else:
            capacity = n * (int((offsets[1:] - offsets[:-1]).max().item()) // 3) * (6 if six else 1)
    check = validate and ((index is not None and host is None) or (rows is not None and host_rows is None))
    out_chars, out_offs, status = _launch(chars, offsets, n_store, idx, frames, n, n_out, t, int(capacity), check)
    if status is not None:
        _raise_status(int(status.item()), n_out, "translate_packed")
    return out_chars, out_offs


def _launch(chars, offsets, n_store, idx, frames, n, n_out, t, capacity, check=False):
    """bsq_translate_packed_device on checked arguments (translate_packed, and the loader with its own store): the output tensors
    (chars, offsets, status), the last None unless asked for."""
    import torch
    dev = chars.device
    out_chars = torch.empty(max(capacity, 1), dtype=torch.uint8, device=dev)
    out_offs = torch.empty(n_out + 1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int64, device=dev) if check else None
    with capi.launching(dev) as stream:
        capi.check(_lib.bsq_translate_packed_device(capi.readable_chars(chars, dev).data_ptr(), offsets.data_ptr(), n_store,
                                                    idx.data_ptr() if idx is not None else None,
                                                    frames.data_ptr() if frames is not None and n else None, n, ctypes.byref(t),
                                                    out_chars.data_ptr(), capacity, out_offs.data_ptr(),
                                                    status.data_ptr() if status is not None else None, stream))
    return out_chars, out_offs, status


def translate_host(chars, offsets, *, index=None, frame=0, table=1, unknown="X", stop="*", validate=True, capacity=None):
    """`translate_packed` on numpy arrays, computed on the CPU by the library's twin (`bsq_translate_packed_host`, the rule text the
    kernels compile): (chars uint8[total], offsets int64[rows + 1]).  validate=False: a bad index or frame code gives an empty row
    instead of IndexError, and a `capacity` too small cuts the batch instead of raising."""
    t, rows = _rule(frame, table, unknown, stop)
    ch, offs = capi.host_batch(chars, offsets)
    n_store = offs.size - 1
    if n_store < 0:
        raise ValueError("offsets must hold at least one entry")
    idx = None if index is None else np.ascontiguousarray(np.asarray(index, dtype=np.int64).ravel())
    n = n_store if idx is None else idx.size
    if validate and idx is not None and idx.size and (idx.min() < 0 or idx.max() >= n_store):
        raise IndexError("Accessing sequence out of range")
    frames = None
    if rows is not None:
        frames = _host_frames(rows, n) if validate else np.ascontiguousarray(np.asarray(rows).ravel(), dtype=np.uint8)
        if frames.size != n:
            raise ValueError("per-row frames must have one code per row (%d)" % n)
    n_out = 6 * n if t.frame == capi.FRAME_SIX else n
    if capacity is None:
        lens = np.diff(offs)
        ok = idx if idx is None else np.clip(idx, 0, max(n_store - 1, 0))
        capacity = _total_residues(lens if ok is None else (lens[ok] if n_store else lens[:0]), t, frames) if n else 0
    capacity = int(capacity)
    out = np.empty(max(capacity, 1), dtype=np.uint8)
    out_offs = np.empty(n_out + 1, dtype=np.int64)
    status = ctypes.c_int64(-1)
    capi.check(_lib.bsq_translate_packed_host(ch.ctypes.data, offs.ctypes.data, n_store, idx.ctypes.data if idx is not None else None,
                                              frames.ctypes.data if frames is not None and n else None, n, ctypes.byref(t),
                                              out.ctypes.data, capacity, out_offs.ctypes.data, ctypes.byref(status)))
    if validate:
        _raise_status(status.value, n_out, "translate_host")
    return out[:min(int(out_offs[-1]), capacity)], out_offs


def kernel_name(n, frame=0):
    """The launches `translate_packed` takes for n source rows in `frame` (a code or "six"): `bsq_translate_kernel_name`."""
    t, _ = _rule(frame if isinstance(frame, (str, int, np.integer)) else 0, 1, "X", "*")
    return _lib.bsq_translate_kernel_name(int(n), ctypes.byref(t)).decode()


__all__ = ["translate_packed", "translate_host", "codon_table", "translated_length", "six_frame_origin", "kernel_name"]
