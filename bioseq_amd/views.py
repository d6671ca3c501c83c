"""Views of packed batches on the device: fixed-width crops and reverse-complement strands (`bsq_crop_packed_device`,
`bsq_views_packed_device`).

Every encode path requires len + bos + eos <= padlen (the reference aborts on a longer sequence, tokenize.h:359-362), so without views
one outlier of a store sets the width of every batch.  A view is a window of a store sequence, optionally reverse-complemented; a list
of views comes back as a packed batch (chars, offsets) that tokenize, one-hot, the multi-batch calls, BLOSUM augmentation and the
masked-LM calls take as they are.

* `crop_packed`   rows drawn from (seed, row, length): a window of `window` characters at a random / head / centre start, and the
                  reverse complement with probability `revcomp_frac` (DNA strand augmentation);
* `gather_views`  explicit (sequence, start, length, strand) rows, e.g. the tiles of `tile_plan` for inference;
* `tile_plan`     the host-side tiling of whole sequences into overlapping windows;
* `crop_plan`     the library's CPU twin of the draw; `complement_table` its 256-byte complement table.

The draw is documented in include/bsq.h (`bsq_crop`).  Every call runs on torch's current stream; stores are packed batches on the
device (chars uint8[total], offsets int64[n + 1]).  A returned `chars` tensor may be longer than the batch: only its first
offsets[-1] bytes belong to it.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi

_lib = capi.load()

MODES = {"random": capi.CROP_RANDOM, "head": capi.CROP_HEAD, "center": capi.CROP_CENTER}


def _crop(window, mode, revcomp_frac, seed, first_row):
    """The bsq_crop struct, with the library's argument rules checked here first (no device is touched for a bad argument)."""
    if int(window) < 0:
        raise ValueError("window must be >= 0, got %r" % (window,))
    if mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(MODES), mode))
    p = float(revcomp_frac)
    if not 0.0 <= p <= 1.0:
        raise ValueError("revcomp_frac must lie in [0, 1], got %r" % (revcomp_frac,))
    if int(first_row) < 0:
        raise ValueError("first_row must be >= 0")
    return capi.Crop(int(window), MODES[mode], p, int(seed) & (2 ** 64 - 1), int(first_row))


def _check_store(chars, offsets):
    return capi.packed_on_device(chars, offsets, "views are cut from packed stores resident on the device (chars, offsets tensors)")


def _index_arg(index, n_store, dev):
    """(device int64 tensor, host array or None): a device tensor is taken as it is, a host list is range-checked and uploaded."""
    import torch
    if isinstance(index, torch.Tensor) and index.is_cuda:
        idx = index.to(torch.int64).contiguous()
        if idx.device != dev:
            raise ValueError("index lives on %s, the store on %s" % (idx.device, dev))
        return idx, None
    host = np.ascontiguousarray(np.asarray(index.cpu() if isinstance(index, torch.Tensor) else index, dtype=np.int64).ravel())
    if host.size and (host.min() < 0 or host.max() >= n_store):
        raise IndexError("Accessing sequence out of range")
    return torch.from_numpy(host).to(dev), host


def _raise_status(bad, n, what):
    if bad < 0:
        return
    if bad >= n:
        raise RuntimeError("%s: row %d did not fit into the output buffer" % (what, bad - n))
    raise IndexError("%s: row %d is out of range" % (what, bad))


def crop_packed(chars, offsets, window, *, index=None, mode="random", revcomp_frac=0.0, seed=0, first_row=0, return_origin=False,
                validate=True, capacity=None):
    """Packed batch (chars, offsets) of the views of store rows -- sequence index[i] (index None: every sequence of the store, in
    order) cut to at most `window` characters (0: whole sequences) and reverse-complemented with probability `revcomp_frac`.

    mode: "random" (a uniform start in [0, L - window]), "head" or "center".  Row i is row `first_row + i` of the draw: pieces of a
    list cut with their first_row give the whole list's views.  return_origin: also (starts int64[n], strand uint8[n]) device tensors
    -- where each view begins in its sequence and whether it was reverse-complemented.  `index`: an int64 device tensor (nothing
    crosses PCIe) or a host list (range-checked and uploaded).  validate=True with a device index reads the status back once and
    raises IndexError for a bad index; validate=False never synchronises (a bad index becomes an empty row).  capacity: bytes of the
    output buffer (default n * window, or the exact total for whole sequences -- a device index then costs one read-back)."""
    c = _crop(window, mode, revcomp_frac, seed, first_row)
    n_store = _check_store(chars, offsets)
    dev = chars.device
    host = None
    if index is None:
        idx, n = None, n_store
    else:
        idx, host = _index_arg(index, n_store, dev)
        n = int(idx.numel())
    if capacity is None:
        if c.window > 0:
            capacity = n * c.window
        elif index is None:
            capacity = int((offsets[-1] - offsets[0]).item()) if n else 0
        elif host is not None:
            lens = (offsets[1:] - offsets[:-1]).cpu().numpy()
            capacity = int(lens[host].clip(min=0).sum()) if n else 0
        else:
            capacity = n * int((offsets[1:] - offsets[:-1]).max().item()) if n and n_store else 0
    check = validate and index is not None and host is None
    out_chars, out_offs, starts, strand, status = _launch_crop(chars, offsets, n_store, idx, n, c, int(capacity), return_origin, check)
    if status is not None:
        _raise_status(int(status.item()), n, "crop_packed")
    return (out_chars, out_offs, starts, strand) if return_origin else (out_chars, out_offs)


def _launch_crop(chars, offsets, n_store, idx, n, c, capacity, origin=False, check=False):
    """bsq_crop_packed_device on checked arguments (crop_packed, and the loader with its own store and keys): the output tensors
    (chars, offsets, starts, strand, status), the last three None unless asked for."""
    import torch
    dev = chars.device
    out_chars = torch.empty(max(capacity, 1), dtype=torch.uint8, device=dev)
    out_offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    starts = torch.empty(n, dtype=torch.int64, device=dev) if origin else None
    strand = torch.empty(n, dtype=torch.uint8, device=dev) if origin else None
    status = torch.empty(1, dtype=torch.int64, device=dev) if check else None
    with capi.launching(dev) as stream:
        capi.check(_lib.bsq_crop_packed_device(capi.readable_chars(chars, dev).data_ptr(), offsets.data_ptr(), n_store,
                                               idx.data_ptr() if idx is not None else None, n, ctypes.byref(c), out_chars.data_ptr(), capacity,
                                               out_offs.data_ptr(), starts.data_ptr() if starts is not None and n else None,
                                               strand.data_ptr() if strand is not None and n else None,
                                               status.data_ptr() if status is not None else None, stream))
    return out_chars, out_offs, starts, strand, status


def gather_views(chars, offsets, seq, start, length, strand=None, validate=True):
    """Packed batch (chars, offsets) of explicit views of a store: row i = length[i] characters of sequence seq[i] from start[i],
    reverse-complemented where strand[i] != 0 (None: every row forward).  Host arrays are uploaded (8 bytes per entry), device
    tensors taken as they are (their total length costs one read-back).  A view outside its sequence becomes an empty row;
    validate=True reads the status back and raises IndexError for it."""
    import torch
    n_store = _check_store(chars, offsets)
    dev = chars.device

    def up(a, dtype):
        if isinstance(a, torch.Tensor):
            return a.to(device=dev, dtype=dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64 if dtype == torch.int64 else np.uint8).ravel())).to(dev)

    d_seq, d_start, d_len = up(seq, torch.int64), up(start, torch.int64), up(length, torch.int64)
    n = int(d_seq.numel())
    if d_start.numel() != n or d_len.numel() != n:
        raise ValueError("seq, start and length must have one entry per view")
    d_strand = None
    if strand is not None:
        d_strand = up(strand, torch.uint8)
        if d_strand.numel() != n:
            raise ValueError("strand must have one entry per view")
    if isinstance(length, torch.Tensor):
        capacity = int(d_len.clamp(min=0).sum().item()) if n else 0
    else:
        capacity = int(np.asarray(length, dtype=np.int64).clip(min=0).sum()) if n else 0
    out_chars = torch.empty(max(capacity, 1), dtype=torch.uint8, device=dev)
    out_offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int64, device=dev) if validate else None
    with capi.launching(dev) as stream:
        capi.check(_lib.bsq_views_packed_device(capi.readable_chars(chars, dev).data_ptr(), offsets.data_ptr(), n_store, d_seq.data_ptr(),
                                                d_start.data_ptr(), d_len.data_ptr(),
                                                d_strand.data_ptr() if d_strand is not None and n else None, n, out_chars.data_ptr(),
                                                capacity, out_offs.data_ptr(), status.data_ptr() if status is not None else None, stream))
    if status is not None:
        _raise_status(int(status.item()), n, "gather_views")
    return out_chars, out_offs


def tile_plan(offsets_or_lengths, window, stride=None, both_strands=False, *, lengths=False):
    """Host-side tiling of whole sequences into windows: (seq, start, length, strand) numpy arrays for `gather_views`.

    offsets_or_lengths: the store's offsets (n + 1 entries), or n sequence lengths with lengths=True.  In a sequence of length L the
    windows start at 0, stride, 2 * stride, ... while start + window < L, and one last window [max(0, L - window), L) covers the
    tail (stride <= window covers every character; default stride = window).  An empty sequence gives one empty view.
    both_strands: every window forward, then reverse-complemented."""
    window = int(window)
    stride = window if stride is None else int(stride)
    if window <= 0 or stride <= 0:
        raise ValueError("window and stride must be positive")
    a = np.asarray(offsets_or_lengths, dtype=np.int64).ravel()
    L = a if lengths else np.diff(a)
    if (L < 0).any():
        raise ValueError("sequence lengths must be >= 0")
    n = L.size
    # regular windows: start = k * stride for k * stride + window < L, i.e. k < ceil((L - window) / stride); then the tail window
    regular = np.where(L > window, (L - window + stride - 1) // stride, 0)
    count = regular + 1
    seq = np.repeat(np.arange(n, dtype=np.int64), count)
    first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(count, out=first[1:])
    k = np.arange(int(first[-1]), dtype=np.int64) - first[:-1][seq]
    Ls = L[seq]
    last = k == regular[seq]
    start = np.where(last, np.maximum(0, Ls - window), k * stride)
    length = np.where(last, np.minimum(Ls, window), window)
    strand = np.zeros(seq.size, dtype=np.uint8)
    if both_strands:
        seq, start, length = np.repeat(seq, 2), np.repeat(start, 2), np.repeat(length, 2)
        strand = np.tile(np.array([0, 1], dtype=np.uint8), k.size)
    return seq, start, length, strand


def crop_plan(offsets, window, *, index=None, mode="random", revcomp_frac=0.0, seed=0, first_row=0):
    """(starts, lengths, strand) numpy arrays of `crop_packed`'s views, computed on the CPU by the library's twin of the draw
    (`bsq_crop_plan_host`, the same code the kernels run).  offsets: the store's host offsets (n_store + 1 entries)."""
    c = _crop(window, mode, revcomp_frac, seed, first_row)
    offs = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).ravel())
    n_store = offs.size - 1
    idx = None if index is None else np.ascontiguousarray(np.asarray(index, dtype=np.int64).ravel())
    n = n_store if idx is None else idx.size
    if idx is not None and idx.size and (idx.min() < 0 or idx.max() >= n_store):
        raise IndexError("Accessing sequence out of range")
    starts, lens, strand = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.uint8)
    capi.check(_lib.bsq_crop_plan_host(offs.ctypes.data, n_store, idx.ctypes.data if idx is not None else None, n, ctypes.byref(c),
                                       starts.ctypes.data, lens.ctypes.data, strand.ctypes.data))
    return starts, lens, strand


def complement_table():
    """The library's complement table as uint8[256]: A<->T, C<->G, R<->Y, K<->M, B<->V, D<->H in either case, every other byte itself."""
    out = np.empty(256, dtype=np.uint8)
    capi.check(_lib.bsq_complement_table(out.ctypes.data))
    return out


__all__ = ["crop_packed", "gather_views", "tile_plan", "crop_plan", "complement_table"]
