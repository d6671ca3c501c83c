"""The exact edit distance of listed pairs of rows of packed stores resident on the device (`bsq_edit_pairs_device`), and the integer
identity rule that turns a candidate list into a verified one: the alignment step behind the k-mer filter of `bioseq_amd.sketch`.

    row, col, *_ = sketch.sketch_pairs(sk, min_jaccard=0.3)                  # generous candidates
    keep, dist = align.verify_pairs(tok, chars, offsets, row, col, min_identity=0.9)
    labels = sketch.cluster_pairs(row[keep], col[keep], B)                   # exact-identity clusters

The distance is the unit-cost Levenshtein distance of the two rows' class strings, global, one launch for the whole list.  The class of a
character is its id in the tokenizer's alphabet, and every character the alphabet does not map shares one extra class: case and alias
groups fold as the tokenizer folds them, `N` equals `N` in DNA4.  include/bsq.h ("edit distance of row pairs") has the rule.

* `edit_distance_pairs`  dist (int32) of every listed pair, a device tensor, nothing read back; -1 (`TOO_LONG`) where the shorter side
                         exceeds `max_len`, -2 (`BAD_INDEX`) where an index lies outside its store;
* `edit_distance_host`, `edit_kernel_name`    the library's CPU twin (numpy), the kernel taken;
* `pair_lengths`, `pair_identity`    (la, lb) of the listed pairs; 1 - dist / max(la, lb) as float32;
* `verify_pairs`, `verify_pairs_host`    (keep, dist): keep[k] <=> identity >= min_identity, decided in integers.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi

_lib = capi.load()

TOO_LONG, BAD_INDEX = -1, -2
MAX_LEN = 4096
_FORM_HOLDS = {1: 256, 2: 1024, 3: 4096}


def _edit(tok, max_len, form):
    """(desc, bsq_edit) with the library's argument rules applied as ValueError (no device is touched)."""
    desc = capi.desc_of(tok)
    if not 1 <= desc.nchars <= 30:
        raise ValueError("the edit distance takes alphabets of 1 .. 30 classes, %r has %d" % (tok.key, desc.nchars))
    if isinstance(max_len, bool) or int(max_len) != max_len or not 1 <= int(max_len) <= MAX_LEN:
        raise ValueError("max_len must be an integer in 1 .. %d, got %r" % (MAX_LEN, max_len))
    form = 0 if form is None else form
    if isinstance(form, bool) or form not in (0, 1, 2, 3) or (form and _FORM_HOLDS[form] < int(max_len)):
        raise ValueError("form must be None or 1, 2, 3 (shorter sides up to 256, 1024, 4096), got %r at max_len %d" % (form, int(max_len)))
    e = capi.Edit(int(max_len), int(form))
    if not _lib.bsq_edit_pairs_kernel_name(ctypes.byref(e)):  # (whatever the rules above do not restate)
        raise ValueError("the library refuses these arguments (include/bsq.h, \"edit distance of row pairs\")")
    return desc, e


def _identity_q16(min_identity):
    if not 0.0 <= float(min_identity) <= 1.0:  # (a NaN fails both comparisons)
        raise ValueError("min_identity must lie in 0 .. 1, got %r" % (min_identity,))
    return int(float(min_identity) * 65536 + 0.5)


def edit_kernel_name(max_len=MAX_LEN, form=None):
    """The kernel `edit_distance_pairs` takes (host only: profiling labels, tests)."""
    e = capi.Edit(int(max_len), 0 if form is None else int(form))
    return _lib.bsq_edit_pairs_kernel_name(ctypes.byref(e)).decode()


def _host_lists(row, col):
    row, col = np.ascontiguousarray(row), np.ascontiguousarray(col)
    if row.dtype != np.int64 or col.dtype != np.int64 or row.ndim != 1 or row.shape != col.shape:
        raise ValueError("row and col are int64 arrays of one length")
    return row, col


def edit_distance_host(tok, chars, offsets, row, col, chars_b=None, offsets_b=None, *, max_len=MAX_LEN, form=None):
    """The library's CPU twin (`bsq_edit_pairs_host`: the class and block-step text of the kernels in plain loops) on numpy arrays:
    dist as an int32 array, with `edit_distance_pairs`' meaning of every argument (form is checked and changes nothing)."""
    desc, e = _edit(tok, max_len, form)
    if (chars_b is None) != (offsets_b is None):
        raise ValueError("chars_b and offsets_b come together")
    row, col = _host_lists(row, col)
    ca, oa = capi.host_batch(chars, offsets)
    cb, ob = (ca, oa) if chars_b is None else capi.host_batch(chars_b, offsets_b)
    dist = np.empty(row.size, np.int32)
    if row.size:
        capi.check(_lib.bsq_edit_pairs_host(ctypes.byref(desc), ca.ctypes.data, oa.ctypes.data, oa.size - 1, cb.ctypes.data, ob.ctypes.data, ob.size - 1,
                                            row.ctypes.data, col.ctypes.data, row.size, ctypes.byref(e), dist.ctypes.data))
    return dist


def _device_lists(row, col, device):
    import torch
    if not (isinstance(row, torch.Tensor) and isinstance(col, torch.Tensor) and row.is_cuda and row.device == col.device == device):
        raise ValueError("row and col are index tensors resident on the device of the stores")
    if row.dtype != torch.int64 or col.dtype != torch.int64 or row.ndim != 1 or row.shape != col.shape or not row.is_contiguous() or not col.is_contiguous():
        raise ValueError("row and col are contiguous int64 tensors of one length")


def edit_distance_pairs(tok, chars, offsets, row, col, chars_b=None, offsets_b=None, *, max_len=MAX_LEN, form=None):
    """dist[k] = the edit distance between row row[k] of the store (chars, offsets) and row col[k] of the store (chars_b, offsets_b) --
    the same store when those are None: an int32 device tensor on torch's current stream, one launch, nothing read back.

    The stores are packed batches resident on one device (chars uint8[total], offsets int64[B + 1]); row and col are contiguous int64
    device tensors of one length.  max_len (1 .. 4096) bounds the SHORTER side of every pair: a pair whose shorter side is longer gets
    `TOO_LONG` (-1); the longer side may have any length.  An index outside its store gives `BAD_INDEX` (-2) and is never followed, so
    the zeros behind a list cut at `max_pairs` are simply the pair (0, 0).  form: None = the smallest that holds max_len, or 1, 2, 3 to
    force 4, 16, 64 lanes per pair (shorter sides up to 256, 1024, 4096; the result does not depend on it).  A smaller max_len is a
    cheaper kernel: 16 (or 4) pairs share a wave instead of one."""
    import torch
    desc, e = _edit(tok, max_len, form)
    if (chars_b is None) != (offsets_b is None):
        raise ValueError("chars_b and offsets_b come together")
    what = "edit_distance_pairs works on packed batches resident on the device (chars, offsets tensors)"
    Ba = capi.packed_on_device(chars, offsets, what)
    Bb = Ba if chars_b is None else capi.packed_on_device(chars_b, offsets_b, what)
    if chars_b is not None and chars_b.device != chars.device:
        raise ValueError("both stores must live on one device")
    _device_lists(row, col, chars.device)
    dist = torch.empty(row.numel(), dtype=torch.int32, device=chars.device)
    if row.numel():
        ca = capi.readable_chars(chars, chars.device)  # (every row may be empty)
        cb = ca if chars_b is None else capi.readable_chars(chars_b, chars.device)
        ob = offsets if offsets_b is None else offsets_b
        with capi.launching(chars.device) as stream:
            capi.check(_lib.bsq_edit_pairs_device(ctypes.byref(desc), ca.data_ptr(), offsets.data_ptr(), Ba, cb.data_ptr(), ob.data_ptr(), Bb,
                                                  row.data_ptr(), col.data_ptr(), row.numel(), ctypes.byref(e), dist.data_ptr(), stream))
    return dist


def pair_lengths(offsets, row, offsets_b=None, col=None):
    """(la, lb): the lengths of rows row[k] of `offsets` and col[k] of `offsets_b` (default: `offsets`; col default: row), int64, in
    torch on the tensors' device.  The indices must be valid: what `edit_distance_pairs` marks BAD_INDEX has no length."""
    offsets_b = offsets if offsets_b is None else offsets_b
    col = row if col is None else col
    return offsets[row + 1] - offsets[row], offsets_b[col + 1] - offsets_b[col]


def pair_identity(dist, la, lb):
    """1 - dist / max(la, lb) as float32 (computed in float64): 1 where both lengths are 0, NaN where dist < 0 (a code)."""
    import torch
    L = torch.maximum(la, lb).to(torch.float64)
    ident = torch.where(L > 0, 1.0 - dist.to(torch.float64) / L.clamp(min=1.0), torch.ones_like(L))
    return torch.where(dist < 0, torch.full_like(ident, float("nan")), ident).to(torch.float32)


def _valid_lengths(xp, offsets, idx):
    """The lengths of rows idx of `offsets`, 0 where idx lies outside the store (numpy or torch by `xp`)."""
    B = offsets.shape[0] - 1
    if B <= 0:
        return xp.zeros_like(idx)
    ok = (idx >= 0) & (idx < B)
    safe = xp.where(ok, idx, xp.zeros_like(idx))
    return xp.where(ok, offsets[safe + 1] - offsets[safe], xp.zeros_like(idx))


def verify_pairs_host(tok, chars, offsets, row, col, chars_b=None, offsets_b=None, *, min_identity=0.9, max_len=MAX_LEN):
    """`verify_pairs` on numpy arrays through the CPU twin: (keep, dist) as numpy arrays, the same bits."""
    T = _identity_q16(min_identity)
    dist = edit_distance_host(tok, chars, offsets, row, col, chars_b, offsets_b, max_len=max_len)
    row, col = _host_lists(row, col)
    oa = np.asarray(offsets, np.int64).ravel()
    ob = oa if offsets_b is None else np.asarray(offsets_b, np.int64).ravel()
    L = np.maximum(_valid_lengths(np, oa, row), _valid_lengths(np, ob, col))
    return (dist >= 0) & (dist.astype(np.int64) * 65536 <= (65536 - T) * L), dist


def verify_pairs(tok, chars, offsets, row, col, chars_b=None, offsets_b=None, *, min_identity=0.9, max_len=MAX_LEN):
    """(keep, dist) of a candidate list: dist as `edit_distance_pairs` gives it, and keep[k] (bool) true when the pair's identity
    1 - dist / L, L = max(la, lb), reaches min_identity.  Decided in 64-bit integers, in torch on the device, nothing read back:
    dist >= 0 and dist * 65536 <= (65536 - T) * L with T = floor(min_identity * 65536 + 0.5), so `verify_pairs_host` keeps the same
    pairs bit for bit.  A pair that got a code (-1, -2) is never kept; two empty rows pass any threshold.  `row[keep]`, `col[keep]` is
    the verified list, which `sketch.cluster_pairs` takes."""
    import torch
    T = _identity_q16(min_identity)
    dist = edit_distance_pairs(tok, chars, offsets, row, col, chars_b, offsets_b, max_len=max_len)
    L = torch.maximum(_valid_lengths(torch, offsets, row), _valid_lengths(torch, offsets if offsets_b is None else offsets_b, col))
    return (dist >= 0) & (dist.to(torch.int64) * 65536 <= (65536 - T) * L), dist


__all__ = ["TOO_LONG", "BAD_INDEX", "MAX_LEN", "edit_distance_pairs", "edit_distance_host", "edit_kernel_name", "pair_lengths", "pair_identity",
           "verify_pairs", "verify_pairs_host"]
