"""Open reading frames on the device: the ORFs of six-frame translations as protein rows (`bsq_orf_count_device`,
`bsq_orf_emit_device`).

A raw frame of a read or contig is a stop every ~21 residues with noise between the stops; the rows that belong in front of a
protein encoder are the stop-free stretches of at least `min_len` residues, optionally from their first start residue.  A nucleotide
store resident on the GPU becomes a packed batch (chars, offsets) of those stretches without the translated batch ever leaving the
device, in the order (row, start) -- the job `orfm` or `getorf` do on the host.

* `find_orfs_packed`   (row, start, length, orf_offsets) of any packed protein batch on the device;
* `orfs_packed`        the whole pipeline on a nucleotide store: translate, count, emit, one views launch;
* `find_orfs_host`, `orfs_host`   the same on numpy arrays through the library's CPU twins (the rule text the kernels compile);
* `orf_spans`          the nucleotide interval an ORF was read from;
* `kernel_name`        the launches of the two device calls.

The rule is documented in include/bsq.h ("open reading frames"): terminators are the stops and the row's end, a segment runs from
behind the previous stop to its terminator, an ORF begins at the segment's first position (start=None) or at its first `start`
residue, and is kept when it has at least `min_len` residues; the stop is not part of it.  Every call runs on torch's current stream.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi
from .translate import _byte, _host_frames, _rule as _translate_rule

_lib = capi.load()


def _rule(min_len, stop, start):
    """The bsq_orf struct, with the library's argument rules checked here first (no device is touched for a bad argument)."""
    if isinstance(min_len, bool) or int(min_len) != min_len or int(min_len) < 1:
        raise ValueError("min_len must be an integer >= 1, got %r" % (min_len,))
    s = _byte(stop, "stop")
    t = -1 if start is None else _byte(start, "start")
    if t == s:
        raise ValueError("start and stop must differ, got %r for both" % (stop,))
    return capi.Orf(s, t, int(min_len))


def _max_orfs(max_orfs):
    if max_orfs is None:
        return None
    if int(max_orfs) < 0:
        raise ValueError("max_orfs must be >= 0, got %r" % (max_orfs,))
    return int(max_orfs)


def _find(chars, offsets, n_rows, rule, max_orfs):
    """count + emit on checked arguments: (row, start, length, orf_offsets, residues) device tensors; `residues` a one-element tensor."""
    import torch
    dev = chars.device
    orf_offs = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
    residues = torch.empty(1, dtype=torch.int64, device=dev)
    src = capi.readable_chars(chars, dev)
    with capi.launching(dev) as stream:
        capi.check(_lib.bsq_orf_count_device(src.data_ptr(), offsets.data_ptr(), n_rows, ctypes.byref(rule), orf_offs.data_ptr(),
                                             residues.data_ptr(), stream))
        if max_orfs is None:
            n, make = int(orf_offs[-1].item()), torch.empty
        else:  # entries at and past the count stay zero: empty views of row 0
            n, make = max_orfs, torch.zeros
        row, start, length = (make(n, dtype=torch.int64, device=dev) for _ in range(3))
        if n:
            capi.check(_lib.bsq_orf_emit_device(src.data_ptr(), offsets.data_ptr(), n_rows, ctypes.byref(rule), orf_offs.data_ptr(), n,
                                                row.data_ptr(), start.data_ptr(), length.data_ptr(), stream))
    return row, start, length, orf_offs, residues


def find_orfs_packed(chars, offsets, *, min_len=30, stop="*", start=None, max_orfs=None):
    """(row, start, length, orf_offsets) int64 device tensors: the ORFs of a packed protein batch (chars, offsets) on the device in
    (row, start) order, and the CSR of their ranks over the rows (the ORFs of row r are orf_offsets[r] .. orf_offsets[r + 1]).

    max_orfs=None reads orf_offsets[-1] back (8 bytes) and sizes the arrays exactly.  max_orfs=N reads nothing back: the arrays hold
    N entries, the ORFs of rank < N and zeros behind the last one; orf_offsets[-1] > N tells later that the list was cut."""
    rule = _rule(min_len, stop, start)
    cap = _max_orfs(max_orfs)
    n_rows = capi.packed_on_device(chars, offsets, "ORFs are found in packed batches resident on the device (chars, offsets tensors)")
    return _find(chars, offsets, n_rows, rule, cap)[:4]


def orfs_packed(chars, offsets, *, index=None, frame="six", table=1, unknown="X", stop="*", min_len=30, start=None, max_orfs=None,
                capacity=None):
    """(orf_chars, orf_offsets, origin): the ORFs of the translated rows of a nucleotide store as a packed protein batch, and where each
    came from -- origin = (source_row, frame_code, start, length) int64 device tensors, start and length in residues of the frame row
    (`orf_spans` turns them into nucleotides).  Row i of the list is store sequence index[i] (index None: every sequence); with
    frame="six" ORF k comes from list row source_row[k] in frame frame_code[k].

    The store is translated into a scratch batch (`translate_packed`'s arguments: frame, table, unknown, stop), its ORFs are counted
    and listed, and one `bsq_views_packed_device` launch copies them out of the scratch.  max_orfs / capacity: rows and bytes of the
    output.  None reads the count / the summed length back (8 bytes each); with both given and index=None nothing is read back, the
    batch has max_orfs rows -- those behind the last ORF empty -- and is cut at `capacity` bytes."""
    import torch
    rule = _rule(min_len, stop, start)
    cap_orfs = _max_orfs(max_orfs)
    if capacity is not None and int(capacity) < 0:
        raise ValueError("capacity must be >= 0, got %r" % (capacity,))
    t, rows = _translate_rule(frame, table, unknown, stop)
    n_store = capi.packed_on_device(chars, offsets, "ORF extraction reads packed stores resident on the device (chars, offsets tensors)")
    dev = chars.device
    if index is None:
        idx, n = None, n_store
    else:
        from .views import _index_arg
        idx, _ = _index_arg(index, n_store, dev)
        n = int(idx.numel())
    frames = None
    if rows is not None:
        if isinstance(rows, torch.Tensor) and rows.is_cuda:
            if rows.device != dev or rows.dim() != 1 or rows.numel() != n:
                raise ValueError("per-row frames must be one code per row (%d) on the store's device" % n)
            frames = rows.to(torch.uint8).contiguous()
        else:
            frames = torch.from_numpy(_host_frames(rows.cpu().numpy() if isinstance(rows, torch.Tensor) else rows, n)).to(dev)
    six = t.frame == capi.FRAME_SIX
    n_out = 6 * n if six else n
    # the scratch: a frame holds at most a third of the characters, the six frames twice their number
    if not n or not n_store:
        scratch = 0
    elif index is None:
        scratch = 2 * int(chars.numel()) if six else int(chars.numel()) // 3
    else:
        scratch = n * (int((offsets[1:] - offsets[:-1]).max().item()) // 3) * (6 if six else 1)
    from .translate import _launch
    p_chars, p_offs, _ = _launch(chars, offsets, n_store, idx, frames, n, n_out, t, scratch)
    row, o_start, o_len, _, residues = _find(p_chars, p_offs, n_out, rule, cap_orfs)
    n_orfs = int(row.numel())
    cap = int(residues.item()) if capacity is None else int(capacity)
    out_chars = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
    out_offs = torch.empty(n_orfs + 1, dtype=torch.int64, device=dev)
    with capi.launching(dev) as stream:
        capi.check(_lib.bsq_views_packed_device(p_chars.data_ptr(), p_offs.data_ptr(), n_out, row.data_ptr(), o_start.data_ptr(),
                                                o_len.data_ptr(), None, n_orfs, out_chars.data_ptr(), cap, out_offs.data_ptr(), None, stream))
    if six:
        source, code = torch.div(row, 6, rounding_mode="floor"), row % 6
    elif frames is not None:
        source, code = row, frames[row].to(torch.int64) if n else row.clone()
    else:
        source, code = row, torch.full_like(row, t.frame)
    return out_chars, out_offs, (source, code, o_start, o_len)


def _host_batch(chars, offsets):
    ch, offs = capi.host_batch(chars, offsets)
    if offs.size < 1:
        raise ValueError("offsets must hold at least one entry")
    return ch, offs


def find_orfs_host(chars, offsets, *, min_len=30, stop="*", start=None, max_orfs=None):
    """`find_orfs_packed` on numpy arrays, computed on the CPU by the library's twins (`bsq_orf_count_host`, `bsq_orf_emit_host`)."""
    rule = _rule(min_len, stop, start)
    cap = _max_orfs(max_orfs)
    ch, offs = _host_batch(chars, offsets)
    n_rows = offs.size - 1
    orf_offs = np.empty(n_rows + 1, dtype=np.int64)
    capi.check(_lib.bsq_orf_count_host(ch.ctypes.data, offs.ctypes.data, n_rows, ctypes.byref(rule), orf_offs.ctypes.data, None))
    n = int(orf_offs[-1]) if cap is None else cap
    row, o_start, o_len = (np.zeros(n, dtype=np.int64) for _ in range(3))
    if n:
        capi.check(_lib.bsq_orf_emit_host(ch.ctypes.data, offs.ctypes.data, n_rows, ctypes.byref(rule), orf_offs.ctypes.data, n,
                                          row.ctypes.data, o_start.ctypes.data, o_len.ctypes.data))
    return row, o_start, o_len, orf_offs


def orfs_host(chars, offsets, *, index=None, frame="six", table=1, unknown="X", stop="*", min_len=30, start=None):
    """`orfs_packed` on numpy arrays through the CPU twins: (orf_chars, orf_offsets, (source_row, frame_code, start, length))."""
    from .translate import translate_host
    _rule(min_len, stop, start)
    p_chars, p_offs = translate_host(chars, offsets, index=index, frame=frame, table=table, unknown=unknown, stop=stop)
    row, o_start, o_len, _ = find_orfs_host(p_chars, p_offs, min_len=min_len, stop=stop, start=start)
    out_offs = np.zeros(row.size + 1, dtype=np.int64)
    np.cumsum(o_len, out=out_offs[1:])
    first = p_offs[row] + o_start
    take = np.repeat(first - out_offs[:-1], o_len) + np.arange(int(out_offs[-1]), dtype=np.int64)
    t, rows = _translate_rule(frame, table, unknown, stop)
    if t.frame == capi.FRAME_SIX:
        source, code = row // 6, row % 6
    elif rows is not None:
        source, code = row, np.asarray(rows, dtype=np.int64).ravel()[row]
    else:
        source, code = row, np.full_like(row, t.frame)
    return p_chars[take], out_offs, (source, code, o_start, o_len)


def orf_spans(L, frame_code, start, length):
    """(a, b): the half-open interval [a, b) of the forward strand of a source row of L characters that an ORF of its frame
    `frame_code` row was read from -- forward frames [f + 3 s, f + 3 (s + len)), reverse frames [L - f - 3 (s + len), L - f - 3 s),
    f = frame_code % 3.  Numbers, numpy arrays or tensors, elementwise."""
    f = frame_code % 3
    lo, hi = 3 * start, 3 * (start + length)
    reverse = frame_code >= 3
    try:
        import torch
        where = torch.where if any(isinstance(x, torch.Tensor) for x in (L, frame_code, start, length)) else np.where
    except ImportError:  # pragma: no cover
        where = np.where
    if where is np.where and np.ndim(reverse) == 0:
        return (L - f - hi, L - f - lo) if reverse else (f + lo, f + hi)
    return where(reverse, L - f - hi, f + lo), where(reverse, L - f - lo, f + hi)


def kernel_name(n_rows):
    """The launches of `bsq_orf_count_device` and `bsq_orf_emit_device` for a batch of n_rows rows, the count's before the ';'."""
    return _lib.bsq_orf_kernel_name(int(n_rows)).decode()


__all__ = ["find_orfs_packed", "orfs_packed", "find_orfs_host", "orfs_host", "orf_spans", "kernel_name"]
