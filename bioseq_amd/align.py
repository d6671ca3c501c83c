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

For proteins the measure is a scored alignment (`bsq_score_pairs_device`; include/bsq.h, "scored alignment of row pairs"): Gotoh's
algorithm with a substitution matrix over the classes and affine gap costs, local or global.

    S = align.blosum62_matrix(tok)
    keep, score = align.verify_score_pairs(tok, chars, offsets, row, col, matrix=S, gap_open=11, gap_extend=1, min_ratio=0.5)

* `score_matrix`, `blosum62_matrix`    match / mismatch and BLOSUM62 matrices over a tokenizer's classes (int8 numpy);
* `score_pairs`, `score_pairs_host`, `score_kernel_name`    score (int32), optionally the ends of the best cell; the CPU twin; the kernel;
* `self_scores`    the perfect score of every row, int64;
* `verify_score_pairs`, `verify_score_pairs_host`    (keep, score): keep[k] <=> score / min(self_a, self_b) >= min_ratio, in integers.

What cd-hit and mmseqs threshold on is the alignment itself: sequence identity over it and coverage of the rows by it
(`bsq_align_stats_device`; include/bsq.h, "alignment statistics of row pairs"): start, end, identical columns and length of one optimal
alignment, carried through the same recurrence in one launch, no traceback.

    row, col, *_ = sketch.sketch_pairs(sk, min_jaccard=0.05)
    keep, score, stats = align.verify_align_pairs(tok, chars, offsets, row, col, matrix=S, gap_open=11, gap_extend=1, min_identity=0.3, min_coverage=0.8)
    labels = sketch.cluster_pairs(row[keep], col[keep], B)

* `stats_pairs`, `stats_pairs_host`, `stats_kernel_name`    (score, stats): stats[k] = (start_a, start_b, end_a, end_b, matches, columns);
* `stats_identity`, `stats_coverage`    matches / columns (or / a length), (end - start) / length, float32;
* `verify_align_pairs`, `verify_align_pairs_host`    (keep, score, stats): identity and coverage thresholds, in integers.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi

_lib = capi.load()

TOO_LONG, BAD_INDEX = -1, -2
MAX_LEN = 4096
_FORM_HOLDS = {1: 256, 2: 1024, 3: 4096}


def _edit(tok, max_len, form, holds=_FORM_HOLDS):
    """(desc, bsq_edit) with the library's argument rules applied as ValueError (no device is touched).  holds: the longest shorter side
    that each of the forms 1, 2, 3 holds in the family that asks (the statistics kernels hold half of what the others do)."""
    desc = capi.desc_of(tok)
    if not 1 <= desc.nchars <= 30:
        raise ValueError("the edit distance takes alphabets of 1 .. 30 classes, %r has %d" % (tok.key, desc.nchars))
    max_len = capi.int_arg("max_len", max_len, 1, holds[3])
    form = 0 if form is None else form
    if isinstance(form, bool) or form not in (0, 1, 2, 3) or (form and holds[form] < max_len):
        raise ValueError("form must be None or 1, 2, 3 (shorter sides up to %d, %d, %d), got %r at max_len %d"
                         % (holds[1], holds[2], holds[3], form, max_len))
    e = capi.Edit(max_len, int(form))
    if not _lib.bsq_edit_pairs_kernel_name(ctypes.byref(e)):  # (whatever the rules above do not restate)
        raise ValueError("the library refuses these arguments (include/bsq.h, \"edit distance of row pairs\")")
    return desc, e


def edit_kernel_name(max_len=MAX_LEN, form=None):
    """The kernel `edit_distance_pairs` takes (host only: profiling labels, tests)."""
    e = capi.Edit(int(max_len), 0 if form is None else int(form))
    return _lib.bsq_edit_pairs_kernel_name(ctypes.byref(e)).decode()


def _pairs_host(entry, desc, rule, chars, offsets, row, col, chars_b, offsets_b, *outs):
    """One call of a CPU twin over listed pairs of rows of two stores -- of one store where chars_b and offsets_b are None.  Every
    output is described by (numpy dtype, shape behind the list's length), or by None where it was not asked for: that one is returned
    as None and goes to the library as a null pointer.  Returns the outputs in order.  An empty list makes no call."""
    if (chars_b is None) != (offsets_b is None):
        raise ValueError("chars_b and offsets_b come together")
    row, col = capi.host_index_lists(row, col)
    ca, oa = capi.host_batch(chars, offsets)
    cb, ob = (ca, oa) if chars_b is None else capi.host_batch(chars_b, offsets_b)
    n = row.size
    out = [None if o is None else np.empty((n,) + o[1], o[0]) for o in outs]
    if n:
        capi.check(entry(ctypes.byref(desc), ca.ctypes.data, oa.ctypes.data, oa.size - 1, cb.ctypes.data, ob.ctypes.data, ob.size - 1,
                         row.ctypes.data, col.ctypes.data, n, ctypes.byref(rule), *[None if x is None else x.ctypes.data for x in out]))
    return out


_ON_DEVICE = "the pair calls work on packed batches resident on the device (chars, offsets tensors)"


def _stores_on_device(chars, offsets, row, col, chars_b, offsets_b):
    """What the three device calls check before they allocate: (Ba, Bb, device, n) of stores and lists resident on one device.  The
    allocations and the launch stay written out in each of them: one shared call path over described outputs cost score_pairs
    0.5 us a call (profiles/r31/pair_surface_refactor.txt)."""
    if (chars_b is None) != (offsets_b is None):
        raise ValueError("chars_b and offsets_b come together")
    Ba = capi.packed_on_device(chars, offsets, _ON_DEVICE)
    Bb = Ba if chars_b is None else capi.packed_on_device(chars_b, offsets_b, _ON_DEVICE)
    if chars_b is not None and chars_b.device != chars.device:
        raise ValueError("both stores must live on one device")
    return Ba, Bb, capi.device_index_lists(row, col, chars.device), row.numel()


def edit_distance_host(tok, chars, offsets, row, col, chars_b=None, offsets_b=None, *, max_len=MAX_LEN, form=None):
    """The library's CPU twin (`bsq_edit_pairs_host`: the class and block-step text of the kernels in plain loops) on numpy arrays:
    dist as an int32 array, with `edit_distance_pairs`' meaning of every argument (form is checked and changes nothing)."""
    desc, e = _edit(tok, max_len, form)
    dist, = _pairs_host(_lib.bsq_edit_pairs_host, desc, e, chars, offsets, row, col, chars_b, offsets_b, (np.int32, ()))
    return dist


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
    Ba, Bb, dev, n = _stores_on_device(chars, offsets, row, col, chars_b, offsets_b)
    dist = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        ca = capi.readable_chars(chars, dev)  # (every row may be empty)
        cb = ca if chars_b is None else capi.readable_chars(chars_b, dev)
        ob = offsets if offsets_b is None else offsets_b
        with capi.launching(dev) as stream:
            capi.check(_lib.bsq_edit_pairs_device(ctypes.byref(desc), ca.data_ptr(), offsets.data_ptr(), Ba, cb.data_ptr(), ob.data_ptr(), Bb,
                                                  row.data_ptr(), col.data_ptr(), n, ctypes.byref(e), dist.data_ptr(), stream))
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
    T = capi.q16_arg("min_identity", min_identity)
    dist = edit_distance_host(tok, chars, offsets, row, col, chars_b, offsets_b, max_len=max_len)
    row, col = capi.host_index_lists(row, col)
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
    T = capi.q16_arg("min_identity", min_identity)
    dist = edit_distance_pairs(tok, chars, offsets, row, col, chars_b, offsets_b, max_len=max_len)
    L = torch.maximum(_valid_lengths(torch, offsets, row), _valid_lengths(torch, offsets if offsets_b is None else offsets_b, col))
    return (dist >= 0) & (dist.to(torch.int64) * 65536 <= (65536 - T) * L), dist


# ---- scored alignment of row pairs (include/bsq.h, "scored alignment of row pairs")

SCORE_TOO_LONG, SCORE_BAD_INDEX = -2**31 + 1, -2**31 + 2
CODE_BELOW = -2**30  # every score <= this is a code
_MODES = {"local": 0, "global": 1}
_BLOSUM_LETTERS = "ARNDCQEGHILKMFPSTWYV"


def score_matrix(tok, match, mismatch):
    """The (C + 1, C + 1) int8 matrix with `match` where two classes are equal (the unmapped class against itself included) and
    `mismatch` elsewhere; C is the number of classes of the tokenizer's alphabet."""
    C = capi.desc_of(tok).nchars
    match, mismatch = capi.int_arg("match", match, -128, 127), capi.int_arg("mismatch", mismatch, -128, 127)
    m = np.full((C + 1, C + 1), mismatch, np.int8)
    np.fill_diagonal(m, match)
    return m


def blosum62_matrix(tok):
    """BLOSUM62 over the tokenizer's classes as a (21, 21) int8 matrix: the 20 letters on the classes the tokenizer gives them, the
    unmapped class on the X row and column (X / X = -1).  ValueError unless the alphabet has 20 classes and the letters land on 20
    distinct ones."""
    desc = capi.desc_of(tok)
    cls = [desc.lut[ord(c)] for c in _BLOSUM_LETTERS]
    if desc.nchars != 20 or min(cls) < 0 or len(set(cls)) != 20:
        raise ValueError("blosum62_matrix needs an alphabet whose 20 classes are the 20 amino acids, got %r" % (tok.key,))
    raw = np.zeros((21, 21), np.int8)
    capi.check(_lib.bsq_blosum62_scores(raw.ctypes.data))
    at = np.array(cls + [20])
    out = np.empty((21, 21), np.int8)
    out[np.ix_(at, at)] = raw
    return out


def _score(tok, matrix, gap_open, gap_extend, mode, max_len, form, holds=_FORM_HOLDS):
    """(desc, bsq_score) with the library's argument rules applied as ValueError (no device is touched); holds: as for `_edit`."""
    desc, e = _edit(tok, max_len, form, holds)
    if mode not in _MODES:
        raise ValueError("mode is 'local' or 'global', got %r" % (mode,))
    for name, v in (("gap_open", gap_open), ("gap_extend", gap_extend)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 127:
            raise ValueError("%s must be an integer in 0 .. 127, got %r" % (name, v))
    m = np.asarray(matrix)
    C = desc.nchars + 1
    if m.dtype.kind not in "iu" or m.shape != (C, C) or m.min() < -128 or m.max() > 127:
        raise ValueError("matrix is a (%d, %d) integer array of int8 values (classes of %r and the unmapped one)" % (C, C, tok.key))
    s = capi.Score(e.max_len, e.form, _MODES[mode], int(gap_open), int(gap_extend))
    np.ctypeslib.as_array(s.matrix)[:C, :C] = m.astype(np.int8)
    if not _lib.bsq_score_pairs_kernel_name(ctypes.byref(s), 0):  # (whatever the rules above do not restate)
        raise ValueError("the library refuses these arguments (include/bsq.h, \"scored alignment of row pairs\")")
    return desc, s


def score_kernel_name(*, mode="local", ends=False, max_len=MAX_LEN, form=None, gap_open=0, gap_extend=0):
    """The kernel `score_pairs` takes (host only: profiling labels, tests); "" for what the library refuses."""
    s = capi.Score(int(max_len), 0 if form is None else int(form), _MODES.get(mode, -1), int(gap_open), int(gap_extend))
    return _lib.bsq_score_pairs_kernel_name(ctypes.byref(s), int(bool(ends))).decode()


def score_pairs_host(tok, chars, offsets, row, col, chars_b=None, offsets_b=None, *, matrix, gap_open, gap_extend, mode="local", ends=False,
                     max_len=MAX_LEN, form=None):
    """The library's CPU twin (`bsq_score_pairs_host`: the cell of the kernels in plain loops) on numpy arrays: score as an int32
    array, or (score, ends) with ends int32 of shape (n, 2); every argument means what it means to `score_pairs`."""
    desc, s = _score(tok, matrix, gap_open, gap_extend, mode, max_len, form)
    score, en = _pairs_host(_lib.bsq_score_pairs_host, desc, s, chars, offsets, row, col, chars_b, offsets_b,
                            (np.int32, ()), (np.int32, (2,)) if ends else None)
    return (score, en) if ends else score


def score_pairs(tok, chars, offsets, row, col, chars_b=None, offsets_b=None, *, matrix, gap_open, gap_extend, mode="local", ends=False,
                max_len=MAX_LEN, form=None):
    """score[k] = the alignment score of row row[k] of the store (chars, offsets) and row col[k] of the store (chars_b, offsets_b) -- the
    same store when those are None -- by Gotoh's algorithm: an int32 device tensor on torch's current stream, one launch, nothing read
    back.  With ends=True, (score, ends) with ends int32 of shape (n, 2): (end_a, end_b) of the best cell.

    matrix[class of A's character][class of B's character] is a (C + 1, C + 1) integer array of int8 values (`score_matrix`,
    `blosum62_matrix`); a gap of L characters costs gap_open + L * gap_extend (BLAST's 11 / 1 is gap_open=11, gap_extend=1).  mode:
    "local" (Smith-Waterman: max(0, best cell); ends of the first best cell, smallest end_a then end_b, (0, 0) for score 0) or
    "global" (Needleman-Wunsch; ends (la, lb)).  Stores, lists, max_len and form as for `edit_distance_pairs`; the longer side may
    have up to 2^20 characters.  Codes: `SCORE_TOO_LONG`, `SCORE_BAD_INDEX` (every score <= `CODE_BELOW` is one), ends (-1, -1)."""
    import torch
    desc, s = _score(tok, matrix, gap_open, gap_extend, mode, max_len, form)
    Ba, Bb, dev, n = _stores_on_device(chars, offsets, row, col, chars_b, offsets_b)
    score = torch.empty(n, dtype=torch.int32, device=dev)
    en = torch.empty((n, 2), dtype=torch.int32, device=dev) if ends else None
    if n:
        ca = capi.readable_chars(chars, dev)  # (every row may be empty)
        cb = ca if chars_b is None else capi.readable_chars(chars_b, dev)
        ob = offsets if offsets_b is None else offsets_b
        with capi.launching(dev) as stream:
            capi.check(_lib.bsq_score_pairs_device(ctypes.byref(desc), ca.data_ptr(), offsets.data_ptr(), Ba, cb.data_ptr(), ob.data_ptr(), Bb,
                                                   row.data_ptr(), col.data_ptr(), n, ctypes.byref(s), score.data_ptr(),
                                                   en.data_ptr() if ends else None, stream))
    return (score, en) if ends else score


def self_scores(tok, chars, offsets, matrix):
    """The score of every row against itself with no gap -- the sum of matrix[c][c] over the row's classes -- as int64: in torch on the
    device for tensors (class table -> diagonal -> cumulative sum -> difference at the offsets, nothing read back), in numpy for arrays."""
    desc = capi.desc_of(tok)
    m = np.asarray(matrix)
    if m.shape != (desc.nchars + 1, desc.nchars + 1):
        raise ValueError("matrix is a (%d, %d) array" % (desc.nchars + 1, desc.nchars + 1))
    lut = np.array(list(desc.lut), np.int64)
    per_byte = np.diagonal(m).astype(np.int64)[np.where(lut >= 0, lut, desc.nchars)]  # the self-score of every byte value
    if isinstance(chars, np.ndarray) or not hasattr(chars, "device"):
        sums = np.concatenate([np.zeros(1, np.int64), np.cumsum(per_byte[np.asarray(chars, np.uint8).ravel()])])
        o = np.asarray(offsets, np.int64).ravel()
        return sums[o[1:]] - sums[o[:-1]]
    import torch
    table = torch.from_numpy(per_byte).to(chars.device)
    sums = torch.cat([torch.zeros(1, dtype=torch.int64, device=chars.device), torch.cumsum(table[chars.to(torch.int64)], 0)])
    return sums[offsets[1:]] - sums[offsets[:-1]]


def _valid_take(xp, values, idx):
    """values[idx], 0 where idx lies outside values (numpy or torch by `xp`)."""
    if values.shape[0] == 0:
        return xp.zeros_like(idx)
    ok = (idx >= 0) & (idx < values.shape[0])
    return xp.where(ok, values[xp.where(ok, idx, xp.zeros_like(idx))], xp.zeros_like(idx))


def _score_keep(xp, score64, self_a, self_b, T, min_score):
    least = xp.minimum(self_a, self_b)
    return (score64 > CODE_BELOW) & (score64 >= min_score) & (least > 0) & (score64 * 65536 >= T * least)


def verify_score_pairs_host(tok, chars, offsets, row, col, chars_b=None, offsets_b=None, *, matrix, gap_open, gap_extend, mode="local",
                            min_ratio=0.5, min_score=1, max_len=MAX_LEN):
    """`verify_score_pairs` on numpy arrays through the CPU twin: (keep, score) as numpy arrays, the same bits."""
    T, min_score = capi.q16_arg("min_ratio", min_ratio), capi.int_arg("min_score", min_score)
    score = score_pairs_host(tok, chars, offsets, row, col, chars_b, offsets_b, matrix=matrix, gap_open=gap_open, gap_extend=gap_extend, mode=mode,
                             max_len=max_len)
    row, col = capi.host_index_lists(row, col)
    sa = self_scores(tok, np.asarray(chars, np.uint8), offsets, matrix)
    sb = sa if chars_b is None else self_scores(tok, np.asarray(chars_b, np.uint8), offsets_b, matrix)
    return _score_keep(np, score.astype(np.int64), _valid_take(np, sa, row), _valid_take(np, sb, col), T, min_score), score


def verify_score_pairs(tok, chars, offsets, row, col, chars_b=None, offsets_b=None, *, matrix, gap_open, gap_extend, mode="local",
                       min_ratio=0.5, min_score=1, max_len=MAX_LEN):
    """(keep, score) of a candidate list: score as `score_pairs` gives it, and keep[k] (bool) true when the score is no code, reaches
    min_score, and its ratio to the perfect score of the weaker row reaches min_ratio: with least = min(self_a, self_b) of
    `self_scores`, least > 0 and score * 65536 >= T * least, T = floor(min_ratio * 65536 + 0.5), in 64-bit integers, in torch on the
    device, nothing read back -- `verify_score_pairs_host` keeps the same pairs bit for bit.  `row[keep]`, `col[keep]` is the verified
    list, which `sketch.cluster_pairs` takes."""
    import torch
    T, min_score = capi.q16_arg("min_ratio", min_ratio), capi.int_arg("min_score", min_score)
    score = score_pairs(tok, chars, offsets, row, col, chars_b, offsets_b, matrix=matrix, gap_open=gap_open, gap_extend=gap_extend, mode=mode,
                        max_len=max_len)
    sa = self_scores(tok, chars, offsets, matrix)
    sb = sa if chars_b is None else self_scores(tok, chars_b, offsets_b, matrix)
    return _score_keep(torch, score.to(torch.int64), _valid_take(torch, sa, row), _valid_take(torch, sb, col), T, min_score), score


# ---- alignment statistics of row pairs (include/bsq.h, "alignment statistics of row pairs")

STATS_MAX_LEN = 2048
_STATS_FORM_HOLDS = {1: 128, 2: 512, 3: 2048}
_IDENTITY_OVER = ("columns", "shorter", "longer")
_COVERAGE = ("both", "shorter", "longer", "a", "b")


def _stats(tok, matrix, gap_open, gap_extend, mode, max_len, form):
    """(desc, bsq_score) for the statistics calls: `_score`'s rules with the narrower max_len and forms (a form that holds a max_len
    here holds it in the score kernels too, so `_score`'s own question to the library stands)."""
    desc, s = _score(tok, matrix, gap_open, gap_extend, mode, max_len, form, _STATS_FORM_HOLDS)
    if not _lib.bsq_align_stats_kernel_name(ctypes.byref(s)):  # (whatever the rules above do not restate)
        raise ValueError("the library refuses these arguments (include/bsq.h, \"alignment statistics of row pairs\")")
    return desc, s


def stats_kernel_name(*, mode="local", max_len=STATS_MAX_LEN, form=None, gap_open=0, gap_extend=0):
    """The kernel `stats_pairs` takes (host only: profiling labels, tests); "" for what the library refuses."""
    s = capi.Score(int(max_len), 0 if form is None else int(form), _MODES.get(mode, -1), int(gap_open), int(gap_extend))
    return _lib.bsq_align_stats_kernel_name(ctypes.byref(s)).decode()


def stats_pairs_host(tok, chars, offsets, row, col, chars_b=None, offsets_b=None, *, matrix, gap_open, gap_extend, mode="local",
                     max_len=STATS_MAX_LEN, form=None):
    """The library's CPU twin (`bsq_align_stats_host`: the cell of the kernels in plain loops) on numpy arrays: (score int32, stats int32
    of shape (n, 6)); every argument means what it means to `stats_pairs`."""
    desc, s = _stats(tok, matrix, gap_open, gap_extend, mode, max_len, form)
    score, stats = _pairs_host(_lib.bsq_align_stats_host, desc, s, chars, offsets, row, col, chars_b, offsets_b, (np.int32, ()), (np.int32, (6,)))
    return score, stats


def stats_pairs(tok, chars, offsets, row, col, chars_b=None, offsets_b=None, *, matrix, gap_open, gap_extend, mode="local",
                max_len=STATS_MAX_LEN, form=None):
    """(score, stats) of the listed pairs: score exactly as `score_pairs` gives it, and stats int32 of shape (n, 6), the row
    (start_a, start_b, end_a, end_b, matches, columns) of one optimal alignment that ends in the best cell -- device tensors on torch's
    current stream, one launch, nothing read back.

    The alignment covers A's characters [start_a, end_a) and B's [start_b, end_b); `matches` of its `columns` columns (gap columns
    included) pair characters of one class.  Global mode: starts (0, 0), ends (la, lb).  A local score of 0 gives six zeros, a code six
    times -1.  Stores, lists, matrix, gap costs and mode as for `score_pairs`; max_len is 1 .. 2048 here (the kernel keeps three times
    the state per row) and form 1, 2, 3 holds shorter sides up to 128, 512, 2048.  `stats_identity`, `stats_coverage` and
    `verify_align_pairs` turn the statistics into the thresholds of cd-hit and mmseqs."""
    import torch
    desc, s = _stats(tok, matrix, gap_open, gap_extend, mode, max_len, form)
    Ba, Bb, dev, n = _stores_on_device(chars, offsets, row, col, chars_b, offsets_b)
    score = torch.empty(n, dtype=torch.int32, device=dev)
    stats = torch.empty((n, 6), dtype=torch.int32, device=dev)
    if n:
        ca = capi.readable_chars(chars, dev)  # (every row may be empty)
        cb = ca if chars_b is None else capi.readable_chars(chars_b, dev)
        ob = offsets if offsets_b is None else offsets_b
        with capi.launching(dev) as stream:
            capi.check(_lib.bsq_align_stats_device(ctypes.byref(desc), ca.data_ptr(), offsets.data_ptr(), Ba, cb.data_ptr(), ob.data_ptr(), Bb,
                                                   row.data_ptr(), col.data_ptr(), n, ctypes.byref(s), score.data_ptr(), stats.data_ptr(), stream))
    return score, stats


def _ratio32(xp, num, den, bad):
    """num / den as float32 (computed in float64), NaN where `bad` or den <= 0."""
    if xp is np:
        out = np.full(num.shape, np.nan, np.float64)
        ok = ~bad & (den > 0)
        out[ok] = num[ok].astype(np.float64) / den[ok].astype(np.float64)
        return out.astype(np.float32)
    ok = ~bad & (den > 0)
    q = num.to(xp.float64) / xp.where(ok, den, xp.ones_like(den)).to(xp.float64)
    return xp.where(ok, q, xp.full_like(q, float("nan"))).to(xp.float32)


def stats_identity(stats, over="columns", la=None, lb=None):
    """matches / D as float32: D = the alignment's columns (over="columns", BLAST's identity), or min(la, lb) ("shorter", cd-hit's) or
    max(la, lb) ("longer") with la and lb from `pair_lengths`.  NaN for a pair with a code and where D is 0.  numpy or torch by `stats`."""
    if over not in _IDENTITY_OVER:
        raise ValueError("over is one of %r, got %r" % (_IDENTITY_OVER, over))
    if over != "columns" and (la is None or lb is None):
        raise ValueError("over=%r needs la and lb (pair_lengths)" % (over,))
    xp = capi.xp_of(stats)
    st = stats.astype(np.int64) if xp is np else stats.to(xp.int64)
    den = st[:, 5] if over == "columns" else (xp.minimum(la, lb) if over == "shorter" else xp.maximum(la, lb))
    return _ratio32(xp, st[:, 4], den, st[:, 5] < 0)


def stats_coverage(stats, la, lb):
    """(cov_a, cov_b): the share of each row the alignment covers, (end - start) / length as float32; NaN for a code and a length of 0."""
    xp = capi.xp_of(stats)
    st = stats.astype(np.int64) if xp is np else stats.to(xp.int64)
    bad = st[:, 5] < 0
    return _ratio32(xp, st[:, 2] - st[:, 0], la, bad), _ratio32(xp, st[:, 3] - st[:, 1], lb, bad)


def _align_thresholds(min_identity, min_coverage, identity_over, coverage, min_score):
    if identity_over not in ("columns", "shorter"):
        raise ValueError("identity_over is 'columns' or 'shorter', got %r" % (identity_over,))
    if coverage not in _COVERAGE:
        raise ValueError("coverage is one of %r, got %r" % (_COVERAGE, coverage))
    Tc, min_score = capi.q16_arg("min_coverage", min_coverage), capi.int_arg("min_score", min_score)
    return capi.q16_arg("min_identity", min_identity), Tc, min_score


def _align_keep(xp, score64, st, la, lb, Ti, Tc, min_score, identity_over, coverage):
    """The rule of `verify_align_pairs` on int64 arrays (numpy or torch by `xp`)."""
    D = st[:, 5] if identity_over == "columns" else xp.minimum(la, lb)
    keep = (score64 > CODE_BELOW) & (score64 >= min_score) & (D > 0) & (st[:, 4] * 65536 >= Ti * D)
    ok_a, ok_b = (st[:, 2] - st[:, 0]) * 65536 >= Tc * la, (st[:, 3] - st[:, 1]) * 65536 >= Tc * lb
    a_short = la <= lb  # (A's row is the shorter one when the lengths are equal, as in the kernels)
    if coverage == "both":
        cov = ok_a & ok_b
    elif coverage == "a":
        cov = ok_a
    elif coverage == "b":
        cov = ok_b
    elif coverage == "shorter":
        cov = xp.where(a_short, ok_a, ok_b)
    else:
        cov = xp.where(a_short, ok_b, ok_a)
    return keep & cov


def verify_align_pairs_host(tok, chars, offsets, row, col, chars_b=None, offsets_b=None, *, matrix, gap_open, gap_extend, mode="local",
                            min_identity=0.9, min_coverage=0.8, identity_over="columns", coverage="both", min_score=1, max_len=STATS_MAX_LEN):
    """`verify_align_pairs` on numpy arrays through the CPU twin: (keep, score, stats) as numpy arrays, the same bits."""
    Ti, Tc, min_score = _align_thresholds(min_identity, min_coverage, identity_over, coverage, min_score)
    score, stats = stats_pairs_host(tok, chars, offsets, row, col, chars_b, offsets_b, matrix=matrix, gap_open=gap_open, gap_extend=gap_extend,
                                    mode=mode, max_len=max_len)
    row, col = capi.host_index_lists(row, col)
    oa = np.asarray(offsets, np.int64).ravel()
    ob = oa if offsets_b is None else np.asarray(offsets_b, np.int64).ravel()
    la, lb = _valid_lengths(np, oa, row), _valid_lengths(np, ob, col)
    return _align_keep(np, score.astype(np.int64), stats.astype(np.int64), la, lb, Ti, Tc, min_score, identity_over, coverage), score, stats


def verify_align_pairs(tok, chars, offsets, row, col, chars_b=None, offsets_b=None, *, matrix, gap_open, gap_extend, mode="local",
                       min_identity=0.9, min_coverage=0.8, identity_over="columns", coverage="both", min_score=1, max_len=STATS_MAX_LEN):
    """(keep, score, stats) of a candidate list: score and stats as `stats_pairs` gives them, and keep[k] (bool) true when the pair
    passes the thresholds protein clustering tools publish -- sequence identity over the alignment and coverage of the rows by it:

    * the score is no code and reaches min_score;
    * matches * 65536 >= Ti * D and D > 0, D = columns (identity_over="columns", `mmseqs --min-seq-id`) or min(la, lb) ("shorter",
      `cd-hit -c`), Ti = floor(min_identity * 65536 + 0.5);
    * (end - start) * 65536 >= Tc * length, Tc likewise from min_coverage, for the rows `coverage` names: "both" (`mmseqs -c` in its
      default coverage mode), "shorter", "longer" (A's row is the shorter one when the lengths are equal), "a" or "b".

    Decided in 64-bit integers, in torch on the device, nothing read back: `verify_align_pairs_host` keeps the same pairs bit for bit.
    `row[keep]`, `col[keep]` is the verified list, which `sketch.cluster_pairs` takes."""
    import torch
    Ti, Tc, min_score = _align_thresholds(min_identity, min_coverage, identity_over, coverage, min_score)
    score, stats = stats_pairs(tok, chars, offsets, row, col, chars_b, offsets_b, matrix=matrix, gap_open=gap_open, gap_extend=gap_extend, mode=mode,
                               max_len=max_len)
    la, lb = _valid_lengths(torch, offsets, row), _valid_lengths(torch, offsets if offsets_b is None else offsets_b, col)
    return _align_keep(torch, score.to(torch.int64), stats.to(torch.int64), la, lb, Ti, Tc, min_score, identity_over, coverage), score, stats


__all__ = ["TOO_LONG", "BAD_INDEX", "MAX_LEN", "edit_distance_pairs", "edit_distance_host", "edit_kernel_name", "pair_lengths", "pair_identity",
           "verify_pairs", "verify_pairs_host", "SCORE_TOO_LONG", "SCORE_BAD_INDEX", "CODE_BELOW", "score_matrix", "blosum62_matrix", "score_pairs",
           "score_pairs_host", "score_kernel_name", "self_scores", "verify_score_pairs", "verify_score_pairs_host", "STATS_MAX_LEN", "stats_pairs",
           "stats_pairs_host", "stats_kernel_name", "stats_identity", "stats_coverage", "verify_align_pairs", "verify_align_pairs_host"]
