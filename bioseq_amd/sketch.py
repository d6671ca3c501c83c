"""MinHash sketches of packed batches and the all-pairs similarity of sketches, on the device (`bsq_minhash_device`,
`bsq_sketch_compare_device`): what a training set is checked with for near-duplicates and train / test leakage without going back to
the host.

A sketch is one fixed-width row of `buckets` values per sequence: every window of `k` characters (k = 21 for nucleotides, about 7 to 14
for proteins; any alphabet of the package with `nchars ** k <= 2 ** 64`) is hashed, the hash picks a bucket, and the bucket keeps the
smallest value that fell into it (one-permutation MinHash; `EMPTY` = -1 marks a bucket nothing fell into).  Two sequences that share a
fraction J of their k-mers agree in about that fraction of their non-empty buckets.  include/bsq.h ("MinHash sketch") has the rule.

* `minhash_packed`    the (B, buckets) sketches of a packed batch resident on the device, one launch;
* `minhash_host`, `minhash_kernel_name`    the library's CPU twin (numpy), the kernel taken;
* `sketch_compare`    `match` and `either` counts of every pair of rows of two sketch matrices, (Ba, Bb) int32, one launch -- no
                      `Ba * Bb * buckets` boolean tensor;
* `sketch_compare_host`    its CPU twin;
* `sketch_jaccard`    match / either as float32, 0 where either == 0;
* `sketch_pairs`      the pairs of rows at least `min_jaccard` similar as an ordered list (row, col, match, either, pair_offsets) --
                      the comparison's arithmetic with a ragged output, so a store of 262 144 sketches is searched against itself
                      without the 550 GB its dense matrices would take (`bsq_sketch_pairs_count_device`, `bsq_sketch_pairs_emit_device`;
                      include/bsq.h, "sketch pairs");
* `sketch_pairs_host`, `sketch_pairs_kernel_name`    its CPU twin, its launches;
* `sketch_duplicates`  (keep, first) from the pair list of a matrix with itself: every row with an earlier near-duplicate is dropped;
* `sketch_clusters`   the single-linkage clusters of a matrix as one int64 label per row -- the connected components of the pairs that
                      pass, by a lock-free union-find inside the comparison's tile walk, with no pair list (`bsq_sketch_clusters_device`;
                      include/bsq.h, "sketch clusters");
* `cluster_pairs`     the same labels from an explicit edge list (`bsq_cluster_pairs_device`): merged lists, pairs from elsewhere;
* `sketch_clusters_host`, `cluster_pairs_host`, `sketch_clusters_kernel_name`    their CPU twins, the launches;
* `cluster_table`, `cluster_split`    (representatives, sizes, dense ids) of a label array; a seeded split in which every cluster goes to
                      one side whole;
* `greedy_pairs`      greedy representatives of an edge list (cd-hit's rule: visit the nodes longest first, keep a node unless an
                      earlier kept node is linked to it): rep[i] per node, no two kept nodes linked, every dropped node linked to a kept
                      one (`bsq_greedy_pairs_device`; include/bsq.h, "greedy representatives");
* `greedy_pairs_host`, `greedy_kernel_name`, `length_key`    its CPU twin, its launches, the "longest first" key of a packed batch;
* `lsh_pairs`         the pair list without the all-pairs comparison: banded LSH over the sketch rows -- rows that agree on a whole band of
                      `rows_per_band` buckets are candidates, and only candidates are compared -- so the cost follows the rows and the
                      candidates, not Ba x Bb (`bsq_lsh_keys_device`, `bsq_lsh_count_device`, `bsq_lsh_emit_device`,
                      `bsq_sketch_compare_list_device`; include/bsq.h, "LSH candidates of a sketch matrix");
* `lsh_candidates`, `lsh_keys`, `sketch_compare_list`    its parts: the candidates before any threshold, the band keys, `match` and
                      `either` of a GIVEN list of pairs (rescoring a list from elsewhere or from a narrower sketch);
* `lsh_keys_host`, `sketch_compare_list_host`, `lsh_kernel_name`    their CPU twins, the launches;
* `lsh_recall`, `lsh_rows_per_band`    the predicted recall of a banding and the choice of `rows_per_band` for a threshold.

The sketch of a sequence equals the bucket-wise UNSIGNED minimum of the sketches of pieces that together cover all its windows (EMPTY
is the largest value), so sketches of longer sequences, or of sets of sequences, are merged without the characters.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi

_lib = capi.load()

EMPTY = -1
_MAX_WINDOWS = 1 << 30  # (include/bsq.h, "MinHash sketch": a row sketches its first 2 ** 30 windows)
_NUMPY = {capi.I32: np.int32, capi.U64: np.uint64}


def _minhash(tok, k, buckets, destchar, canonical, seed, form, total_chars=0):
    """(desc, bsq_minhash, dtype code, torch dtype) with the library's argument rules applied as ValueError (no device is touched)."""
    desc = capi.desc_of(tok)
    k, buckets = int(k), int(buckets)
    if not 1 <= k <= 32 or desc.nchars ** k > 2 ** 64:
        raise ValueError("k = %r with %d classes: k must lie in 1 .. 32 and nchars ** k within 2 ** 64" % (k, desc.nchars))
    if not 1 <= buckets <= 1 << 14:
        raise ValueError("buckets must lie in 1 .. 2 ** 14, got %r" % (buckets,))
    dt, tdt = capi.destchar_arg(destchar, (capi.I32, capi.U64), "a sketch takes 'i' (int32) or 'q' (int64)")
    if canonical and not capi.has_strands(desc):
        raise ValueError("canonical needs an alphabet with strands: the four classes A, C, G, T = 0, 1, 2, 3 (DNA, DNA4), not %r" % (tok.key,))
    form = 0 if form is None else int(form)
    if form not in (0, 1, 2) or (form == 1 and buckets > 1024):
        raise ValueError("form must be None, 1 (a wave per row: buckets <= 1024) or 2 (a workgroup per row), got %r at %d buckets" % (form, buckets))
    m = capi.MinHash(k, buckets, int(bool(canonical)), form, int(seed) & (2 ** 64 - 1), int(total_chars), 0)
    if not _lib.bsq_minhash_kernel_name(ctypes.byref(desc), ctypes.byref(m), 0, dt):  # (whatever the rules above do not restate)
        raise ValueError("the library refuses these sketch arguments (include/bsq.h, \"MinHash sketch\")")
    return desc, m, dt, tdt


def minhash_kernel_name(tok, k, B, buckets=1024, destchar="i", *, canonical=False, form=None, total_chars=0):
    """The kernel `minhash_packed` takes (host only: profiling labels, tests); total_chars: `chars.numel()` of the call, 0 = unknown."""
    desc, m, dt, _ = _minhash(tok, k, buckets, destchar, canonical, 0, form, total_chars)
    return _lib.bsq_minhash_kernel_name(ctypes.byref(desc), ctypes.byref(m), int(B), dt).decode()


def minhash_host(tok, chars, offsets, k, buckets=1024, destchar="i", *, canonical=False, seed=0):
    """The library's CPU twin (`bsq_minhash_host`, the word, hash and element code of the kernels) on numpy arrays: a (B, buckets) matrix,
    int32 for 'i' and uint64 for 'q' (EMPTY = all bits set: -1 as a signed value)."""
    desc, m, dt, _ = _minhash(tok, k, buckets, destchar, canonical, seed, None)
    chars, offsets = capi.host_batch(chars, offsets)
    B = offsets.size - 1
    out = np.empty((B, m.buckets), dtype=_NUMPY[dt])
    if B > 0:
        capi.check(_lib.bsq_minhash_host(ctypes.byref(desc), chars.ctypes.data, offsets.ctypes.data, B, ctypes.byref(m), dt, out.ctypes.data))
    return out


def minhash_packed(tok, chars, offsets, k, buckets=1024, destchar="i", *, canonical=False, seed=0, form=None, validate=True):
    """The MinHash sketches of a packed batch on the device (chars uint8[total], offsets int64[B + 1]): a (B, buckets) device tensor on
    torch's current stream, one launch, nothing read back.

    out[i, s] = the smallest hash value of the windows of k characters of row i that fall into bucket s, `EMPTY` (-1) where none does; a
    window with an unmapped character counts nowhere.  destchar 'i': int32 holding the 32 bits (compare as unsigned), 'q': int64 holding
    0 .. 2 ** 32 - 2.  canonical (DNA, DNA4): a window and its reverse complement hash alike, so a row and its reverse complement have
    equal sketches.  seed: another hash family.  form: None = the library chooses from `chars.numel()` / B, 1 = a wave per row
    (buckets <= 1024), 2 = a workgroup per row.  validate: malformed offsets and a row of more than 2 ** 30 windows raise the library's
    errors instead of being clamped."""
    B = capi.packed_on_device(chars, offsets, "minhash_packed works on packed batches resident on the device (chars, offsets tensors)")
    desc, m, dt, tdt = _minhash(tok, k, buckets, destchar, canonical, seed, form, chars.numel())
    return capi._row_table_packed(chars, offsets, B, m.buckets, tdt, _MAX_WINDOWS - 1 + m.k if validate else None, lambda src, out, stream:
                                  _lib.bsq_minhash_device(ctypes.byref(desc), src, offsets.data_ptr(), B, ctypes.byref(m), dt, out, stream))


def _pair_shape(a, b):
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1] or a.dtype != b.dtype:
        raise ValueError("sketch matrices are 2-D, of one element type and one width; got %r %s and %r %s" % (tuple(a.shape), a.dtype, tuple(b.shape), b.dtype))
    if not 1 <= a.shape[1] <= 1 << 14:
        raise ValueError("sketches are 1 .. 2 ** 14 buckets wide, got %d" % a.shape[1])
    return int(a.shape[0]), int(b.shape[0]), int(a.shape[1])


_HOST_CODES = {np.dtype(np.int32): capi.I32, np.dtype(np.int64): capi.U64, np.dtype(np.uint64): capi.U64}


def _host_sketches(a, b=None):
    """contiguous numpy matrices of one accepted element type and width: (a, b or None, Ba, Bb, S, dtype code); Bb = 0 without b"""
    a = np.ascontiguousarray(a)
    b = None if b is None else np.ascontiguousarray(b)
    if a.dtype not in _HOST_CODES:
        raise ValueError("sketches are int32, int64 or uint64, got %s" % a.dtype)
    Ba, Bb, S = _pair_shape(a, a if b is None else b)
    return a, b, Ba, Bb if b is not None else 0, S, _HOST_CODES[a.dtype]


def _device_sketches(a, b, what):
    """device matrices of one accepted element type, width and device: (Ba, Bb, S, dtype code); Bb = 0 without b"""
    import torch
    other = a if b is None else b
    if not (isinstance(a, torch.Tensor) and isinstance(other, torch.Tensor) and a.is_cuda and other.is_cuda and a.device == other.device):
        raise ValueError("%s works on sketch matrices resident on one device (numpy matrices go through the CPU twin)" % what)
    if a.dtype not in (torch.int32, torch.int64) or not a.is_contiguous() or not other.is_contiguous():
        raise ValueError("sketches are contiguous int32 or int64 tensors")
    Ba, Bb, S = _pair_shape(a, other)
    return Ba, Bb if b is not None else 0, S, capi.I32 if a.dtype == torch.int32 else capi.U64


def sketch_compare_host(a, b=None, *, either=True):
    """The library's CPU twin of `sketch_compare` (`bsq_sketch_compare_host`) on numpy matrices of int32, int64 or uint64: (match,
    either or None), int32 (Ba, Bb)."""
    a, b, Ba, Bb, S, dt = _host_sketches(a, b)
    if b is None:
        b, Bb = a, Ba
    match = np.empty((Ba, Bb), np.int32)
    eith = np.empty((Ba, Bb), np.int32) if either else None
    if Ba and Bb:
        capi.check(_lib.bsq_sketch_compare_host(a.ctypes.data, Ba, b.ctypes.data, Bb, S, dt, match.ctypes.data,
                                                eith.ctypes.data if either else None))
    return match, eith


def sketch_compare(a, b=None, *, either=True):
    """All pairs of rows of two sketch matrices on the device: (match, either or None), int32 (Ba, Bb) device tensors on torch's current
    stream, one launch.  a (Ba, S), b (Bb, S): contiguous int32 or int64 device tensors as `minhash_packed` returns them; b = None
    compares a with itself.

    match[i, j] = the buckets in which a[i] and b[j] hold the same non-EMPTY value; either[i, j] = the buckets that are non-EMPTY in a[i]
    or in b[j].  match / either estimates the Jaccard similarity of the two rows' k-mer sets (`sketch_jaccard`)."""
    import torch
    Ba, Bb, S, dt = _device_sketches(a, b, "sketch_compare")
    if b is None:
        b, Bb = a, Ba
    match = torch.empty((Ba, Bb), dtype=torch.int32, device=a.device)
    eith = torch.empty((Ba, Bb), dtype=torch.int32, device=a.device) if either else None
    if Ba and Bb:
        with capi.launching(a.device) as stream:
            capi.check(_lib.bsq_sketch_compare_device(a.data_ptr(), Ba, b.data_ptr(), Bb, S, dt, match.data_ptr(),
                                                      eith.data_ptr() if either else None, stream))
    return match, eith


def sketch_jaccard(a, b=None):
    """The Jaccard estimate of every pair of rows: float32 (Ba, Bb), match / either of `sketch_compare` and 0 where either == 0 -- the
    division of the exact integers.  Device tensors give a device tensor; numpy matrices go through the CPU twin and give numpy."""
    xp = capi.xp_of(a)
    if xp is np:
        m, e = sketch_compare_host(a, b)
        return np.where(e > 0, m.astype(np.float32) / np.maximum(e, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    m, e = sketch_compare(a, b)
    return xp.where(e > 0, m.to(xp.float32) / e.clamp(min=1).to(xp.float32), xp.zeros((), dtype=xp.float32, device=m.device))


def _pairs_rule(S, min_jaccard, min_match, max_pairs, segments, upper):
    """(bsq_sketch_pairs, max_pairs or None) with the library's argument rules applied as ValueError (no device is touched)."""
    T, min_match = capi.q16_arg("min_jaccard", min_jaccard), capi.int_arg("min_match", min_match, 0, S)  # (S: the sketch width)
    cap = capi.int_arg("max_pairs", max_pairs, 0, none=True)
    segments = capi.int_arg("segments", segments, 0, 64, none=True) or 0  # (0 has always been taken and means what None means: the library chooses)
    return capi.SketchPairs(min_match, T, int(upper), segments), cap


def sketch_pairs_host(a, b=None, *, min_jaccard=0.5, min_match=1, max_pairs=None, either=True):
    """The library's CPU twin of `sketch_pairs` (`bsq_sketch_pairs_host`) on numpy matrices of int32, int64 or uint64: (row, col, match,
    either or None, pair_offsets) as numpy arrays, with `sketch_pairs`' meaning of every argument."""
    upper = b is None
    a, b, Ba, Bb, S, dt = _host_sketches(a, b)
    if upper:
        b, Bb = a, Ba
    rule, cap = _pairs_rule(S, min_jaccard, min_match, max_pairs, None, upper)
    offs = np.zeros(Ba + 1, np.int64)

    def call(n, *arrays):  # the twin counts and lists in one call; with max_pairs = 0 it only counts and takes no arrays
        capi.check(_lib.bsq_sketch_pairs_host(a.ctypes.data, Ba, b.ctypes.data, Bb, S, dt, ctypes.byref(rule), offs.ctypes.data, n,
                                              *(None if x is None else x.ctypes.data for x in arrays)))

    if cap is None:
        call(0, None, None, None, None)
        cap = int(offs[-1])
    row, col = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
    match, eith = np.zeros(cap, np.int32), np.zeros(cap, np.int32) if either else None
    call(cap, row, col, match, eith)
    return row, col, match, eith, offs


def sketch_pairs(a, b=None, *, min_jaccard=0.5, min_match=1, max_pairs=None, either=True, segments=None):
    """The pairs of rows of two sketch matrices that are at least `min_jaccard` similar, as a list -- never the dense (Ba, Bb) matrices
    of `sketch_compare`: (row, col, match, either or None, pair_offsets), device tensors on torch's current stream.

    a (Ba, S), b (Bb, S): contiguous int32 or int64 device tensors as `minhash_packed` returns them.  The pair (i, j) is listed when
    match[i, j] >= min_match and match[i, j] / either[i, j] >= min_jaccard (decided in integers: match * 65536 >= T * either with
    T = floor(min_jaccard * 65536 + 0.5), so the CPU twin `sketch_pairs_host` selects the same pairs bit for bit).  b=None lists the pairs
    i < j of `a` with itself and computes half the tiles.  Pairs come in ascending (i, j); row and col are int64, match and either
    int32, and pair_offsets (int64, Ba + 1) is the CSR of the ranks over the rows of a: pair_offsets[-1] is the number of pairs that
    pass.  min_match=0 lets two rows without a filled bucket pass every threshold.

    max_pairs=None reads that total back (8 bytes) and sizes the arrays exactly.  max_pairs=N reads nothing back: the arrays hold N
    entries, the pairs of rank < N and zeros behind the last one, and pair_offsets[-1] > N tells later that the list was cut.
    segments: None, or 1 .. 64 to force how a strip's tiles are split over workgroups (the result does not depend on it).

    Train / test leakage: `sketch_pairs(train, test, min_jaccard=...)[1].unique()` are the test rows to drop."""
    import torch
    upper = b is None
    Ba, Bb, S, dt = _device_sketches(a, b, "sketch_pairs")
    if upper:
        b, Bb = a, Ba
    rule, cap = _pairs_rule(S, min_jaccard, min_match, max_pairs, segments, upper)
    dev = a.device
    nseg = _lib.bsq_sketch_pairs_segments(Ba, Bb, rule.segments)
    if nseg < 1:
        raise ValueError("the library refuses these sizes (include/bsq.h, \"sketch pairs\")")
    segs = torch.empty(Ba * nseg + 1, dtype=torch.int64, device=dev)
    offs = torch.empty(Ba + 1, dtype=torch.int64, device=dev)
    with capi.launching(dev) as stream:
        capi.check(_lib.bsq_sketch_pairs_count_device(a.data_ptr(), Ba, b.data_ptr(), Bb, S, dt, ctypes.byref(rule), segs.data_ptr(), offs.data_ptr(),
                                                      stream))
        if cap is None:
            n, make = int(offs[-1].item()), torch.empty
        else:  # entries at and past the total stay zero
            n, make = cap, torch.zeros
        row, col = make(n, dtype=torch.int64, device=dev), make(n, dtype=torch.int64, device=dev)
        match = make(n, dtype=torch.int32, device=dev)
        eith = make(n, dtype=torch.int32, device=dev) if either else None
        if n:
            capi.check(_lib.bsq_sketch_pairs_emit_device(a.data_ptr(), Ba, b.data_ptr(), Bb, S, dt, ctypes.byref(rule), segs.data_ptr(), n,
                                                         row.data_ptr(), col.data_ptr(), match.data_ptr(), eith.data_ptr() if either else None,
                                                         stream))
    return row, col, match, eith, offs


def sketch_duplicates(a, *, min_jaccard=0.9, min_match=1, max_pairs=None):
    """De-duplication of one sketch matrix from its pair list: (keep, first).  first[j] (int64, B) is the smallest i < j that
    `sketch_pairs(a, min_jaccard=..., min_match=...)` lists with j, or j itself; keep = first == arange(B) (bool).  `a[keep]` drops EVERY
    row that has an earlier near-duplicate: of a chain A ~ B ~ C it loses B and C even when A and C are not similar (`greedy_pairs` over
    the pair list keeps C there: every dropped row then has a kept neighbour).  A device tensor
    gives device tensors (`scatter_reduce(amin)` over the list), a numpy matrix goes through the CPU twin and gives numpy.

    max_pairs=None sizes the list exactly (one 8-byte read-back on the device) and returns (keep, first).  max_pairs=N reads nothing
    back on the device, so a cut list cannot raise there; the call then returns (keep, first, total) with `total` the number of pairs
    that pass (a 0-d tensor): where total > N the list was cut and the answer is partial -- rows may be kept that have a duplicate.
    On numpy input the total is known: a cut list raises ValueError, and the result is always (keep, first)."""
    if isinstance(a, np.ndarray):
        row, col, _, _, offs = sketch_pairs_host(a, min_jaccard=min_jaccard, min_match=min_match, max_pairs=max_pairs, either=False)
        if offs[-1] > row.size:
            raise ValueError("%d pairs pass, max_pairs = %d: the list was cut" % (offs[-1], row.size))
        first = np.arange(a.shape[0], dtype=np.int64)
        np.minimum.at(first, col, row)
        return first == np.arange(a.shape[0]), first
    import torch
    row, col, _, _, offs = sketch_pairs(a, min_jaccard=min_jaccard, min_match=min_match, max_pairs=max_pairs, either=False)
    ident = torch.arange(a.shape[0], dtype=torch.int64, device=a.device)
    first = ident.scatter_reduce(0, col, row, "amin")  # (the zeros behind a short list: first[0] <- min(0, 0))
    keep = first == ident
    return (keep, first) if max_pairs is None else (keep, first, offs[-1])


def sketch_pairs_kernel_name(Ba, Bb, segments=None):
    """The launches of `sketch_pairs` for these sizes (host only: profiling labels, tests), the count's before the ';'."""
    return _lib.bsq_sketch_pairs_kernel_name(int(Ba), int(Bb), 0 if segments is None else int(segments)).decode()


def sketch_clusters_host(a, *, min_jaccard=0.9, min_match=1):
    """The library's CPU twin of `sketch_clusters` (`bsq_sketch_clusters_host`) on a numpy matrix of int32, int64 or uint64: the int64
    labels as a numpy array."""
    a, _, B, _, S, dt = _host_sketches(a)
    rule, _ = _pairs_rule(S, min_jaccard, min_match, None, None, True)
    labels = np.empty(B, np.int64)
    if B:
        capi.check(_lib.bsq_sketch_clusters_host(a.ctypes.data, B, S, dt, ctypes.byref(rule), labels.ctypes.data))
    return labels


def sketch_clusters(a, *, min_jaccard=0.9, min_match=1, segments=None):
    """The near-duplicate clusters of one sketch matrix: labels (int64, B), labels[i] = the smallest row index that row i reaches over
    links, where rows i and j are linked when `sketch_pairs(a, min_jaccard=..., min_match=...)` would list them.  A row linked to nothing
    is its own label; `labels[labels] == labels` and `labels <= arange(B)` always hold, and `labels == arange(B)` marks one
    representative per cluster.  A device tensor (contiguous int32 or int64, as `minhash_packed` returns it) gives a device tensor on
    torch's current stream, three launches (`sketch_clusters_kernel_name`), nothing read back and no pair list at any point: a store
    that is one cluster of 100 000 rows costs what any other costs.  A numpy matrix goes through the CPU twin (`sketch_clusters_host`)
    and gives numpy; the two agree bit for bit.  segments: as in `sketch_pairs` (the result does not depend on it).

    Single linkage: this is the clustering by connected components.  Chains merge -- of A ~ B ~ C all three share one label even when
    A and C are not similar -- so the two ends of a large cluster need not resemble each other; that is what a leakage-free split wants
    (nothing similar to a test row stays in the training set) and not what a choice of representatives at a fixed radius wants.
    `sketch_duplicates` is unchanged and remains the "earliest neighbour" filter.
    `greedy_pairs` over a pair list is the choice of representatives (no two kept rows linked, every dropped row linked to a kept one).

    A train set together with a test set: `labels = sketch_clusters(torch.cat([train, test]))`, then `cluster_split(labels, ...)` for a
    new split of both, or compare `labels[:len(train)]` with `labels[len(train):]` for the clusters that straddle the old one."""
    if isinstance(a, np.ndarray):
        capi.int_arg("segments", segments, 0, 64, none=True)  # (the twin has no segments: the argument is checked all the same)
        return sketch_clusters_host(a, min_jaccard=min_jaccard, min_match=min_match)
    import torch
    B, _, S, dt = _device_sketches(a, None, "sketch_clusters")
    rule, _ = _pairs_rule(S, min_jaccard, min_match, None, segments, True)
    if _lib.bsq_sketch_pairs_segments(B, B, rule.segments) < 1:
        raise ValueError("the library refuses these sizes (include/bsq.h, \"sketch clusters\")")
    parent = torch.empty(B, dtype=torch.int64, device=a.device)
    labels = torch.empty(B, dtype=torch.int64, device=a.device)
    if B:
        with capi.launching(a.device) as stream:
            capi.check(_lib.bsq_sketch_clusters_device(a.data_ptr(), B, S, dt, ctypes.byref(rule), parent.data_ptr(), labels.data_ptr(), stream))
    return labels


_MAX_NODES, _MAX_ROUNDS = 2 ** 31 - 1, 2 ** 30 - 1  # the most nodes an edge list may join, the most rounds a greedy run may take


def cluster_pairs_host(row, col, n):
    """The library's CPU twin of `cluster_pairs` (`bsq_cluster_pairs_host`) on numpy index arrays: the int64 labels of n nodes."""
    n = capi.int_arg("n", n, 0, _MAX_NODES)
    row, col = capi.host_index_lists(row, col)
    labels = np.empty(n, np.int64)
    if n:
        capi.check(_lib.bsq_cluster_pairs_host(row.ctypes.data if row.size else None, col.ctypes.data if row.size else None, row.size, n,
                                               labels.ctypes.data))
    return labels


def cluster_pairs(row, col, n):
    """The clusters of an explicit edge list: labels (int64, n) with `sketch_clusters`' meaning, where entry k links nodes row[k] and
    col[k].  This is how lists are merged before clustering -- `torch.cat` the row and col arrays of `sketch_pairs` at several
    thresholds or sketch widths, of a train list and a train x test list with the columns offset by `len(train)`, or of pairs found
    elsewhere.  An entry with row == col is ignored (the zeros behind a list cut at `max_pairs`), and so is one with an index outside
    0 .. n - 1.  Device int64 tensors give a device tensor on torch's current stream, nothing read back; numpy arrays go through the CPU
    twin."""
    if isinstance(row, np.ndarray) and isinstance(col, np.ndarray):
        return cluster_pairs_host(row, col, n)
    import torch
    n = capi.int_arg("n", n, 0, _MAX_NODES)
    capi.device_index_lists(row, col)
    parent = torch.empty(n, dtype=torch.int64, device=row.device)
    labels = torch.empty(n, dtype=torch.int64, device=row.device)
    if n:
        with capi.launching(row.device) as stream:
            capi.check(_lib.bsq_cluster_pairs_device(row.data_ptr(), col.data_ptr(), row.numel(), n, parent.data_ptr(), labels.data_ptr(), stream))
    return labels


def sketch_clusters_kernel_name(B, segments=None):
    """The launches of `sketch_clusters` for B rows joined by '+' (host only: profiling labels, tests); '' for B = 0, which launches
    nothing, and for sizes the library refuses."""
    return _lib.bsq_sketch_clusters_kernel_name(int(B), 0 if segments is None else int(segments)).decode()


def _greedy_host_args(row, col, n, key, weight):
    n = capi.int_arg("n", n, 0, _MAX_NODES)
    row, col = capi.host_index_lists(row, col)
    if key is not None:
        key = np.ascontiguousarray(key)
        if key.dtype != np.int64 or key.shape != (n,):
            raise ValueError("key is an int64 array of n entries")
    if weight is not None:
        weight = np.ascontiguousarray(weight)
        if weight.dtype != np.int32 or weight.shape != row.shape:
            raise ValueError("weight is an int32 array of the list's length")
    return row, col, n, key, weight


def greedy_pairs_host(row, col, n, *, key=None, weight=None):
    """The library's CPU twin of `greedy_pairs` (`bsq_greedy_pairs_host`, the plain sequential visit) on numpy arrays: rep (int64, n)."""
    row, col, n, key, weight = _greedy_host_args(row, col, n, key, weight)
    rep = np.empty(n, np.int64)
    if n:
        capi.check(_lib.bsq_greedy_pairs_host(row.ctypes.data if row.size else None, col.ctypes.data if row.size else None,
                                              None if weight is None or not row.size else weight.ctypes.data, row.size, n,
                                              None if key is None else key.ctypes.data, rep.ctypes.data))
    return rep


def greedy_pairs(row, col, n, *, key=None, weight=None, max_rounds=None, rounds_per_call=16):
    """Greedy representatives of an edge list (cd-hit's rule; include/bsq.h, "greedy representatives"): rep (int64, n).  Entry k links
    nodes row[k] and col[k] (either orientation, duplicates allowed; an entry with row == col or an index outside 0 .. n - 1 is ignored,
    as in `cluster_pairs`).  Node u comes before node v when (key[u], u) < (key[v], v); key=None is index order and `length_key(offsets)`
    is "longest first".  The nodes are visited in that order and a node is kept as a representative unless one of its earlier neighbours
    is kept.  rep[i] = i for a representative; for a member, the representative neighbour before i that comes first in the order, or,
    with weight (int32, one per entry), the one whose entry has the largest weight (ties to the first in the order).  No entry joins two
    representatives, every member has an entry to rep[i], `rep[rep] == rep`, and rep serves `cluster_table` and `cluster_split` as
    labels; `rep == arange(n)` is the keep mask.  The result depends on the edges and the order alone.

    Device int64 tensors give a device tensor on torch's current stream (`bsq_greedy_pairs_device`: rounds of two launches over the
    list; random lists take about ten rounds, a path laid out in visiting order as many as it has nodes).  max_rounds=None: calls of
    `rounds_per_call` rounds, each followed by an 8-byte read-back of the count of nodes left; while it is positive the run continues
    where it stopped with twice the rounds per call; returns rep.  max_rounds=N: one call of N rounds, nothing read back; returns
    (rep, undecided) with rep[i] = -1 where node i is not decided yet, final everywhere else, and `undecided` (a 0-d tensor) the
    number of those.  numpy arrays go through the CPU twin (`greedy_pairs_host`) and give numpy -- rep, or (rep, 0) with max_rounds;
    the two agree bit for bit."""
    max_rounds = capi.int_arg("max_rounds", max_rounds, 0, _MAX_ROUNDS, none=True)
    rounds_per_call = capi.int_arg("rounds_per_call", rounds_per_call, 0, _MAX_ROUNDS)
    if rounds_per_call < 1:
        raise ValueError("rounds_per_call must be at least 1")
    if isinstance(row, np.ndarray) and isinstance(col, np.ndarray):
        rep = greedy_pairs_host(row, col, n, key=key, weight=weight)
        return rep if max_rounds is None else (rep, np.int64(0))
    import torch
    n = capi.int_arg("n", n, 0, _MAX_NODES)
    capi.device_index_lists(row, col)
    if key is not None and not (isinstance(key, torch.Tensor) and key.device == row.device and key.dtype == torch.int64 and key.shape == (n,)
                                and key.is_contiguous()):
        raise ValueError("key is a contiguous int64 tensor of n entries on the list's device")
    if weight is not None and not (isinstance(weight, torch.Tensor) and weight.device == row.device and weight.dtype == torch.int32
                                   and weight.shape == row.shape and weight.is_contiguous()):
        raise ValueError("weight is a contiguous int32 tensor of the list's length on the list's device")
    dev = row.device
    rep = torch.empty(n, dtype=torch.int64, device=dev)
    left = torch.zeros((), dtype=torch.int64, device=dev)
    if n:
        scratch = torch.empty((_lib.bsq_greedy_scratch_bytes(n, row.numel()) + 7) // 8, dtype=torch.int64, device=dev)
        done, step = 0, rounds_per_call if max_rounds is None else max_rounds
        with capi.launching(dev) as stream:
            while True:
                step = min(step, (1 << 30) - 1 - done)
                capi.check(_lib.bsq_greedy_pairs_device(row.data_ptr(), col.data_ptr(), None if weight is None else weight.data_ptr(), row.numel(), n,
                                                        None if key is None else key.data_ptr(), scratch.data_ptr(), done, step, rep.data_ptr(),
                                                        left.data_ptr(), stream))
                done += step
                if max_rounds is not None or int(left.item()) == 0:
                    break
                if step == 0:
                    raise RuntimeError("greedy_pairs: %d nodes left after 2 ** 30 - 1 rounds" % int(left.item()))
                step *= 2
    return rep if max_rounds is None else (rep, left)


def greedy_kernel_name(*, key=False, weight=False):
    """The launches `greedy_pairs` takes with or without a key and a weight (host only: profiling labels, tests): those of one round,
    then, behind the ';', those of the assignment that ends every call."""
    return _lib.bsq_greedy_kernel_name(int(bool(key)), int(bool(weight))).decode()


# ---- LSH candidates of a sketch matrix (include/bsq.h, "LSH candidates of a sketch matrix") ----

def lsh_recall(jaccard, rows_per_band, bands):
    """1 - (1 - J ** r) ** T: the chance that two rows of Jaccard similarity J share the key of at least one of T bands of r buckets.
    This is the independent-bucket approximation -- every bucket of two rows agrees with probability J, independently of the others --
    which one-permutation sketches with EMPTY buckets follow only roughly; scripts/lsh_lab.py sets the measured recall beside it.
    Pure Python."""
    j, r, t = float(jaccard), int(rows_per_band), int(bands)
    if not 0.0 <= j <= 1.0 or r < 1 or t < 0:
        raise ValueError("jaccard must lie in 0 .. 1, rows_per_band be at least 1 and bands at least 0")
    return 1.0 - (1.0 - j ** r) ** t


def lsh_rows_per_band(S, min_jaccard, recall=0.95):
    """The largest r in 1 .. S whose predicted recall `lsh_recall(min_jaccard, r, S // r)` reaches `recall` -- the fewest, widest bands
    (the fewest chance collisions) that still find that share of the pairs at the threshold; 1, the most sensitive choice, when no r
    reaches it.  Pure Python.  lsh_rows_per_band(128, 0.5) == 3: 42 bands, predicted recall 0.996 (r = 4: 0.873)."""
    S = int(S)
    if S < 1 or not 0.0 <= float(recall) <= 1.0:
        raise ValueError("S must be at least 1 and recall lie in 0 .. 1")
    good = [r for r in range(1, S + 1) if lsh_recall(min_jaccard, r, S // r) >= recall]
    return max(good) if good else 1


def _lsh_rule(S, rows_per_band, max_bucket, seed, max_candidates=None):
    """(bsq_lsh, bands) with the library's argument rules applied as ValueError (no device is touched)."""
    rows_per_band = capi.int_arg("rows_per_band", rows_per_band, 1, S)  # (S: the sketch width)
    max_bucket = capi.int_arg("max_bucket", max_bucket, 2, 2 ** 31 - 1)
    capi.int_arg("max_candidates", max_candidates, 0, none=True)
    return capi.Lsh(rows_per_band, max_bucket, int(seed) & (2 ** 64 - 1), 0), S // rows_per_band


def _lsh_width(a, b, what):
    """The width of sketch matrices of either kind, which `lsh_candidates` and `lsh_pairs` need for their rules before numpy and torch
    part ways (`_host_sketches` / `_device_sketches` then check everything else)."""
    other = a if b is None else b
    if not (hasattr(a, "ndim") and hasattr(other, "ndim")):
        raise ValueError("%s works on sketch matrices resident on one device, or on numpy matrices" % what)
    return _pair_shape(a, other)[2]


def lsh_kernel_name(S, destchar="i"):
    """The launches of the LSH family for sketches of S buckets (host only: profiling labels, tests): those of `lsh_candidates`, then,
    behind the ';', the kernel `sketch_compare_list` takes; '' for a width the library refuses."""
    dt, _ = capi.destchar_arg(destchar, (capi.I32, capi.U64), "a sketch takes 'i' (int32) or 'q' (int64)")
    return _lib.bsq_lsh_kernel_name(int(S), dt).decode()


def lsh_keys_host(a, rows_per_band, seed=0):
    """The library's CPU twin of `lsh_keys` (`bsq_lsh_keys_host`) on a numpy matrix of int32, int64 or uint64: (T, N) int64."""
    a, _, N, _, S, dt = _host_sketches(a)
    rule, T = _lsh_rule(S, rows_per_band, 2, seed)
    keys = np.empty((T, N), np.int64)
    if N:
        capi.check(_lib.bsq_lsh_keys_host(a.ctypes.data, N, S, dt, ctypes.byref(rule), keys.ctypes.data, N))
    return keys


def lsh_keys(a, rows_per_band, seed=0):
    """The band keys of a sketch matrix: (T, N) int64, T = S // rows_per_band, band-major -- keys[t, i] hashes buckets t r .. t r + r - 1
    of row i (0 .. 2 ** 63 - 1), and is -1 where all of them are EMPTY.  Two rows share a key exactly when they agree on the whole band
    (up to a 63-bit hash).  int32 and int64 sketches of one batch give equal keys; another seed gives another family.  A device tensor
    gives a device tensor on torch's current stream, one launch, nothing read back; a numpy matrix goes through the CPU twin."""
    if isinstance(a, np.ndarray):
        return lsh_keys_host(a, rows_per_band, seed)
    import torch
    N, _, S, dt = _device_sketches(a, None, "lsh_keys")
    rule, T = _lsh_rule(S, rows_per_band, 2, seed)
    keys = torch.empty((T, N), dtype=torch.int64, device=a.device)
    if N:
        with capi.launching(a.device) as stream:
            capi.check(_lib.bsq_lsh_keys_device(a.data_ptr(), N, S, dt, ctypes.byref(rule), keys.data_ptr(), N, stream))
    return keys


def sketch_compare_list_host(a, row, col, b=None, *, either=True):
    """The library's CPU twin of `sketch_compare_list` (`bsq_sketch_compare_list_host`) on numpy arrays: (match, either or None)."""
    a, b, Ba, Bb, S, dt = _host_sketches(a, b)
    row, col = capi.host_index_lists(row, col)
    n = row.size
    match = np.empty(n, np.int32)
    eith = np.empty(n, np.int32) if either else None
    if n:
        other = a if b is None else b
        capi.check(_lib.bsq_sketch_compare_list_host(a.ctypes.data if Ba else None, Ba, other.ctypes.data if other.shape[0] else None, other.shape[0], S,
                                                     dt, row.ctypes.data, col.ctypes.data, n, match.ctypes.data, eith.ctypes.data if either else None))
    return match, eith


def sketch_compare_list(a, row, col, b=None, *, either=True):
    """`match` and `either` of LISTED pairs of rows: (match, either or None), int32, one entry per pair (row[p], col[p]) of a (Ba, S)
    and b (Bb, S) -- b=None: of a with itself -- with `sketch_compare`'s meaning of both counts.  It rescores a candidate list, from
    `lsh_candidates`, from elsewhere or from a narrower sketch, at the cost of the list and not of Ba x Bb.  An index outside its
    matrix gives match = either = -1 and is never followed.  Device tensors (contiguous sketches, contiguous int64 indices) give device
    tensors on torch's current stream, one launch, nothing read back; numpy arrays go through the CPU twin."""
    if isinstance(a, np.ndarray):
        return sketch_compare_list_host(a, row, col, b, either=either)
    import torch
    Ba, Bb, S, dt = _device_sketches(a, b, "sketch_compare_list")
    other = a if b is None else b
    capi.device_index_lists(row, col, a.device)
    n = row.numel()
    match = torch.empty(n, dtype=torch.int32, device=a.device)
    eith = torch.empty(n, dtype=torch.int32, device=a.device) if either else None
    if n:
        with capi.launching(a.device) as stream:
            capi.check(_lib.bsq_sketch_compare_list_device(a.data_ptr() if Ba else None, Ba, other.data_ptr() if other.shape[0] else None,
                                                           other.shape[0], S, dt, row.data_ptr(), col.data_ptr(), n, match.data_ptr(),
                                                           eith.data_ptr() if either else None, stream))
    return match, eith


def _too_many(total, cap):
    return ValueError("%d candidates before the union, max_candidates = %d: lower max_bucket (long runs then yield their centre's pairs "
                      "only) or raise rows_per_band (fewer, more selective bands)" % (total, cap))


def _lsh_host(a, b, lsh, rule, cap, either):
    """bsq_lsh_pairs_host twice -- to count, then to list -- as `sketch_pairs_host` calls its twin"""
    a, b, Ba, Bb, S, dt = _host_sketches(a, b)
    offs = np.zeros(Ba + 1, np.int64)
    total = ctypes.c_int64(0)

    def call(n, *arrays):
        capi.check(_lib.bsq_lsh_pairs_host(a.ctypes.data if Ba else None, Ba, None if b is None else b.ctypes.data, Bb, S, dt, ctypes.byref(lsh),
                                           None if rule is None else ctypes.byref(rule), -1 if cap is None else cap, ctypes.byref(total),
                                           offs.ctypes.data, n, *(None if x is None else x.ctypes.data for x in arrays)))

    if b is None or Bb:  # (a `b` without rows: no pair, and no pointer that says "two matrices")
        call(0, None, None, None, None)
    if cap is not None and total.value > cap:
        raise _too_many(total.value, cap)
    n = int(offs[-1])
    row, col = np.zeros(n, np.int64), np.zeros(n, np.int64)
    match = None if rule is None else np.zeros(n, np.int32)
    eith = np.zeros(n, np.int32) if rule is not None and either else None
    if n:
        call(n, row, col, match, eith)
    return row, col, match, eith, offs


def _lsh_device(a, b, lsh, T, cap):
    """the candidates (row, col) of device matrices, ascending and each once: keys, torch's stable sort of every band, count, scan,
    emit, torch.unique of the codes"""
    import torch
    Ba, Bb, S, dt = _device_sketches(a, b, "lsh_pairs")
    N, dev = Ba + Bb, a.device
    if N >= 2 ** 31:
        raise ValueError("the two matrices together have more than 2 ** 31 - 1 rows")
    none = torch.empty(0, dtype=torch.int64, device=dev)
    if N == 0:
        return none, none
    with capi.launching(dev) as stream:
        keys = torch.empty((T, N), dtype=torch.int64, device=dev)
        if Ba:
            capi.check(_lib.bsq_lsh_keys_device(a.data_ptr(), Ba, S, dt, ctypes.byref(lsh), keys.data_ptr(), N, stream))
        if Bb:
            capi.check(_lib.bsq_lsh_keys_device(b.data_ptr(), Bb, S, dt, ctypes.byref(lsh), keys.data_ptr() + 8 * Ba, N, stream))
        keys, order = torch.sort(keys, dim=1, stable=True)
        counts = torch.empty(T * N, dtype=torch.int64, device=dev)
        capi.check(_lib.bsq_lsh_count_device(keys.data_ptr(), T, N, ctypes.byref(lsh), counts.data_ptr(), stream))
        ends = torch.cumsum(counts, 0)
        total = int(ends[-1].item())
        if cap is not None and total > cap:
            raise _too_many(total, cap)
        if total == 0:
            return none, none
        codes = torch.empty(total, dtype=torch.int64, device=dev)
        capi.check(_lib.bsq_lsh_emit_device(keys.data_ptr(), order.data_ptr(), T, N, ctypes.byref(lsh), (ends - counts).data_ptr(), total,
                                            codes.data_ptr(), stream))
        del keys, order, counts, ends
        codes = torch.unique(codes)  # (sorted: ascending (i, j))
        row = torch.div(codes, N, rounding_mode="floor")
        col = codes - row * N
        if b is not None:
            cross = (row < Ba) & (col >= Ba)
            row, col = row[cross], col[cross] - Ba
    return row.contiguous(), col.contiguous()


def lsh_candidates(a, b=None, *, rows_per_band, max_bucket=32, max_candidates=None, seed=0):
    """The LSH candidates of a sketch matrix, before any threshold: (row, col), int64, ascending (i, j), each pair once -- the pairs of
    rows that share the key of at least one band (`lsh_keys`).  b=None: the pairs i < j of `a`; b given: the rule runs over `a` followed
    by `b` and the pairs (i in a, j in b) are kept.  In a band, a group of up to `max_bucket` rows with one key yields all its pairs, a
    larger group only the pairs of its smallest row with each other member (linclust's centre rule), so a store that is one read
    repeated costs N - 1 candidates per band and not N * (N - 1) / 2.  max_candidates: raise ValueError, before the candidate list
    is allocated, when the candidates before the union over the bands number more.  Arguments and the device / numpy split as in
    `lsh_pairs`."""
    S = _lsh_width(a, b, "lsh_candidates")
    lsh, T = _lsh_rule(S, rows_per_band, max_bucket, seed, max_candidates)
    cap = None if max_candidates is None else int(max_candidates)
    if isinstance(a, np.ndarray):
        return _lsh_host(a, b, lsh, None, cap, False)[:2]
    return _lsh_device(a, b, lsh, T, cap)


def lsh_pairs(a, b=None, *, rows_per_band, min_jaccard=0.5, min_match=1, max_bucket=32, max_candidates=None, either=True, seed=0):
    """Near-duplicate search without the all-pairs comparison: (row, col, match, either or None, pair_offsets) with the shape and meaning
    of `sketch_pairs`' result, over the LSH candidates of the matrices instead of over every pair.  The cost follows the number of rows
    and of candidates, not Ba x Bb (include/bsq.h, "LSH candidates of a sketch matrix").

    The sketch rows are cut into T = S // rows_per_band bands of `rows_per_band` buckets; two rows are candidates when they agree on a
    whole band (`lsh_candidates`), and a candidate is listed when it passes `sketch_pairs`' rule -- match >= min_match and
    match * 65536 >= floor(min_jaccard * 65536 + 0.5) * either over all S buckets.  With no group above `max_bucket` the result is
    exactly `sketch_pairs`' list restricted to the pairs that share a band; identical rows with a filled bucket among the first
    T * rows_per_band are always listed; rows that are EMPTY throughout never are.  `lsh_rows_per_band(S, min_jaccard)` chooses
    rows_per_band for a predicted recall (`lsh_recall`) at the threshold.  b=None lists the pairs i < j of `a`; b given lists pairs
    (i of a, j of b).  pair_offsets (int64, Ba + 1) is the CSR over the rows of a.  seed: another family of band keys.

    Device tensors (contiguous int32 or int64, as `minhash_packed` returns them) give device tensors on torch's current stream: the
    library's kernels for the keys, the candidates of the sorted bands and the counts of the listed pairs, torch for the stable sort of
    every band, the scan, the union (`torch.unique`) and the compaction.  The call reads three sizes back (the candidates before the
    union, the union's and the result's).  max_candidates=M raises ValueError before the candidate list is allocated when the candidates
    before the union exceed M; None means no limit (8 bytes a candidate).  numpy matrices go through the CPU twin
    (`bsq_lsh_pairs_host`) and give the same bytes."""
    S = _lsh_width(a, b, "lsh_pairs")
    lsh, T = _lsh_rule(S, rows_per_band, max_bucket, seed, max_candidates)
    rule, _ = _pairs_rule(S, min_jaccard, min_match, None, None, False)
    cap = None if max_candidates is None else int(max_candidates)
    if isinstance(a, np.ndarray):
        return _lsh_host(a, b, lsh, rule, cap, either)
    import torch
    row, col = _lsh_device(a, b, lsh, T, cap)
    match, eith = sketch_compare_list(a, row, col, b)
    keep = (match >= rule.min_match) & (match.to(torch.int64) * 65536 >= eith.to(torch.int64) * rule.jaccard_q16)
    row, col, match = row[keep], col[keep], match[keep]
    offs = torch.searchsorted(row, torch.arange(a.shape[0] + 1, dtype=torch.int64, device=a.device))
    return row, col, match, eith[keep] if either else None, offs


def length_key(offsets):
    """The key of cd-hit's order, "longest first": -(offsets[1:] - offsets[:-1]) as int64, a tensor for a tensor (on its device) and a
    numpy array otherwise.  Rows of one length fall to the earlier row."""
    if isinstance(offsets, np.ndarray) or not hasattr(offsets, "is_cuda"):
        o = np.asarray(offsets, np.int64).ravel()
        return np.ascontiguousarray(o[:-1] - o[1:])
    import torch
    o = offsets.to(torch.int64).reshape(-1)
    return (o[:-1] - o[1:]).contiguous()


def cluster_table(labels):
    """(representatives, sizes, dense_id) of a label array: the rows with labels == arange, ascending (int64); their member counts
    (int64); and dense_id[i], the rank of labels[i] among the representatives -- consecutive cluster numbers 0 .. C - 1 in order of each
    cluster's first row.  Plain torch on a tensor (on its device), plain numpy on an array."""
    if isinstance(labels, np.ndarray):
        reps = np.nonzero(labels == np.arange(labels.size, dtype=np.int64))[0].astype(np.int64)
        return reps, np.bincount(labels, minlength=labels.size).astype(np.int64)[reps], np.searchsorted(reps, labels).astype(np.int64)
    import torch
    reps = torch.nonzero(labels == torch.arange(labels.numel(), dtype=torch.int64, device=labels.device)).reshape(-1)
    return reps, torch.bincount(labels, minlength=labels.numel())[reps], torch.searchsorted(reps, labels)


_GOLDEN, _MIX_A, _MIX_B = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def cluster_split(labels, fractions, seed=0):
    """The split index (int64, 0 .. len(fractions) - 1) of every row, THE SAME FOR ALL ROWS OF A CLUSTER: a leakage-free train / test
    (/ validation) split over the labels of `sketch_clusters` or `cluster_pairs`.  The split of a row is decided by (seed, label) alone,
    so rows keep their split when unrelated rows are added after them, and another seed gives another split.

    The fractions are over CLUSTERS, not rows: each cluster goes to split s with probability fractions[s], whatever its size, so a store
    with one very large cluster has row shares that differ from the fractions (`cluster_table` gives the sizes).  They must be positive
    and sum to 1 within 1e-6, else ValueError.

    Integers only: h = the first output of splitmix64 from the state (seed + label) mod 2^64, that is mix64((seed + label +
    0x9E3779B97F4A7C15) mod 2^64) with the finalizer of include/bsq.h ("MinHash sketch"); u = h >> 32; the split is the first s with
    u < floor((fractions[0] + ... + fractions[s]) * 2^32), and the last split takes the rest.  The numpy form computes in uint64, the
    torch form (any device) in int64 with wrap-around products and masked shifts; they give identical arrays."""
    fr = [float(f) for f in fractions]
    if not fr or not all(f > 0.0 for f in fr) or not abs(sum(fr) - 1.0) <= 1e-6:  # (a NaN fails the comparisons)
        raise ValueError("fractions must be positive and sum to 1, got %r" % (fractions,))
    bounds, run = [], 0.0
    for f in fr[:-1]:
        run += f
        bounds.append(min(int(run * 4294967296.0), 1 << 32))
    state = (int(seed) + _GOLDEN) & (2 ** 64 - 1)
    if isinstance(labels, np.ndarray):
        z = labels.astype(np.int64).view(np.uint64) + np.uint64(state)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_MIX_A)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_MIX_B)
        u = (z ^ (z >> np.uint64(31))) >> np.uint64(32)
        return np.searchsorted(np.array(bounds, np.uint64), u, side="right").astype(np.int64)
    import torch

    def signed(c):  # the int64 that holds these 64 bits
        return c - (1 << 64) if c >> 63 else c

    def shr(z, k):  # the logical shift: an arithmetic one with the copies of the sign masked off
        return (z >> k) & ((1 << (64 - k)) - 1)

    z = labels.to(torch.int64) + signed(state)
    z = (z ^ shr(z, 30)) * signed(_MIX_A)
    z = (z ^ shr(z, 27)) * signed(_MIX_B)
    u = shr(z ^ shr(z, 31), 32)
    return torch.searchsorted(torch.tensor(bounds, dtype=torch.int64, device=labels.device), u, right=True)


__all__ = ["EMPTY", "minhash_packed", "minhash_host", "minhash_kernel_name", "sketch_compare", "sketch_compare_host", "sketch_jaccard",
           "sketch_pairs", "sketch_pairs_host", "sketch_duplicates", "sketch_pairs_kernel_name", "sketch_clusters", "sketch_clusters_host",
           "cluster_pairs", "cluster_pairs_host", "sketch_clusters_kernel_name", "cluster_table", "cluster_split", "greedy_pairs",
           "greedy_pairs_host", "greedy_kernel_name", "length_key", "lsh_pairs", "lsh_candidates", "lsh_keys", "lsh_keys_host",
           "sketch_compare_list", "sketch_compare_list_host", "lsh_recall", "lsh_rows_per_band", "lsh_kernel_name"]
