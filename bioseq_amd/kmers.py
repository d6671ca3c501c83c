"""k-mer ids of packed batches on the device (`bsq_kmer_tokenize_device`): the vocabulary DNA language models are trained on.

Every other encode path of the package stops at one token per character.  Here a token is a window of `k` characters -- overlapping
(stride 1: DNABERT's 3- to 6-mers), non-overlapping (stride k: 6-mers as the Nucleotide Transformer reads them) or any other stride,
over any alphabet of the package whose `nchars ** k` stays within 2 ** 24 -- written in ONE launch from the packed batch, instead of
tokens + `unfold` + weighted sum + `where` in torch.

With A = the alphabet's classes and V = A ** k: plain ids are 0 .. V - 1 in lexicographic order (first character most significant),
UNK = V marks a window with any unmapped character (an N under DNA4), then BOS, EOS and PAD follow in the tokenizer's own order of
its specials.  A tail shorter than k is dropped.  include/bsq.h (`bsq_kmer`) has the full rules.

* `kmer_tokenize_packed`  the ids of a packed batch resident on the device, (B, padlen) or (padlen, B);
* `kmer_vocab_size`, `kmer_special_ids`, `kmer_padlen`, `kmer_count`  the sizes an embedding table and a batch need;
* `kmer_decode`           ids -> words (host code: what one needs to write a vocabulary file);
* `kmer_tokenize_host`    the library's CPU twin of the ids (numpy in, numpy out; no device);
* `kmer_mlm_tokenize_packed`  span-masked masked-LM pairs (inputs, labels) over the k-mer ids, drawn in the encode launch (DNABERT's
                          objective: contiguous runs of `span` windows are selected, then BERT's 80/10/10 replacement);
* `kmer_mlm_tokenize_host`, `span_anchor_prob`, `kmer_mlm_kernel_name`  its CPU twin, the share -> anchor rate helper, the kernel taken;
* `kmer_spectrum_packed`  the k-mer SPECTRUM of a packed batch: one (B, nchars ** k) matrix of per-sequence counts or frequencies
                          (tetranucleotide frequencies, di- / tripeptide composition, 6-mer profiles), one strand or both, in one launch
                          -- a histogram per row in LDS, no id matrix, no scatter_add_ (`bsq_kmer_spectrum_device`);
* `kmer_spectrum_host`, `kmer_spectrum_width`, `kmer_spectrum_kernel_name`, `kmer_canonical_columns`  its CPU twin, its width, the
                          kernel taken, and the columns v <= rc(v) that turn a both-strand spectrum into the canonical-k-mer profile.

The crops and reverse-complement views of `views` hand this module packed batches as they are:
`kmer_tokenize_packed(tok, *views.crop_packed(chars, offsets, 1000, revcomp_frac=0.5), k=6, padlen=...)`.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi

_lib = capi.load()

_NUMPY = {capi.I8: np.int8, capi.I16: np.int16, capi.I32: np.int32, capi.U64: np.uint64, capi.F32: np.float32, capi.F64: np.float64}


def _kmer(tok, k, stride=1):
    """(bsq_desc, bsq_kmer) with the library's argument rules applied (ValueError; no device is touched for a bad argument)."""
    desc = capi.desc_of(tok)
    km = capi.Kmer(int(k), int(stride))
    if km.stride < 1:
        raise ValueError("stride must be >= 1, got %r" % (stride,))
    if _lib.bsq_kmer_vocab_size(ctypes.byref(desc), ctypes.byref(km)) < 0:
        raise ValueError("k = %r with %d classes: %s" % (k, desc.nchars, _lib.bsq_last_error().decode()))
    return desc, km


def _dtype(desc, km, destchar):
    """capi.dtype_of, refusing an element type that cannot hold every id of the vocabulary (the library's BSQ_ERR_DTYPE, by its own
    rule `bsq_dtype_holds`) as a ValueError."""
    dt, tdt = capi.dtype_of(destchar)
    vocab = _lib.bsq_kmer_vocab_size(ctypes.byref(desc), ctypes.byref(km))
    if not _lib.bsq_dtype_holds(dt, 0, vocab - 1):
        raise ValueError("destchar %r cannot hold every id of a vocabulary of %d (the rule is in include/bsq.h, bsq_dtype_holds)" % (destchar, vocab))
    return dt, tdt


def kmer_vocab_size(tok, k):
    """Ids of the k-mer vocabulary of `tok`: nchars ** k plain words, UNK, and BOS / EOS / PAD where the tokenizer has them."""
    desc, km = _kmer(tok, k)
    return int(_lib.bsq_kmer_vocab_size(ctypes.byref(desc), ctypes.byref(km)))


def kmer_special_ids(tok, k):
    """{"unk", "bos", "eos", "pad"}: bos / eos are -1 where the tokenizer has none; pad is the id whether or not the tokenizer pads
    with it (an unpadded tokenizer stores 0 at pad positions, as `tokenize_packed` does)."""
    desc, km = _kmer(tok, k)
    d, m = ctypes.byref(desc), ctypes.byref(km)
    return {"unk": int(_lib.bsq_kmer_unk_id(d, m)), "bos": int(_lib.bsq_kmer_bos_id(d, m)), "eos": int(_lib.bsq_kmer_eos_id(d, m)),
            "pad": int(_lib.bsq_kmer_pad_id(d, m))}


def kmer_count(k, length, stride=1):
    """Whole windows of k characters at multiples of `stride` in a sequence of `length` characters (0 below k)."""
    km = capi.Kmer(int(k), int(stride))
    n = int(_lib.bsq_kmer_count(ctypes.byref(km), int(length)))
    if n < 0:
        raise ValueError("k and stride must be >= 1")
    return n


def kmer_padlen(tok, k, max_seq_len, stride=1):
    """The padlen that holds every sequence of up to `max_seq_len` characters: its windows + BOS + EOS."""
    _kmer(tok, k, stride)
    return kmer_count(k, max_seq_len, stride) + int(tok.includes_bos()) + int(tok.includes_eos())


def kmer_max_length(tok, k, padlen, stride=1):
    """The longest sequence whose windows all fit into `padlen` positions (a longer one is clamped by the kernels)."""
    room = int(padlen) - int(tok.includes_bos()) - int(tok.includes_eos())
    return max(room, 0) * int(stride) + int(k) - 1


def kmer_decode(tok, k, ids):
    """The words of k-mer ids, as a list of str (nested like `ids`): the first byte of each class for a plain id, `<UNK>`, `<BOS>`,
    `<EOS>`, `<PAD>` for the specials.  Host code over a numpy / CPU array or a list."""
    desc, km = _kmer(tok, k)
    sp = kmer_special_ids(tok, k)
    lut = np.frombuffer(bytes(desc.lut), dtype=np.int8)
    letters = [chr(int(np.flatnonzero(lut == c)[0])) for c in range(desc.nchars)]
    names = {sp["unk"]: "<UNK>", sp["pad"]: "<PAD>"}
    if sp["bos"] >= 0:
        names[sp["bos"]] = "<BOS>"
    if sp["eos"] >= 0:
        names[sp["eos"]] = "<EOS>"
    arr = np.asarray(ids.cpu() if hasattr(ids, "cpu") else ids)
    V = desc.nchars ** km.k

    def word(v):
        v = int(v)
        if v in names:
            return names[v]
        if not 0 <= v < V:
            raise ValueError("%d is not an id of this vocabulary" % v)
        out = []
        for _ in range(km.k):
            v, r = divmod(v, desc.nchars)
            out.append(letters[r])
        return "".join(reversed(out))

    def walk(a):
        return [walk(x) for x in a] if a.ndim > 1 else [word(v) for v in a]

    return word(arr) if arr.ndim == 0 else walk(arr)


def kmer_kernel_name(tok, k, B, padlen, destchar="q", batch_first=True, *, stride=1):
    """The kernel `kmer_tokenize_packed` takes for this shape (host only: profiling labels, tests)."""
    desc, km = _kmer(tok, k, stride)
    dt, _ = _dtype(desc, km, destchar)
    return _lib.bsq_kmer_kernel_name(ctypes.byref(desc), ctypes.byref(km), int(B), int(padlen), int(bool(batch_first)), dt).decode()


def kmer_tokenize_host(tok, chars, offsets, k, padlen, destchar="q", batch_first=True, *, stride=1):
    """The library's CPU twin (`bsq_kmer_tokenize_host`, the same id code as the kernels) on numpy arrays: a numpy matrix."""
    desc, km = _kmer(tok, k, stride)
    dt, _ = _dtype(desc, km, destchar)
    if int(padlen) <= 0:
        raise ValueError("padlen must be positive")
    chars, offsets = capi.host_batch(chars, offsets)
    B = offsets.size - 1
    out = np.empty((B, int(padlen)) if batch_first else (int(padlen), B), dtype=_NUMPY[dt])
    capi.check(_lib.bsq_kmer_tokenize_host(ctypes.byref(desc), chars.ctypes.data, offsets.ctypes.data, B, int(padlen), int(bool(batch_first)),
                                           ctypes.byref(km), dt, out.ctypes.data))
    return out


def _validate(tok, chars, offsets, B, desc, km, padlen):
    """The over-long-sequence check of `tokenize_packed` with the k-mer bound (the library's error), and malformed offsets."""
    bound = kmer_max_length(tok, km.k, padlen, km.stride)
    bad = ctypes.c_int64(-1)
    with capi.launching(chars.device) as stream:
        st = _lib.bsq_validate_packed_device(offsets.data_ptr(), B, bound, 0, 0, chars.numel(), ctypes.byref(bad), stream)
    if st == capi.ERR_SEQ_TOO_LONG:
        i = int(bad.value)
        raise RuntimeError("seq len %d holds more than padlen %d k-mers (k %d, stride %d, bos + eos %d): at most %d characters fit"
                           % (int(offsets[i + 1] - offsets[i]), padlen, km.k, km.stride, desc.bos + desc.eos, bound))
    capi.check(st)


def kmer_tokenize_packed(tok, chars, offsets, k, padlen, destchar="q", batch_first=True, *, stride=1, validate=True):
    """k-mer ids of a packed batch on the device (chars uint8[total], offsets int64[B + 1]): a device tensor (B, padlen) when
    batch_first else (padlen, B), on torch's current stream, one launch.

    Row = [BOS] id_0 .. id_{n-1} [EOS] PAD ..., window j = characters [j * stride, j * stride + k).  validate: the over-long-sequence
    check of `tokenize_packed` with the k-mer bound -- a sequence longer than `kmer_max_length(tok, k, padlen, stride)` raises the
    library's over-long error instead of being clamped; malformed offsets raise too."""
    import torch
    desc, km = _kmer(tok, k, stride)
    dt, tdt = _dtype(desc, km, destchar)
    padlen = int(padlen)
    if padlen <= 0:
        raise ValueError("padlen must be positive")
    B = capi.packed_on_device(chars, offsets, "kmer_tokenize_packed works on packed batches resident on the device (chars, offsets tensors)")
    if validate and B > 0:
        _validate(tok, chars, offsets, B, desc, km, padlen)
    out = torch.empty((B, padlen) if batch_first else (padlen, B), dtype=tdt, device=chars.device)
    if B > 0:
        src = capi.readable_chars(chars, offsets.device)  # (every sequence may be empty)
        with capi.launching(src.device) as stream:
            capi.check(_lib.bsq_kmer_tokenize_device(ctypes.byref(desc), src.data_ptr(), offsets.data_ptr(), B, padlen, int(bool(batch_first)),
                                                     ctypes.byref(km), dt, out.data_ptr(), stream))
    return out


def span_anchor_prob(frac, span):
    """The anchor rate at which a share `frac` of the windows of a long row is covered by spans of `span` windows:
    1 - (1 - frac) ** (1 / span) (`bsq_kmer_mlm_anchor_prob`)."""
    p = float(_lib.bsq_kmer_mlm_anchor_prob(float(frac), int(span)))
    if p < 0:
        raise ValueError("frac must lie in [0, 1] and span in 1 .. 16, got %r and %r" % (frac, span))
    return p


def _kmer_mlm(tok, k, stride, destchar, label_destchar, frac, span, anchor_prob, mask_prob, random_prob, mask_token, ignore_index, seed, first_row):
    """(desc, km, bsq_kmer_mlm, input dtype, label dtype, torch dtypes) with the library's argument rules applied as ValueError."""
    desc, km = _kmer(tok, k, stride)
    span = -(-km.k // km.stride) if span is None else int(span)
    if not 1 <= span <= 16:
        raise ValueError("span must lie in 1 .. 16, got %r" % (span,))
    if anchor_prob is None:
        anchor_prob = span_anchor_prob(frac, span)
    elif frac != 0.15:
        raise ValueError("give frac or anchor_prob, not both")
    vocab = int(_lib.bsq_kmer_vocab_size(ctypes.byref(desc), ctypes.byref(km)))
    m = capi.KmerMlm(float(anchor_prob), float(mask_prob), float(random_prob), span, vocab if mask_token is None else int(mask_token),
                     int(ignore_index), int(seed) & (2 ** 64 - 1), int(first_row))
    for name, p in (("anchor_prob", m.anchor_prob), ("mask_prob", m.mask_prob), ("random_prob", m.random_prob)):
        if not 0.0 <= p <= 1.0:
            raise ValueError("%s must lie in [0, 1], got %r" % (name, p))
    if m.mask_prob + m.random_prob > 1.0 + 1e-12:
        raise ValueError("mask_prob + random_prob > 1")
    if m.first_row < 0 or m.mask_token < 0:
        raise ValueError("first_row and mask_token must be >= 0")
    dt, tdt = capi.dtype_of(destchar)
    ldt, ltdt = capi.dtype_of(label_destchar)
    top = max(vocab - 1, m.mask_token)
    if not _lib.bsq_dtype_holds(dt, 0, top):
        raise ValueError("destchar %r cannot hold ids up to %d (vocabulary and mask token)" % (destchar, top))
    last = desc.nchars ** km.k - 1
    if not _lib.bsq_dtype_holds(ldt, min(m.ignore_index, 0), max(m.ignore_index, last)):
        raise ValueError("label_destchar %r cannot hold plain ids up to %d and ignore_index %d" % (label_destchar, last, m.ignore_index))
    return desc, km, m, dt, ldt, tdt, ltdt


def kmer_mlm_kernel_name(tok, k, B, padlen, destchar="q", batch_first=True, *, stride=1, label_destchar="q", mask_token=None, ignore_index=-100):
    """The kernel `kmer_mlm_tokenize_packed` takes for this shape (host only: profiling labels, tests).  mask_token and ignore_index
    matter only to the element-type rule: a call the encode would refuse is a ValueError here too."""
    desc, km, m, dt, ldt, _, _ = _kmer_mlm(tok, k, stride, destchar, label_destchar, 0.15, None, None, 0.8, 0.1, mask_token, ignore_index, 0, 0)
    return _lib.bsq_kmer_mlm_kernel_name(ctypes.byref(desc), ctypes.byref(km), ctypes.byref(m), int(B), int(padlen), int(bool(batch_first)),
                                         dt, ldt).decode()


def kmer_mlm_tokenize_host(tok, chars, offsets, k, padlen, destchar="q", batch_first=True, *, stride=1, frac=0.15, span=None, anchor_prob=None,
                           mask_prob=0.8, random_prob=0.1, mask_token=None, ignore_index=-100, label_destchar="q", seed=0, first_row=0):
    """The library's CPU twin (`bsq_kmer_mlm_tokenize_host`, the element code of the kernels) on numpy arrays: (inputs, labels)."""
    desc, km, m, dt, ldt, _, _ = _kmer_mlm(tok, k, stride, destchar, label_destchar, frac, span, anchor_prob, mask_prob, random_prob, mask_token,
                                           ignore_index, seed, first_row)
    if int(padlen) <= 0:
        raise ValueError("padlen must be positive")
    chars, offsets = capi.host_batch(chars, offsets)
    B = offsets.size - 1
    shape = (B, int(padlen)) if batch_first else (int(padlen), B)
    inputs, labels = np.empty(shape, dtype=_NUMPY[dt]), np.empty(shape, dtype=_NUMPY[ldt])
    if B > 0:
        capi.check(_lib.bsq_kmer_mlm_tokenize_host(ctypes.byref(desc), chars.ctypes.data, offsets.ctypes.data, B, int(padlen), int(bool(batch_first)),
                                                   ctypes.byref(km), ctypes.byref(m), dt, inputs.ctypes.data, ldt, labels.ctypes.data))
    return inputs, labels


def kmer_mlm_tokenize_packed(tok, chars, offsets, k, padlen, destchar="q", batch_first=True, *, stride=1, frac=0.15, span=None, anchor_prob=None,
                             mask_prob=0.8, random_prob=0.1, mask_token=None, ignore_index=-100, label_destchar="q", seed=0, first_row=0,
                             validate=True):
    """Span-masked masked-LM pairs over the k-mer ids of a packed batch on the device: (inputs, labels) device tensors, (B, padlen) when
    batch_first else (padlen, B), on torch's current stream, one launch (`bsq_kmer_mlm_tokenize_device`; include/bsq.h has the draw).

    Anchors open runs of `span` consecutive windows (None: ceil(k / stride), the windows that share a character -- k at stride 1, 1 at
    stride k); a selected window becomes `mask_token` (None: `kmer_vocab_size`) with probability mask_prob, a uniform plain id with
    random_prob, else keeps its id; labels hold the plain id at selected windows and ignore_index elsewhere.  UNK windows and BOS / EOS /
    PAD are never selected.  `frac` is the share of windows covered in a long row (`anchor_prob` = `span_anchor_prob(frac, span)`);
    give `anchor_prob` instead to set the anchor rate itself -- both is a ValueError.  A window's fate depends on (seed, first_row + its
    row, its index) only.  validate: as `kmer_tokenize_packed`."""
    import torch
    desc, km, m, dt, ldt, tdt, ltdt = _kmer_mlm(tok, k, stride, destchar, label_destchar, frac, span, anchor_prob, mask_prob, random_prob,
                                                mask_token, ignore_index, seed, first_row)
    padlen = int(padlen)
    if padlen <= 0:
        raise ValueError("padlen must be positive")
    B = capi.packed_on_device(chars, offsets, "kmer_mlm_tokenize_packed works on packed batches resident on the device (chars, offsets tensors)")
    if validate and B > 0:
        _validate(tok, chars, offsets, B, desc, km, padlen)
    shape = (B, padlen) if batch_first else (padlen, B)
    inputs = torch.empty(shape, dtype=tdt, device=chars.device)
    labels = torch.empty(shape, dtype=ltdt, device=chars.device)
    if B > 0:
        src = capi.readable_chars(chars, offsets.device)  # (every sequence may be empty)
        with capi.launching(src.device) as stream:
            capi.check(_lib.bsq_kmer_mlm_tokenize_device(ctypes.byref(desc), src.data_ptr(), offsets.data_ptr(), B, padlen, int(bool(batch_first)),
                                                         ctypes.byref(km), ctypes.byref(m), dt, inputs.data_ptr(), ldt, labels.data_ptr(), stream))
    return inputs, labels


_SPECTRUM_MAX_WINDOWS = 1 << 23  # (include/bsq.h, "k-mer spectrum": a row counts its first 2 ** 23 windows)


def _spectrum(tok, k, stride, destchar, both_strands, normalize, form, total_chars=0):
    """(desc, km, bsq_kmer_spectrum, dtype code, torch dtype, V) with the library's argument rules applied as ValueError."""
    desc, km = _kmer(tok, k, stride)
    V = int(_lib.bsq_kmer_spectrum_width(ctypes.byref(desc), ctypes.byref(km)))
    if V < 0:
        raise ValueError("k = %r with %d classes: %s" % (k, desc.nchars, _lib.bsq_last_error().decode()))
    if normalize:
        dt, tdt = capi.destchar_arg(destchar, (capi.F32, capi.F64), "a spectrum of frequencies takes 'f' or 'd'")
    else:
        dt, tdt = capi.destchar_arg(destchar, (capi.I32, capi.U64, capi.F32, capi.F64), "a spectrum of counts takes 'i', 'q', 'f' or 'd'")
    if both_strands and not capi.has_strands(desc):
        raise ValueError("both_strands needs an alphabet with strands: the four classes A, C, G, T = 0, 1, 2, 3 (DNA, DNA4), not %r" % (tok.key,))
    form = 0 if form is None else int(form)
    if form not in (0, 1, 2) or (form == 1 and V > 1024):
        raise ValueError("form must be None, 1 (a wave per row: nchars ** k <= 1024) or 2 (a workgroup per row), got %r at width %d" % (form, V))
    return desc, km, capi.KmerSpectrum(int(bool(both_strands)), int(bool(normalize)), form, 0, int(total_chars)), dt, tdt, V


def kmer_spectrum_width(tok, k):
    """Columns of the spectrum: nchars ** k (ValueError beyond 2 ** 14: DNA4 up to k = 7, DNA5 6, AMINO20 3, SEB8 4)."""
    desc, km = _kmer(tok, k)
    V = int(_lib.bsq_kmer_spectrum_width(ctypes.byref(desc), ctypes.byref(km)))
    if V < 0:
        raise ValueError("k = %r with %d classes: %s" % (k, desc.nchars, _lib.bsq_last_error().decode()))
    return V


def kmer_canonical_columns(tok, k):
    """The sorted int64 columns v with v <= rc(v) (host numpy): `spectrum[:, cols]` of a `both_strands` spectrum is the canonical-k-mer
    profile -- (4 ** k + 4 ** (k / 2)) / 2 columns for even k, 4 ** k / 2 for odd k.  ValueError for an alphabet without strands."""
    desc, km = _kmer(tok, k)
    if not capi.has_strands(desc):
        raise ValueError("canonical k-mers need an alphabet with strands: the four classes A, C, G, T = 0, 1, 2, 3 (DNA, DNA4), not %r" % (tok.key,))
    V = kmer_spectrum_width(tok, k)
    v = np.arange(V, dtype=np.int64)
    rc, rest = np.zeros(V, dtype=np.int64), v.copy()
    for _ in range(km.k):
        rc = rc * 4 + (3 - rest % 4)
        rest //= 4
    return v[v <= rc]


def kmer_spectrum_kernel_name(tok, k, B, destchar="f", *, stride=1, both_strands=False, normalize=False, form=None, total_chars=0):
    """The kernel `kmer_spectrum_packed` takes (host only: profiling labels, tests); total_chars: `chars.numel()` of the call, 0 = unknown."""
    desc, km, o, dt, _, _ = _spectrum(tok, k, stride, destchar, both_strands, normalize, form, total_chars)
    return _lib.bsq_kmer_spectrum_kernel_name(ctypes.byref(desc), ctypes.byref(km), ctypes.byref(o), int(B), dt).decode()


def kmer_spectrum_host(tok, chars, offsets, k, destchar="f", *, stride=1, both_strands=False, normalize=False):
    """The library's CPU twin (`bsq_kmer_spectrum_host`, the window and element code of the kernels) on numpy arrays: a (B, V) matrix."""
    desc, km, o, dt, _, V = _spectrum(tok, k, stride, destchar, both_strands, normalize, None)
    chars, offsets = capi.host_batch(chars, offsets)
    B = offsets.size - 1
    out = np.empty((B, V), dtype=_NUMPY[dt])
    if B > 0:
        capi.check(_lib.bsq_kmer_spectrum_host(ctypes.byref(desc), chars.ctypes.data, offsets.ctypes.data, B, ctypes.byref(km), ctypes.byref(o), dt,
                                               out.ctypes.data))
    return out


def kmer_spectrum_packed(tok, chars, offsets, k, destchar="f", *, stride=1, both_strands=False, normalize=False, form=None, validate=True):
    """The k-mer spectrum of a packed batch on the device (chars uint8[total], offsets int64[B + 1]): a (B, nchars ** k) device tensor
    on torch's current stream, one launch, nothing read back.

    out[i, v] = the windows of row i (those of `kmer_tokenize_packed` at the same k and stride; BOS / EOS / PAD play no part) whose id is
    v; a window with an unmapped character counts nowhere.  both_strands (DNA, DNA4): every window also counts at the id of its reverse
    complement, so columns v and rc(v) are equal and `[:, kmer_canonical_columns(tok, k)]` is the canonical profile.  normalize: each row
    divided by its sum (destchar 'f' or 'd'; an empty row stays zero); counts take 'i', 'q', 'f' or 'd'.  form: None = the library
    chooses from `chars.numel()` / B, 1 = a wave per row, 2 = a workgroup per row.  validate: malformed offsets and a row of more than
    2 ** 23 windows raise the library's errors instead of being clamped."""
    B = capi.packed_on_device(chars, offsets, "kmer_spectrum_packed works on packed batches resident on the device (chars, offsets tensors)")
    desc, km, o, dt, tdt, V = _spectrum(tok, k, stride, destchar, both_strands, normalize, form, chars.numel())
    max_len = (_SPECTRUM_MAX_WINDOWS - 1) * km.stride + km.k if validate else None
    return capi._row_table_packed(chars, offsets, B, V, tdt, max_len, lambda src, out, stream: _lib.bsq_kmer_spectrum_device(
        ctypes.byref(desc), src, offsets.data_ptr(), B, ctypes.byref(km), ctypes.byref(o), dt, out, stream))


__all__ = ["kmer_tokenize_packed", "kmer_tokenize_host", "kmer_vocab_size", "kmer_special_ids", "kmer_count", "kmer_padlen",
           "kmer_max_length", "kmer_decode", "kmer_kernel_name", "kmer_mlm_tokenize_packed", "kmer_mlm_tokenize_host", "span_anchor_prob",
           "kmer_mlm_kernel_name", "kmer_spectrum_packed", "kmer_spectrum_host", "kmer_spectrum_width", "kmer_spectrum_kernel_name",
           "kmer_canonical_columns"]
