"""Byte-pair encoding of packed batches on the device (`bsq_bpe_tokenize_device`): the vocabulary DNABERT-2, GENA-LM, GROVER and
ProtGPT2 are trained on, where `kmers.kmer_tokenize_packed` is the wrong tokeniser.

A `BPEVocab` is a tokenizer of the package (its classes are the base symbols: case and aliases fold as the tokenizer folds them) and
an ordered list of merges.  Ids: 0 .. C - 1 the classes, C + m the product of merge m, V = C + M; UNK = V marks every unmapped byte
(an N under DNA4) and is never fused; BOS, EOS and PAD follow in the tokenizer's own order of its specials.  A row is one word: no
pre-tokenisation, no dropout, no fuse_unk.  include/bsq.h ("BPE ids of a packed batch") has the full rules.

* `BPEVocab.from_merges`, `BPEVocab.from_tokenizers_json`  a vocabulary from pairs of strings / from a Hugging Face tokenizer.json;
* `bpe_tokenize_packed`   (tokens, lengths) of a packed batch resident on the device, (B, padlen) or (padlen, B), one launch;
* `bpe_tokenize_host`     the library's CPU twin (numpy in, numpy out; no device);
* `bpe_vocab_size`, `bpe_special_ids`, `bpe_strings`, `bpe_decode`, `bpe_external_ids`  the sizes an embedding table needs, the
                          vocabulary-file strings, ids -> strings (host), and the map from these ids to a published vocabulary's;
* `bpe_mlm_tokenize_packed`  (inputs, labels, lengths): masked-LM batches over those ids, drawn on the device in the same launch;
* `bpe_mlm_tokenize_host`  its CPU twin;
* `bpe_kernel_name`, `bpe_mlm_kernel_name`  the kernel a call takes;
* `bpe_train_packed`      learns the merges from a packed store resident on the device (`bsq_bpe_train_*_device`: two launches per
                          merge, the corpus read once per merge), or from numpy arrays through the library's CPU twin;
* `bpe_train_kernel_name` the pass kernel such a call takes;
* `bpe_train_host`        the same rule as plain numpy, a sort of the whole sample per merge: the independent statement the trainer is
                          held against, for samples of a few MB (`bpe_train_packed` is the corpus-scale trainer).

Rows longer than `max_chars` (at most 8192) get length -1 and an empty token row: crop first with `views.crop_packed`.
"""
from __future__ import annotations

import ctypes
import json

import numpy as np

from . import capi

_lib = capi.load()

_NUMPY = {capi.I8: np.int8, capi.I16: np.int16, capi.I32: np.int32, capi.U64: np.uint64, capi.F32: np.float32, capi.F64: np.float64}

TOO_LONG = -1      # lengths[i] of a row of more than max_chars characters (BSQ_BPE_TOO_LONG)
MAX_CHARS = 8192   # the longest row a call takes
WAVE_MAX_CHARS = 1024  # up to here a call takes the wave form: a smaller bound is a cheaper call


def _letters(desc):
    """The first byte of each class, as str: what `kmers.kmer_decode` prints."""
    lut = np.frombuffer(bytes(desc.lut), dtype=np.int8)
    return [chr(int(np.flatnonzero(lut == c)[0])) for c in range(desc.nchars)]


class BPEVocab:
    """A tokenizer and its merges, validated by the library (`bsq_bpe_table_build`): `merges` the (M, 2) int32 array of id pairs,
    `table` the host lookup table, `device_table(device)` its lazily uploaded copy (one per device, kept for the object's life)."""

    def __init__(self, tok, merges):
        self.tok = tok
        self.desc = capi.desc_of(tok)
        m = np.asarray(merges, dtype=np.int64).reshape(-1, 2)
        if m.size and (m.min() < -2 ** 31 or m.max() >= 2 ** 31):
            raise ValueError("a merge names an id outside 32 bits")
        self.merges = np.ascontiguousarray(m.astype(np.int32))
        self.merges.setflags(write=False)
        nbytes = int(_lib.bsq_bpe_table_bytes(self.desc.nchars, self.M))
        if nbytes < 0:
            raise ValueError("%d classes and %d merges: %s" % (self.desc.nchars, self.M, _lib.bsq_last_error().decode()))
        self.table = np.empty(nbytes, dtype=np.uint8)
        if _lib.bsq_bpe_table_build(ctypes.byref(self.desc), self.merges.ctypes.data, self.M, self.table.ctypes.data) != capi.OK:
            raise ValueError("illegal merge list: " + _lib.bsq_last_error().decode())
        self.table.setflags(write=False)
        self._device_tables = {}

    @property
    def M(self):
        return int(self.merges.shape[0])

    def device_table(self, device):
        """The table as a uint8 tensor on `device`, uploaded at the first call."""
        import torch
        device = torch.device(device)
        if device.index is None:
            device = torch.device(device.type, torch.cuda.current_device())
        t = self._device_tables.get(device)
        if t is None:
            t = self._device_tables[device] = torch.from_numpy(self.table.copy()).to(device)
        return t

    @classmethod
    def from_merges(cls, tok, pairs):
        """From pairs of strings in merge order, [("A", "A"), ("AA", "C"), ...].  The strings are resolved through the tokenizer's
        table, so "a" is "A" and an alias is its class; a string must be one class or the product of an earlier merge.  An unmapped
        character, an unknown string and two entries that fold to one pair are a ValueError."""
        desc = capi.desc_of(tok)
        ids = {(c,): c for c in range(desc.nchars)}
        seen, merges = {}, []
        for m, pair in enumerate(pairs):
            if len(pair) != 2:
                raise ValueError("merge %d is not a pair: %r" % (m, pair))
            sides = []
            for s in pair:
                classes = tuple(int(desc.lut[b]) for b in str(s).encode("latin-1"))
                if not classes or min(classes) < 0:
                    raise ValueError("merge %d: %r is empty or holds a character the tokenizer does not map" % (m, s))
                if classes not in ids:
                    raise ValueError("merge %d: %r is neither a class nor the product of an earlier merge" % (m, s))
                sides.append(classes)
            key = (ids[sides[0]], ids[sides[1]])
            if key in seen:
                raise ValueError("merges %d and %d fold to one pair: %r" % (seen[key], m, pair))
            seen[key] = m
            merges.append(key)
            ids.setdefault(sides[0] + sides[1], desc.nchars + m)
        return cls(tok, np.array(merges, dtype=np.int64).reshape(-1, 2))

    @classmethod
    def from_tokenizers_json(cls, tok, path_or_dict):
        """From `model.merges` of a Hugging Face tokenizer.json (a path or the parsed dict): entries "A B" or ["A", "B"].  Read with the
        standard `json` module; the `tokenizers` package is not needed."""
        if isinstance(path_or_dict, dict):
            doc = path_or_dict
        else:
            with open(path_or_dict, "r", encoding="utf-8") as fh:
                doc = json.load(fh)
        model = doc.get("model", doc)
        if "merges" not in model:
            raise ValueError("no model.merges in the tokenizer description")
        pairs = []
        for m, e in enumerate(model["merges"]):
            parts = e.split(" ") if isinstance(e, str) else list(e)
            if len(parts) != 2:
                raise ValueError("merge %d is not a pair: %r" % (m, e))
            pairs.append((parts[0], parts[1]))
        return cls.from_merges(tok, pairs)


def bpe_vocab_size(vocab):
    """Ids of the vocabulary: the classes, the merges, UNK, and BOS / EOS / PAD where the tokenizer has them."""
    return int(_lib.bsq_bpe_vocab_size(ctypes.byref(vocab.desc), vocab.M))


def bpe_special_ids(vocab):
    """{"unk", "bos", "eos", "pad"}: bos / eos are -1 where the tokenizer has none; pad is the id whether or not the tokenizer pads with
    it (an unpadded tokenizer stores 0 at pad positions, as `tokenize_packed` does)."""
    d, M = ctypes.byref(vocab.desc), vocab.M
    return {"unk": int(_lib.bsq_bpe_unk_id(d, M)), "bos": int(_lib.bsq_bpe_bos_id(d, M)), "eos": int(_lib.bsq_bpe_eos_id(d, M)),
            "pad": int(_lib.bsq_bpe_pad_id(d, M))}


def bpe_strings(vocab):
    """The string of every id, 0 .. bpe_vocab_size - 1: the first byte of each class, the concatenation of a merge's sides, and
    `<UNK>`, `<BOS>`, `<EOS>`, `<PAD>` -- the lines of a vocabulary file.  (Two merges may spell one string; both ids keep it.)"""
    out = _letters(vocab.desc)
    for l, r in vocab.merges:
        out.append(out[int(l)] + out[int(r)])
    sp = bpe_special_ids(vocab)
    names = {sp["unk"]: "<UNK>"}
    if sp["bos"] >= 0:
        names[sp["bos"]] = "<BOS>"
    if sp["eos"] >= 0:
        names[sp["eos"]] = "<EOS>"
    if vocab.desc.padchar:
        names[sp["pad"]] = "<PAD>"
    return out + [names[i] for i in range(len(out), bpe_vocab_size(vocab))]


def bpe_decode(vocab, ids):
    """The strings of BPE ids, as a list of str nested like `ids` (host code over a numpy / CPU array or a list); the pad id of an
    unpadded tokenizer's vocabulary (never stored) is a ValueError like any other stranger."""
    strings = bpe_strings(vocab)
    arr = np.asarray(ids.cpu() if hasattr(ids, "cpu") else ids)

    def word(v):
        v = int(v)
        if not 0 <= v < len(strings):
            raise ValueError("%d is not an id of this vocabulary" % v)
        return strings[v]

    def walk(a):
        return [walk(x) for x in a] if a.ndim > 1 else [word(v) for v in a]

    return word(arr) if arr.ndim == 0 else walk(arr)


def bpe_external_ids(vocab, foreign, *, unk=None, bos=None, eos=None, pad=None):
    """An int64 array over these ids holding the ids of a published vocabulary `foreign` ({string: id}), -1 where it has no such
    string: `map[tokens]` renumbers a token matrix.  unk / bos / eos / pad: the foreign strings of the specials ("[UNK]", "<|endoftext|>")."""
    own = {"<UNK>": unk, "<BOS>": bos, "<EOS>": eos, "<PAD>": pad}
    out = np.full(bpe_vocab_size(vocab), -1, dtype=np.int64)
    for i, s in enumerate(bpe_strings(vocab)):
        s = own.get(s, s) if i >= vocab.desc.nchars + vocab.M else s
        if s is not None and s in foreign:
            out[i] = int(foreign[s])
    return out


def _bpe(vocab, destchar, max_chars, form):
    """(bsq_bpe, dtype code, torch dtype) with the library's argument rules applied as ValueError."""
    max_chars = MAX_CHARS if max_chars is None else int(max_chars)
    form = 0 if form is None else int(form)
    if not 1 <= max_chars <= MAX_CHARS:
        raise ValueError("max_chars must lie in 1 .. %d, got %r" % (MAX_CHARS, max_chars))
    if form not in (0, 1, 2) or (form == 1 and max_chars > WAVE_MAX_CHARS):
        raise ValueError("form must be None, 1 (a wave per row: max_chars <= %d) or 2 (a workgroup per row), got %r at max_chars %d"
                         % (WAVE_MAX_CHARS, form, max_chars))
    dt, tdt = capi.dtype_of(destchar)
    size = bpe_vocab_size(vocab)
    if not _lib.bsq_dtype_holds(dt, 0, size - 1):
        raise ValueError("destchar %r cannot hold every id of a vocabulary of %d (the rule is in include/bsq.h, bsq_dtype_holds)" % (destchar, size))
    return capi.Bpe(max_chars, form, 0), dt, tdt


def bpe_kernel_name(vocab=None, *, max_chars=None, form=None):
    """The kernel `bpe_tokenize_packed` takes for this bound (host only: profiling labels, tests); `vocab` plays no part."""
    max_chars = MAX_CHARS if max_chars is None else int(max_chars)
    name = _lib.bsq_bpe_kernel_name(ctypes.byref(capi.Bpe(max_chars, 0 if form is None else int(form), 0))).decode()
    if not name:
        raise ValueError("max_chars must lie in 1 .. %d and form be None, 1 (max_chars <= %d) or 2" % (MAX_CHARS, WAVE_MAX_CHARS))
    return name


def bpe_tokenize_host(vocab, chars, offsets, padlen, destchar="q", batch_first=True, *, max_chars=None, form=None):
    """The library's CPU twin (`bsq_bpe_tokenize_host`, the lookup and selection code of the kernels) on numpy arrays:
    (tokens, lengths) as numpy arrays.  max_chars: None = 8192; form is checked and changes nothing on the host."""
    bpe, dt, _ = _bpe(vocab, destchar, max_chars, form)
    padlen = int(padlen)
    if padlen <= 0:
        raise ValueError("padlen must be positive")
    chars, offsets = capi.host_batch(chars, offsets)
    B = offsets.size - 1
    tokens = np.empty((B, padlen) if batch_first else (padlen, B), dtype=_NUMPY[dt])
    lengths = np.empty(B, dtype=np.int32)
    if B > 0:
        capi.check(_lib.bsq_bpe_tokenize_host(ctypes.byref(vocab.desc), chars.ctypes.data, offsets.ctypes.data, B, padlen, int(bool(batch_first)),
                                              vocab.table.ctypes.data, vocab.M, ctypes.byref(bpe), dt, tokens.ctypes.data, lengths.ctypes.data))
    return tokens, lengths


def bpe_tokenize_packed(vocab, chars, offsets, padlen, destchar="q", batch_first=True, *, max_chars=None, form=None):
    """BPE ids of a packed batch on the device (chars uint8[total], offsets int64[B + 1]): (tokens, lengths) device tensors on torch's
    current stream, one launch.  tokens is (B, padlen) when batch_first else (padlen, B), row = [BOS] id_0 .. id_{n-1} [EOS] PAD ...,
    cut at padlen; lengths (int32) holds every row's n BEFORE the cut, so `lengths + bos + eos > padlen` finds the cut rows, and -1
    (`TOO_LONG`) for a row of more than max_chars characters, whose token row is that of an empty row.

    max_chars: None reads the longest row back (8 bytes, one synchronisation) and takes 1024 where that holds every row, else 8192;
    a number (1 .. 8192) reads nothing back.  At most 1024 takes the wave form, which is the cheaper call.  form: None = the library
    chooses, 1 = a wave per row, 2 = a workgroup per row."""
    import torch
    B = capi.packed_on_device(chars, offsets, "bpe_tokenize_packed works on packed batches resident on the device (chars, offsets tensors)")
    if max_chars is None:
        longest = int((offsets[1:] - offsets[:-1]).max().item()) if B > 0 else 0
        max_chars = WAVE_MAX_CHARS if longest <= WAVE_MAX_CHARS and form != 2 else MAX_CHARS
    bpe, dt, tdt = _bpe(vocab, destchar, max_chars, form)
    padlen = int(padlen)
    if padlen <= 0:
        raise ValueError("padlen must be positive")
    tokens = torch.empty((B, padlen) if batch_first else (padlen, B), dtype=tdt, device=chars.device)
    lengths = torch.empty(B, dtype=torch.int32, device=chars.device)
    if B > 0:
        src = capi.readable_chars(chars, offsets.device)  # (every sequence may be empty)
        table = vocab.device_table(src.device)
        with capi.launching(src.device) as stream:
            capi.check(_lib.bsq_bpe_tokenize_device(ctypes.byref(vocab.desc), src.data_ptr(), offsets.data_ptr(), B, padlen, int(bool(batch_first)),
                                                    table.data_ptr(), vocab.M, ctypes.byref(bpe), dt, tokens.data_ptr(), lengths.data_ptr(), stream))
    return tokens, lengths


def _bpe_mlm(vocab, destchar, label_destchar, frac, mask_prob, random_prob, mask_token, ignore_index, seed, first_row, max_chars, form):
    """(bsq_bpe, bsq_bpe_mlm, input dtype, label dtype, torch dtypes) with the library's argument rules applied as ValueError."""
    bpe, dt, tdt = _bpe(vocab, destchar, max_chars, form)
    for name, p in (("frac", frac), ("mask_prob", mask_prob), ("random_prob", random_prob)):
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError("%s must lie in [0, 1], got %r" % (name, p))
    if float(mask_prob) + float(random_prob) > 1.0 + 1e-12:
        raise ValueError("mask_prob + random_prob must not exceed 1")
    size = bpe_vocab_size(vocab)
    m = capi.BpeMlm(float(frac), float(mask_prob), float(random_prob), size if mask_token is None else int(mask_token), int(ignore_index),
                    int(seed) & (2 ** 64 - 1), int(first_row))
    if m.first_row < 0 or m.mask_token < 0:
        raise ValueError("first_row and mask_token must be >= 0")
    ldt, ltdt = capi.dtype_of(label_destchar)
    top = max(size - 1, m.mask_token)
    if not _lib.bsq_dtype_holds(dt, 0, top):
        raise ValueError("destchar %r cannot hold ids up to %d (vocabulary and mask token)" % (destchar, top))
    last = vocab.desc.nchars + vocab.M - 1
    if not _lib.bsq_dtype_holds(ldt, min(m.ignore_index, 0), max(m.ignore_index, last)):
        raise ValueError("label_destchar %r cannot hold plain ids up to %d and ignore_index %d" % (label_destchar, last, m.ignore_index))
    return bpe, m, dt, ldt, tdt, ltdt


def bpe_mlm_kernel_name(vocab=None, *, max_chars=None, form=None):
    """The kernel `bpe_mlm_tokenize_packed` takes for this bound (host only: profiling labels, tests); `vocab` plays no part."""
    max_chars = MAX_CHARS if max_chars is None else int(max_chars)
    name = _lib.bsq_bpe_mlm_kernel_name(ctypes.byref(capi.Bpe(max_chars, 0 if form is None else int(form), 0))).decode()
    if not name:
        raise ValueError("max_chars must lie in 1 .. %d and form be None, 1 (max_chars <= %d) or 2" % (MAX_CHARS, WAVE_MAX_CHARS))
    return name


def bpe_mlm_tokenize_host(vocab, chars, offsets, padlen, destchar="q", batch_first=True, *, label_destchar="q", frac=0.15, mask_prob=0.8,
                          random_prob=0.1, mask_token=None, ignore_index=-100, seed=0, first_row=0, max_chars=None, form=None):
    """The library's CPU twin (`bsq_bpe_mlm_tokenize_host`: the twin's merge loop and the element code of the kernels) on numpy arrays:
    (inputs, labels, lengths) as numpy arrays.  max_chars: None = 8192; form is checked and changes nothing on the host."""
    bpe, m, dt, ldt, _, _ = _bpe_mlm(vocab, destchar, label_destchar, frac, mask_prob, random_prob, mask_token, ignore_index, seed, first_row,
                                     max_chars, form)
    padlen = int(padlen)
    if padlen <= 0:
        raise ValueError("padlen must be positive")
    chars, offsets = capi.host_batch(chars, offsets)
    B = offsets.size - 1
    shape = (B, padlen) if batch_first else (padlen, B)
    inputs, labels = np.empty(shape, dtype=_NUMPY[dt]), np.empty(shape, dtype=_NUMPY[ldt])
    lengths = np.empty(B, dtype=np.int32)
    if B > 0:
        capi.check(_lib.bsq_bpe_mlm_tokenize_host(ctypes.byref(vocab.desc), chars.ctypes.data, offsets.ctypes.data, B, padlen, int(bool(batch_first)),
                                                  vocab.table.ctypes.data, vocab.M, ctypes.byref(bpe), ctypes.byref(m), dt, inputs.ctypes.data, ldt,
                                                  labels.ctypes.data, lengths.ctypes.data))
    return inputs, labels, lengths


def bpe_mlm_tokenize_packed(vocab, chars, offsets, padlen, destchar="q", batch_first=True, *, label_destchar="q", frac=0.15, mask_prob=0.8,
                            random_prob=0.1, mask_token=None, ignore_index=-100, seed=0, first_row=0, max_chars=None, form=None):
    """Masked-LM batches over the BPE ids of a packed batch on the device: (inputs, labels, lengths) device tensors on torch's current
    stream, one launch (`bsq_bpe_mlm_tokenize_device`; include/bsq.h, "BPE masked-LM", has the draw).  inputs and labels are (B, padlen)
    when batch_first else (padlen, B), with `bpe_tokenize_packed`'s positions; lengths is `bpe_tokenize_packed`'s.

    A share `frac` of a row's tokens is selected (UNK, BOS, EOS and PAD never are); a selected token becomes `mask_token` (None:
    `bpe_vocab_size`) with probability mask_prob, a uniform id of the classes and merge products with random_prob, else keeps its id;
    labels hold the plain id at selected tokens and ignore_index elsewhere.  A token's fate depends on (seed, first_row + its row, its
    index in the row) and its own id only: not on padlen, the layout, the element types, max_chars, form, the batch's size or the
    stream, so a shard drawn with its `first_row` is the same rows of the whole batch.  max_chars / form: exactly as `bpe_tokenize_packed`."""
    import torch
    B = capi.packed_on_device(chars, offsets, "bpe_mlm_tokenize_packed works on packed batches resident on the device (chars, offsets tensors)")
    if max_chars is None:
        longest = int((offsets[1:] - offsets[:-1]).max().item()) if B > 0 else 0
        max_chars = WAVE_MAX_CHARS if longest <= WAVE_MAX_CHARS and form != 2 else MAX_CHARS
    bpe, m, dt, ldt, tdt, ltdt = _bpe_mlm(vocab, destchar, label_destchar, frac, mask_prob, random_prob, mask_token, ignore_index, seed, first_row,
                                          max_chars, form)
    padlen = int(padlen)
    if padlen <= 0:
        raise ValueError("padlen must be positive")
    shape = (B, padlen) if batch_first else (padlen, B)
    inputs = torch.empty(shape, dtype=tdt, device=chars.device)
    labels = torch.empty(shape, dtype=ltdt, device=chars.device)
    lengths = torch.empty(B, dtype=torch.int32, device=chars.device)
    if B > 0:
        src = capi.readable_chars(chars, offsets.device)  # (every sequence may be empty)
        table = vocab.device_table(src.device)
        with capi.launching(src.device) as stream:
            capi.check(_lib.bsq_bpe_mlm_tokenize_device(ctypes.byref(vocab.desc), src.data_ptr(), offsets.data_ptr(), B, padlen, int(bool(batch_first)),
                                                        table.data_ptr(), vocab.M, ctypes.byref(bpe), ctypes.byref(m), dt, inputs.data_ptr(), ldt,
                                                        labels.data_ptr(), lengths.data_ptr(), stream))
    return inputs, labels, lengths


def _train_cfg(max_chars, form, n_merges, table_slots):
    """bsq_bpe_train with the library's argument rules applied as ValueError."""
    form = 0 if form is None else int(form)
    table_slots = 0 if table_slots is None else int(table_slots)
    max_chars, n_merges = int(max_chars), int(n_merges)
    if not 1 <= max_chars <= MAX_CHARS:
        raise ValueError("max_chars must lie in 1 .. %d, got %r" % (MAX_CHARS, max_chars))
    if form not in (0, 1, 2) or (form == 1 and max_chars > WAVE_MAX_CHARS):
        raise ValueError("form must be None, 1 (a wave per row: max_chars <= %d) or 2 (a workgroup per row), got %r at max_chars %d"
                         % (WAVE_MAX_CHARS, form, max_chars))
    if not 0 <= n_merges < 2 ** 31:
        raise ValueError("n_merges must lie in 0 .. 2 ** 31 - 1, got %r" % n_merges)
    if table_slots != 0 and (table_slots < 16 or table_slots > 2 ** 28 or table_slots & (table_slots - 1)):
        raise ValueError("table_slots must be None or a power of two in 16 .. 2 ** 28, got %r" % table_slots)
    return capi.BpeTrain(max_chars, form, n_merges, 0, table_slots)


def _train_bound(longest, max_chars, form):
    """The bound of a call whose longest row was read: the wave form's where it holds every row, else 8192; a longer row is refused."""
    if max_chars is not None:
        return max_chars
    if longest > MAX_CHARS:
        raise ValueError("a row of %d characters: bpe_train_packed takes rows of at most %d; crop first with views.crop_packed or "
                         "FlatFile.windows_device, or pass max_chars to leave longer rows out" % (longest, MAX_CHARS))
    return WAVE_MAX_CHARS if longest <= WAVE_MAX_CHARS and form != 2 else MAX_CHARS


def bpe_train_kernel_name(max_chars=None, form=None):
    """The pass kernel `bpe_train_packed` takes for this bound (host only: profiling labels, tests); None is 8192."""
    max_chars = MAX_CHARS if max_chars is None else int(max_chars)
    name = _lib.bsq_bpe_train_kernel_name(ctypes.byref(capi.BpeTrain(max_chars, 0 if form is None else int(form), 0, 0, 0))).decode()
    if not name:
        raise ValueError("max_chars must lie in 1 .. %d and form be None, 1 (max_chars <= %d) or 2" % (MAX_CHARS, WAVE_MAX_CHARS))
    return name


def _decode_records(best):
    """(merges (M, 2) int64, counts (M,) int64) of a run's records (uint64): those in front of the first count below 2."""
    best = np.asarray(best, dtype=np.uint64)
    counts = (best >> np.uint64(32)).astype(np.int64)
    stop = np.flatnonzero(counts < 2)
    M = int(stop[0]) if stop.size else int(best.size)
    key = (np.uint64(0xFFFFFFFF) - (best[:M] & np.uint64(0xFFFFFFFF))).astype(np.int64)
    return np.stack([key >> 16, key & 0xFFFF], axis=1).reshape(-1, 2), counts[:M]


def bpe_train_packed(tok, chars, offsets, n_merges, *, max_chars=None, form=None, table_slots=None, steps_per_call=256, return_info=False):
    """Learns a `BPEVocab` of at most `n_merges` merges from a packed store (chars uint8[total], offsets int64[B + 1]) by the rule of
    `bpe_train_host` (include/bsq.h, "BPE training"): a row is a word, an unmapped byte a barrier; every step takes the most frequent
    adjacent pair, counted without overlap, ties to the smallest (l, r), and stops when the best count is below 2.

    Device tensors train on the device, on torch's current stream: `steps_per_call` steps (two launches each) are enqueued, then the
    last record is read back (8 bytes) to see whether the stop was reached, until n_merges merges are made; the merges do not depend on
    steps_per_call.  numpy arrays go through the library's CPU twin (`bsq_bpe_train_host`).  chars and offsets are never modified.

    max_chars: None reads the longest row back (8 bytes, one synchronisation); a row above 8192 is a ValueError.  A number (1 .. 8192)
    reads nothing back: longer rows take no part and are counted in `skipped_rows`.  At most 1024 takes the wave form; form: None = the
    library chooses, 1 = a wave per row, 2 = a workgroup per row; the merges never depend on it.  table_slots: None sizes the pair table
    for the last step (a power of two, at most 2 ** 28 slots of 8 bytes); a number overrides it, and a table that overflowed is a
    RuntimeError after the read-back, never a wrong vocabulary.  More than 2 ** 31 - 1 characters is a ValueError.

    return_info=True: (vocab, info) with info = {"counts": int64 winning count of each merge, "skipped_rows", "steps_launched",
    "table_slots", "kernel"}."""
    desc = capi.desc_of(tok)
    steps_per_call = int(steps_per_call)
    if steps_per_call < 1:
        raise ValueError("steps_per_call must be at least 1")
    if isinstance(chars, np.ndarray) and isinstance(offsets, np.ndarray):
        hchars, hoffs = capi.host_batch(chars, offsets)
        B = hoffs.size - 1
        total = int(chars.size)
        if total > 2 ** 31 - 1:
            raise ValueError("bpe_train_packed takes at most 2 ** 31 - 1 characters, got %d" % total)
        longest = int((hoffs[1:] - hoffs[:-1]).max()) if B > 0 and max_chars is None else 0
        cfg = _train_cfg(_train_bound(longest, max_chars, form), form, n_merges, table_slots)
        room = min(cfg.n_merges, 65536 - 4 - desc.nchars)
        merges, counts = np.zeros((room, 2), np.int32), np.zeros(room, np.int64)
        made, skipped = ctypes.c_int64(0), ctypes.c_int64(0)
        if B > 0:
            capi.check(_lib.bsq_bpe_train_host(ctypes.byref(desc), hchars.ctypes.data, hoffs.ctypes.data, B, total, ctypes.byref(cfg),
                                               merges.ctypes.data, counts.ctypes.data, ctypes.byref(made), ctypes.byref(skipped)))
        vocab = BPEVocab(tok, merges[:made.value].astype(np.int64))
        info = {"counts": counts[:made.value].copy(), "skipped_rows": int(skipped.value), "steps_launched": 0,
                "table_slots": int(_lib.bsq_bpe_train_table_slots(ctypes.byref(desc), B, total, ctypes.byref(cfg))),
                "kernel": "bsq_bpe_train_host"}
        return (vocab, info) if return_info else vocab
    import torch
    B = capi.packed_on_device(chars, offsets, "bpe_train_packed works on a packed store resident on the device (chars, offsets tensors), or on numpy arrays")
    total = int(chars.numel())
    if total > 2 ** 31 - 1:
        raise ValueError("bpe_train_packed takes at most 2 ** 31 - 1 characters, got %d" % total)
    longest = int((offsets[1:] - offsets[:-1]).max().item()) if B > 0 and max_chars is None else 0
    cfg = _train_cfg(_train_bound(longest, max_chars, form), form, n_merges, table_slots)
    room = min(cfg.n_merges, 65536 - 4 - desc.nchars)
    slots = int(_lib.bsq_bpe_train_table_slots(ctypes.byref(desc), B, total, ctypes.byref(cfg)))
    info = {"counts": np.zeros(0, np.int64), "skipped_rows": 0, "steps_launched": 0, "table_slots": slots,
            "kernel": _lib.bsq_bpe_train_kernel_name(ctypes.byref(cfg)).decode()}
    merges = np.zeros((0, 2), np.int64)
    if B > 0:
        nbytes = int(_lib.bsq_bpe_train_workspace_bytes(ctypes.byref(desc), B, total, ctypes.byref(cfg)))
        if nbytes < 0:
            raise ValueError("bpe_train_packed: " + _lib.bsq_last_error().decode())
        src = capi.readable_chars(chars, offsets.device)  # (every row may be empty)
        work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=src.device)
        done = 0
        with capi.launching(src.device) as stream:
            capi.check(_lib.bsq_bpe_train_begin_device(ctypes.byref(desc), src.data_ptr(), offsets.data_ptr(), B, total, ctypes.byref(cfg),
                                                       work.data_ptr(), stream))
            while done < room:
                step = min(steps_per_call, room - done)
                capi.check(_lib.bsq_bpe_train_steps_device(ctypes.byref(desc), offsets.data_ptr(), B, total, ctypes.byref(cfg), work.data_ptr(),
                                                           done, step, stream))
                done += step
                if done < room and (int(work[2 + done - 1].item()) >> 32) & 0xFFFFFFFF < 2:  # (the last record: 8 bytes)
                    break
        head = work[:2 + room].cpu().numpy()
        info["steps_launched"], info["skipped_rows"] = done, int(head[0])
        if head[1] != 0:
            raise RuntimeError("bpe_train_packed: the pair table of %d slots overflowed and pairs were dropped; pass a larger table_slots "
                               "(None sizes it for the last step)" % slots)
        merges, info["counts"] = _decode_records(head[2:2 + done].view(np.uint64))
    vocab = BPEVocab(tok, merges)
    return (vocab, info) if return_info else vocab


def _taken(a, key, best):
    """The positions of `a` where the pair `best` is replaced, left to right without overlap: in a run of consecutive occurrences (they
    exist only when l == r) those at even distance from the run's start."""
    hit = key == best
    idx = np.flatnonzero(hit)
    if idx.size == 0:
        return idx
    start = np.ones(idx.size, dtype=bool)
    start[1:] = idx[1:] != idx[:-1] + 1
    run_start = np.maximum.accumulate(np.where(start, idx, 0))
    return idx[(idx - run_start) % 2 == 0]


def bpe_train_host(tok, chars, offsets, n_merges):
    """A plain deterministic BPE trainer on a host sample (numpy chars, offsets): a `BPEVocab` of at most `n_merges` merges.

    Every step takes the most frequent adjacent pair -- occurrences counted without overlap (AAA holds (A, A) once), ties broken by the
    smallest (l, r) -- and stops when the best count is below 2.  Rows are words; an unmapped byte ends one.  It works on the whole
    sample with numpy, a sort per merge: it is meant for samples of a few MB, so that tests, the lab and users without published merges
    have tables.  It is NOT a corpus-scale trainer."""
    desc = capi.desc_of(tok)
    chars, offsets = capi.host_batch(chars, offsets)
    lut = np.frombuffer(bytes(desc.lut), dtype=np.int8).astype(np.int64)
    B = offsets.size - 1
    total = int(offsets[B]) if B > 0 else 0
    a = lut[chars[:total]]
    a = np.insert(a, np.clip(offsets[1:B], 0, total), -1) if B > 1 else a  # (a barrier between rows)
    C = desc.nchars
    n_merges = min(int(n_merges), 65536 - 4 - C)
    merges = []
    while len(merges) < n_merges and a.size >= 2:
        l, r = a[:-1], a[1:]
        key = np.where((l >= 0) & (r >= 0), l * 65536 + r, -1)
        # without overlap: of a run of equal symbols only every second pair counts
        same = np.flatnonzero((l == r) & (l >= 0))
        drop = np.zeros(key.size, dtype=bool)
        if same.size:
            start = np.ones(same.size, dtype=bool)
            start[1:] = same[1:] != same[:-1] + 1
            run_start = np.maximum.accumulate(np.where(start, same, 0))
            drop[same[(same - run_start) % 2 == 1]] = True
        counted = key[(key >= 0) & ~drop]
        if counted.size == 0:
            break
        keys, counts = np.unique(counted, return_counts=True)
        k = int(np.argmax(counts))  # (the first maximum: the smallest key, which is the smallest (l, r))
        if counts[k] < 2:
            break
        best = int(keys[k])
        merges.append((best >> 16, best & 0xFFFF))
        take = _taken(a, key, best)
        a[take] = C + len(merges) - 1
        keep = np.ones(a.size, dtype=bool)
        keep[take + 1] = False
        a = a[keep]
    return BPEVocab(tok, np.array(merges, dtype=np.int64).reshape(-1, 2))


__all__ = ["BPEVocab", "bpe_tokenize_packed", "bpe_tokenize_host", "bpe_vocab_size", "bpe_special_ids", "bpe_strings", "bpe_decode",
           "bpe_external_ids", "bpe_kernel_name", "bpe_train_host", "bpe_train_packed", "bpe_train_kernel_name", "bpe_mlm_tokenize_packed", "bpe_mlm_tokenize_host", "bpe_mlm_kernel_name", "TOO_LONG", "MAX_CHARS", "WAVE_MAX_CHARS"]
