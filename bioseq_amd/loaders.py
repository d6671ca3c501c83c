"""Dataset layer over FlatFile + Tokenizer -- the surface of /root/reference/bioseq/loaders.py, with the
batch as the unit of work.

The reference's `FlatFileDataset.__getitem__` tokenises ONE sequence per call on the host
(`batch_tokenize([seq], ...)`, loaders.py:84,103) and the DataLoader stacks the results.  Here a batch is
encoded by ONE launch from the FlatFile's packed bytes (`get_batch`, and `__getitems__` for
torch >= 2 DataLoader batched fetching), optionally after BLOSUM62 augmentation on the device, and the
conv-net layout 'length batch emb -> batch emb length' + .float() (loaders.py:74) is written directly
by the kernel (`layout="bcl"`, float32) instead of being produced by a permute + cast.
"""
from __future__ import annotations

import numpy as np
import torch

from . import blosum, capi, kmers, masking, packing, views
from . import bpe as bpe_ids
from . import translate as translation
from .flatfile import FlatFile


def FF2NP(x, tokenizer, destfile, *, batch_size=8192):
    """Token matrix of a whole FlatFile as a uint8 memmap at `destfile`: (nseqs, maxseqlen + bos + eos), batch-first
    (the reference's helper of the same name, loaders.py:11-26) -- `batch_size` sequences per device encode."""
    if not isinstance(x, FlatFile):
        raise TypeError("FF2NP expects a FlatFile")
    n = x.nseqs()
    width = x.maxseqlen + int(tokenizer.includes_bos()) + int(tokenizer.includes_eos())
    tokens = np.memmap(destfile, dtype=np.uint8, mode="w+", shape=(n, width))
    first = 0
    while first < n:
        last = min(n, first + batch_size)
        rows = x.batch_tokenize(tokenizer, first, last, padlen=width, destchar="B", batch_first=True)
        tokens[first:last] = rows.view(np.uint8)
        first = last
    return tokens, destfile


class FlatFileDataset(torch.utils.data.Dataset):
    """FlatFile + Tokenizer dataset (loaders.py:29-115).

    cnn=False: items are token rows (max_seq_len,) int64; cnn=True: one-hot (C, max_seq_len) float32.
    `augment` BLOSUM62 point mutations are applied to a sequence with probability `augment_frac`
    (>= 1: always) before encoding.  `get_batch(start, stop)` / `__getitems__(indices)` return the
    stacked batch -- (B, P) int64 or (B, C, P) float32 on `device` -- from a single encode.

    masked=True (keyword; off by default): batches are masked-LM pairs drawn on the device at rate `maskfrac` --
    (inputs, labels) of BERT's 80/10/10 replacement (masking.mlm_tokenize_packed; labels int64 with ignore_index -100,
    mask token = tokenizer.alphabet_size()) for token rows, (masked one-hot (B, C, P) float32, labels) for cnn=True
    (masking.onehot_masked_packed).  The masks come from `seed` and the call: every get_batch / __getitems__ call and
    every `batches()` epoch draws with the next key of the dataset's own counter (a rebuilt dataset repeats them), and
    inside an epoch a row is keyed by its index in the epoch's order -- `group` and `prefetch` hand out the same masks.
    With `augment` the mutations come first, on the batch's own copy.

    crop=N (keyword; off by default): every row is a window of at most N characters of its sequence (views.crop_packed, drawn on
    the device; crop_mode "random", "head" or "center"), so max_seq_len = crop + bos + eos whatever the longest stored sequence is,
    and batches are trusted (no validation read-back).  revcomp_frac=p > 0 (nucleotide keys DNA / DNA4 / DNA5 only) reverse-
    complements a row with probability p; without `crop` whole sequences are flipped and the width stays.  The views come first,
    then the augmentation, then the mask and the encode.  Their draw is keyed like the masks, by a counter of its own (enabling crop
    changes no mask): a fresh key per get_batch / __getitems__ / __getitem__ / fetch call and per `batches()` epoch, a row keyed by
    its index in the epoch's order.

    kmer=k (keyword; off by default; token rows only): a token is a window of k characters, `kmer_stride` characters apart
    (kmers.kmer_tokenize_packed: 1 = overlapping, k = non-overlapping), so max_seq_len = kmers.kmer_padlen of the longest stored
    sequence, or of `crop` when cropping.  It composes with crop, revcomp_frac, shuffle, group and prefetch -- they all hand the encode
    a packed batch.  With cnn=True, augment > 0 or masked=True it raises ValueError: a k-mer one-hot and protein mutations under
    k-mers are not provided, and masking overlapping windows needs span masks, which this draw is not -- the span-masked form has a
    keyword of its own:

    kmer_mlm=True (keyword; off by default; only with kmer=): the k-mer batches are span-masked masked-LM batches drawn on the device
    (kmers.kmer_mlm_tokenize_packed, one launch) -- `get_batch`, `__getitems__` and `batches()` hand out (inputs, labels): anchors open
    runs of `kmer_span` consecutive windows (None: ceil(kmer / kmer_stride), the windows that share a character) so that a share
    `maskfrac` of the windows is selected, then BERT's 80/10/10 replacement with mask token = kmers.kmer_vocab_size; labels int64 with
    ignore_index -100.  Keyed like masked=True: a fresh key per call and per `batches()` epoch, a row keyed by its index in the epoch's
    order -- crop, revcomp_frac, shuffle, `group` and `prefetch` compose and hand out the same masks.  With cnn=True, augment > 0,
    masked=True or pack= it raises ValueError, and so it does without kmer=.  `token_dtype` must hold every id and the mask token
    (the rule of include/bsq.h): 'f' at nchars ** kmer = 2 ** 24 (DNA4 kmer=12) cannot, and the first batch raises ValueError.

    spectrum=k (keyword; off by default): a batch is the (B, nchars ** k) float32 k-mer spectrum of its sequences
    (kmers.kmer_spectrum_packed, one launch): frequencies (`spectrum_normalize`, the default) or counts of the windows `spectrum_stride`
    characters apart, of one strand or, with `spectrum_both_strands` (DNA, DNA4), of both.  `get_batch`, `__getitems__` and `batches()`
    hand the matrix out; it composes with crop, revcomp_frac, shuffle and prefetch.  With cnn=True, augment > 0, masked=True, kmer=,
    pack= or group > 1 it raises ValueError.

    translate=0 | 1 | 2 (keyword; off by default): the store holds NUCLEOTIDES, the tokenizer is a protein one, and every batch is
    translated on the device in that forward frame (translate.translate_packed, NCBI table `codon_table` or 64 bytes of the caller's
    own) after the gather or the crop / strand views and before everything else: masked, pack, pack_mlm, cnn, augment, kmer,
    spectrum, group and prefetch see a protein batch and work unchanged.  max_seq_len = (crop or the longest sequence) // 3 + bos + eos.
    A codon with a byte that is no base becomes X and a stop stays '*': unmapped characters to the protein tokenizers, encoded as
    they encode any unmapped character.  revcomp_frac > 0 is allowed with it whatever the tokenizer: the strand draw in front of the
    frame makes the batch a sample of the six frames.  Translation draws nothing: no key or counter is added, no existing draw shifts.

    bpe=vocab (keyword; off by default; token rows only; a `bpe.BPEVocab` over this dataset's tokenizer): a token is a BPE id
    (bpe.bpe_tokenize_packed, one launch; `token_dtype`, batch-first) from `get_batch`, `__getitems__`, `__getitem__` and `batches()`.
    max_seq_len = `bpe_padlen` when given (a smaller number cuts rows, as padlen does everywhere), else longest + bos + eos with
    `longest` the crop, the store's maxseqlen, or a third of it under translate=: no merge can lengthen a row.  `longest` is also the
    call's max_chars, so no batch reads anything back; above 8192 it is a ValueError: give crop=.  A store whose lengths are not
    trusted (opened with a smaller maxseqlen than its longest sequence) has every batch's lengths checked, and a row that is too long
    raises, as validated batches do.  It composes with crop, revcomp_frac, translate, shuffle, group and prefetch.  With cnn=True,
    augment > 0, masked=True, kmer=, pack= or spectrum= it raises ValueError.

    bpe_mlm=True (keyword; off by default; only with bpe=): the BPE batches are masked-LM batches drawn on the device at rate `maskfrac`
    (bpe.bpe_mlm_tokenize_packed, the same single launch) -- (inputs, labels): BERT's 80/10/10 replacement with mask token =
    bpe.bpe_vocab_size, labels int64 with ignore_index -100.  Keyed like kmer_mlm=True: a fresh key per call and per `batches()` epoch,
    a row keyed by its index in the epoch's order, so `group` and `prefetch` hand out the same masks.

    span_corrupt=True (keyword; off by default; token rows only): the batches are T5's span-corruption batches drawn on the device
    (masking.span_corrupt_packed, one launch) -- `get_batch`, `__getitems__`, `__getitem__` and `batches()` hand out (inputs, labels):
    anchors open spans of `span` characters so that a share `maskfrac` of a long row is covered, every run of covered characters
    becomes one sentinel (tokenizer.alphabet_size() upwards, at most 100 per row) in the (B, max_seq_len) inputs, and the labels,
    (B, `target_len`) int64 with ignore_index -100, hold each sentinel followed by the tokens it stands for.  target_len=None is the
    input width: a target body is at most one element longer than its sequence, so only a longest sequence that is cut out whole, of
    a tokenizer without BOS, loses its last label; a smaller one cuts label rows at it.  Keyed exactly like kmer_mlm=True: a fresh key
    per call and per `batches()` epoch, a row keyed by its index in the epoch's order.  It composes with crop, revcomp_frac, translate,
    shuffle, group and prefetch.  With cnn=True, augment > 0, masked=True, kmer=, bpe=, pack= or spectrum= it raises ValueError.

    pack="nextfit" | "stream" (keyword; off by default; token rows only): batches are sequence-packed -- several sequences per row
    of max_seq_len positions (packing.pack_tokenize_packed) -- and `get_batch`, `__getitems__` and `batches()` hand out
    (tokens, segment_ids, position_ids), each (rows, max_seq_len), rows being what the batch needs (one 8-byte read-back per batch:
    the host waits for the batch's plan before it issues the encode, also under `prefetch`, where that wait falls into the issue of the
    NEXT batch -- the encode still runs under the consumer's kernels, the host-side overlap of the issue is what is lost).
    It composes with crop, revcomp_frac, shuffle and prefetch.  With cnn=True, augment > 0, masked=True, kmer= or group > 1 it raises
    ValueError: a super-batch's row blocks are not the batches' own packings, and the masked form of a packed batch has a keyword
    of its own:

    pack_mlm=True (keyword; off by default; only with pack=): the packed batches are masked-LM batches drawn on the device at rate
    `maskfrac` (packing.pack_mlm_tokenize_packed, one encode launch) -- `get_batch`, `__getitems__` and `batches()` hand out
    (inputs, labels, segment_ids, position_ids).  The mask draw is keyed by a sequence's row in the draw and a character's index in
    its sequence, which the packed encode carries for every position: the masks are those masked=True gives the same sequences,
    keyed the same way (a fresh key per call and per `batches()` epoch, a row keyed by its index in the epoch's order; `prefetch`
    hands out the same masks).  The exclusions of pack= hold.
    """

    NUCLEOTIDE_KEYS = ("DNA", "DNA4", "DNA5")

    def __init__(self, ff, tokenizer, *, augment=0, augment_frac=0.5, cnn=False, device=None, maskfrac=0.15, seed=13, token_dtype="q", prefetch=0, masked=False,
                 crop=None, crop_mode="random", revcomp_frac=0.0, kmer=None, kmer_stride=1, pack=None, pack_mlm=False,
                 kmer_mlm=False, kmer_span=None, spectrum=None, spectrum_stride=1, spectrum_both_strands=False, spectrum_normalize=True,
                 translate=None, codon_table=1, bpe=None, bpe_padlen=None, bpe_mlm=False, span_corrupt=False, span=3, target_len=None):
        super().__init__()
        if not isinstance(ff, FlatFile):
            raise TypeError("FlatFileDataset expects a FlatFile")
        self.device = torch.device("cuda" if device is None else device)
        self.ff, self.tokenizer = ff, tokenizer
        # FlatFile(path, maxseqlen=N) takes the caller's word for N; when a stored sequence is longer than that, max_seq_len is too
        # short for it: the reference aborts on such a sequence (tokenize.h:359-362), so batches are then validated (and raise) instead
        # of being trusted (unvalidated kernels would clamp the sequence silently)
        self._trusted_lengths = ff.maxseqlen >= getattr(ff, "_longest", ff.maxseqlen + 1)
        # attribute names as in the reference's class (loaders.py:36-47)
        self.max_seq_len = self.maxseqlen = ff.maxseqlen + int(tokenizer.includes_bos()) + int(tokenizer.includes_eos())
        self.augment, self.augment_frac = augment, augment_frac
        self.cnn, self.maskfrac = cnn, maskfrac
        self._seed = int(seed)
        self._calls = 0
        # element type of the token rows: 'q' = int64 as the reference's loader hands them to nn.Embedding (loaders.py:84-86);
        # 'b' = int8 -- an eighth of the bytes, and with `augment` set the whole batch step is ONE launch (bsq_augment_tokenize_device)
        self.token_dtype = token_dtype
        # `batches()`: how many batches are encoded ahead of the consumer on the two side streams (0: in order on the current stream)
        self.prefetch = int(prefetch)
        self._side = None
        self.masked = bool(masked)
        self._mask_calls = 0
        if crop is not None and int(crop) <= 0:
            raise ValueError("crop must be a positive number of characters, got %r" % (crop,))
        views._crop(int(crop or 0), crop_mode, revcomp_frac, 0, 0)  # (mode and revcomp_frac checked here)
        if translate is not None and (isinstance(translate, (bool, str)) or int(translate) not in (0, 1, 2)):
            raise ValueError("translate must be a forward frame 0, 1 or 2, got %r" % (translate,))
        self.translate = None if translate is None else int(translate)
        # (the table is checked here; the struct is what every batch's launch takes)
        self._translate_rule = None if translate is None else translation._rule(self.translate, codon_table, "X", "*")[0]
        if float(revcomp_frac) > 0 and translate is None and tokenizer.key not in self.NUCLEOTIDE_KEYS:
            raise ValueError("revcomp_frac > 0 needs a nucleotide alphabet (%s), not %r" % (", ".join(self.NUCLEOTIDE_KEYS), tokenizer.key))
        self.crop = None if crop is None else int(crop)
        self.crop_mode, self.revcomp_frac = crop_mode, float(revcomp_frac)
        self._views = self.crop is not None or self.revcomp_frac > 0
        self._crop_calls = 0
        if self.crop is not None:  # every view fits: nothing to validate
            self.max_seq_len = self.maxseqlen = self.crop + int(tokenizer.includes_bos()) + int(tokenizer.includes_eos())
            self._trusted_lengths = True
        if self.translate is not None:  # a row holds at most a third of its source's characters, whatever the frame
            longest = self.crop if self.crop is not None else ff.maxseqlen
            self.max_seq_len = self.maxseqlen = longest // 3 + int(tokenizer.includes_bos()) + int(tokenizer.includes_eos())
        self.kmer = None if kmer is None else int(kmer)
        self.kmer_stride = int(kmer_stride)
        if self.kmer is not None:
            if cnn or augment or masked:
                raise ValueError("kmer= gives token rows of the plain batch: it cannot be combined with cnn=True, augment > 0 or masked=True")
            # (k, stride and nchars ** k are checked here); at least one position, so that a store of sequences shorter than k still encodes
            longest = self.crop if self.crop is not None else ff.maxseqlen
            if self.translate is not None:
                longest //= 3
            self.max_seq_len = self.maxseqlen = max(1, kmers.kmer_padlen(tokenizer, self.kmer, longest, self.kmer_stride))
        self.pack = pack
        if pack is not None:
            if pack not in ("nextfit", "stream"):
                raise ValueError("pack must be 'nextfit' or 'stream', got %r" % (pack,))
            if cnn or augment or masked or kmer is not None:
                raise ValueError("pack= gives packed token rows of the plain batch: it cannot be combined with cnn=True, augment > 0, "
                                 "masked=True or kmer= (masked-LM batches over packed rows: pack_mlm=True)")
        self.kmer_mlm = bool(kmer_mlm)
        self.kmer_span = None if kmer_span is None else int(kmer_span)
        if self.kmer_mlm:
            if self.kmer is None:
                raise ValueError("kmer_mlm=True masks the k-mer batches of kmer=: give kmer=k with it")
            if cnn or augment or masked or pack is not None:  # (the first three are refused by kmer= above)
                raise ValueError("kmer_mlm=True cannot be combined with cnn=True, augment > 0, masked=True or pack=")
            kmers.span_anchor_prob(maskfrac, -(-self.kmer // self.kmer_stride) if self.kmer_span is None else self.kmer_span)  # (checked here)
        self.pack_mlm = bool(pack_mlm)
        if self.pack_mlm and pack is None:
            raise ValueError("pack_mlm=True masks the packed batches of pack=: give pack='nextfit' or pack='stream' with it")
        self.spectrum = None if spectrum is None else int(spectrum)
        self.spectrum_stride, self.spectrum_both_strands = int(spectrum_stride), bool(spectrum_both_strands)
        self.spectrum_normalize = bool(spectrum_normalize)
        if self.spectrum is not None:
            if cnn or augment or masked or kmer is not None or pack is not None:
                raise ValueError("spectrum= gives one k-mer spectrum per sequence of the plain batch: it cannot be combined with cnn=True, "
                                 "augment > 0, masked=True, kmer= or pack=")
            # (k, stride, nchars ** k and the strands are checked here)
            kmers.kmer_spectrum_kernel_name(tokenizer, self.spectrum, 1, "f", stride=self.spectrum_stride,
                                            both_strands=self.spectrum_both_strands, normalize=self.spectrum_normalize)

        self.bpe, self.bpe_mlm = bpe, bool(bpe_mlm)
        if self.bpe_mlm and bpe is None:
            raise ValueError("bpe_mlm=True masks the BPE batches of bpe=: give bpe=vocab with it")
        if bpe is not None:
            if cnn or augment or masked or kmer is not None or pack is not None or spectrum is not None:
                raise ValueError("bpe= gives BPE token rows of the plain batch: it cannot be combined with cnn=True, augment > 0, masked=True, "
                                 "kmer=, pack= or spectrum= (masked-LM batches over BPE ids: bpe_mlm=True)")
            if not isinstance(bpe, bpe_ids.BPEVocab) or bytes(bpe.desc) != bytes(capi.desc_of(tokenizer)):
                raise ValueError("bpe= must be a BPEVocab over this dataset's tokenizer (the same alphabet and eos / bos / padchar flags)")
            longest = self.crop if self.crop is not None else ff.maxseqlen
            if self.translate is not None:
                longest //= 3
            if longest > bpe_ids.MAX_CHARS:
                raise ValueError("bpe= takes rows of at most %d characters and this store's reach %d: give crop=" % (bpe_ids.MAX_CHARS, longest))
            self._bpe_max_chars = max(1, longest)
            if bpe_padlen is not None and int(bpe_padlen) <= 0:
                raise ValueError("bpe_padlen must be a positive number of positions, got %r" % (bpe_padlen,))
            width = longest + int(tokenizer.includes_bos()) + int(tokenizer.includes_eos())
            self.max_seq_len = self.maxseqlen = int(bpe_padlen) if bpe_padlen is not None else max(1, width)
            # (token_dtype and maskfrac are checked here)
            if self.bpe_mlm:
                bpe_ids._bpe_mlm(bpe, token_dtype, "q", maskfrac, 0.8, 0.1, None, -100, 0, 0, self._bpe_max_chars, None)
            else:
                bpe_ids._bpe(bpe, token_dtype, self._bpe_max_chars, None)

        self.span_corrupt, self.span = bool(span_corrupt), span
        self.target_len = None
        if self.span_corrupt:
            if cnn or augment or masked or kmer is not None or bpe is not None or pack is not None or spectrum is not None:
                raise ValueError("span_corrupt=True gives span-corruption batches of the plain token rows: it cannot be combined with cnn=True, "
                                 "augment > 0, masked=True, kmer=, bpe=, pack= or spectrum=")
            if target_len is not None and int(target_len) <= 0:
                raise ValueError("target_len must be a positive number of positions, got %r" % (target_len,))
            self.target_len = self.max_seq_len if target_len is None else int(target_len)
            masking._span_params(tokenizer, token_dtype, "q", maskfrac, span, None, None, 1, 100, -100, 0, 0)  # (checked here)

    def __len__(self):
        return self.ff.nseqs()

    def _packed_device(self, start, stop, indices=None, trusted=False, view=None):
        """The batch every encode takes: the rows of `_source_device`, translated when translate= is set (one more launch, a fresh
        buffer; it draws nothing)."""
        chars, offs = self._source_device(start, stop, indices, trusted, view)
        if self.translate is None:
            return chars, offs
        n = int(offs.numel()) - 1
        cap = int(chars.numel()) // 3  # (never synchronises: the buffer bounds the batch)
        if self.crop is not None:
            cap = min(cap, n * (self.crop // 3))
        return translation._launch(chars, offs, n, None, None, n, n, self._translate_rule, cap)[:2]

    def _source_device(self, start, stop, indices=None, trusted=False, view=None):
        """The batch's own packed copy on the device (never the resident store when it is going to be mutated).
        trusted: `indices` is this dataset's own permutation (in range, no repeats) -- nothing to check, nothing read back.
        view: (key, first_row) of the crop / strand draw (None: the next key of the dataset's counter, rows from 0)."""
        if self._views:
            return self._views_device(start, stop, indices, trusted, view if view is not None else (self._crop_key(), 0))
        if indices is None:
            chars, offs = self.ff.packed_device(start, stop, self.device)
            if self.augment:
                chars = chars.clone()  # never mutate the resident store
        else:  # arbitrary index set (a shuffling sampler): rebuilt on the device from the resident store, no host gather
            chars, offs = self.ff.gather_device(indices, self.device, validate=not trusted, distinct=trusted)
        return chars, offs

    def _crop_key(self):
        """Seed of the next crop / strand draw: the dataset's seed and its own counter of view calls."""
        self._crop_calls += 1
        return (self._seed * 0xC2B2AE3D27D4EB4F + self._crop_calls) & (2 ** 64 - 1)

    def _views_device(self, start, stop, indices, trusted, view):
        """The batch's views (views.crop_packed) read straight from the resident store -- in place of the gather, one launch for
        up to 4096 rows.  A fresh buffer: augmentation may mutate it."""
        key, first_row = view
        ff = self.ff
        chars, offs = ff.to_device(self.device)
        window = self.crop or 0
        kw = dict(mode=self.crop_mode, revcomp_frac=self.revcomp_frac, seed=key, first_row=first_row)
        if indices is None:
            stop = min(int(stop), ff.nseqs())
            start = min(max(0, int(start)), stop)
            cap = (stop - start) * window if window else int(ff._offsets[stop] - ff._offsets[start])
            return views.crop_packed(chars, offs[start:stop + 1], window, capacity=cap, validate=False, **kw)
        if trusted:  # this dataset's own permutation: in range, no repeats -- the launch alone, nothing checked, nothing read back
            n = int(indices.numel())
            cap = n * window if window else (int(ff._top_lengths_cumsum()[n - 1]) if n else 0)
            c = views._crop(window, self.crop_mode, self.revcomp_frac, key, first_row)
            return views._launch_crop(chars, offs, ff.nseqs(), indices, n, c, cap)[:2]
        if isinstance(indices, torch.Tensor) and indices.is_cuda:
            n = int(indices.numel())
            cap = n * window if window else n * ff._longest
            return views.crop_packed(chars, offs, window, index=indices, capacity=cap, **kw)
        host = np.asarray(indices, dtype=np.int64).ravel()
        cap = host.size * window if window else (int((ff._offsets[host + 1] - ff._offsets[host]).sum()) if host.size else 0)
        return views.crop_packed(chars, offs, window, index=host, capacity=cap, **kw)

    def _mask_key(self):
        """Seed of the next masked call: the dataset's seed and its own counter of masked calls."""
        self._mask_calls += 1
        return (self._seed * 0x9E3779B97F4A7C15 + self._mask_calls) & (2 ** 64 - 1)

    def _encode_masked(self, chars, offs, mask_seed, first_row):
        trusted = self._trusted_lengths
        if self.augment:
            self._calls += 1
            blosum.augment_packed(chars, offs, self.augment, self.augment_frac, self._seed + self._calls)
        if self.cnn:
            return masking.onehot_masked_packed(self.tokenizer, chars, offs, self.max_seq_len, "f", "bcl", frac=self.maskfrac, seed=mask_seed,
                                                first_row=first_row, validate=not trusted)
        return masking.mlm_tokenize_packed(self.tokenizer, chars, offs, self.max_seq_len, self.token_dtype, True, frac=self.maskfrac,
                                           seed=mask_seed, first_row=first_row, validate=not trusted)

    def _encode_pack_mlm(self, chars, offs, mask_seed, first_row):
        return tuple(packing.pack_mlm_tokenize_packed(self.tokenizer, chars, offs, self.max_seq_len, self.token_dtype, mode=self.pack,
                                                      frac=self.maskfrac, seed=mask_seed, first_row=first_row,
                                                      validate=not self._trusted_lengths)[:4])

    def _encode_kmer_mlm(self, chars, offs, mask_seed, first_row):
        return kmers.kmer_mlm_tokenize_packed(self.tokenizer, chars, offs, self.kmer, self.max_seq_len, self.token_dtype, True,
                                              stride=self.kmer_stride, frac=self.maskfrac, span=self.kmer_span, seed=mask_seed,
                                              first_row=first_row, validate=not self._trusted_lengths)

    def _encode_span_corrupt(self, chars, offs, mask_seed, first_row):
        return masking.span_corrupt_packed(self.tokenizer, chars, offs, self.max_seq_len, self.target_len, self.token_dtype, frac=self.maskfrac,
                                           span=self.span, seed=mask_seed, first_row=first_row, validate=not self._trusted_lengths)[:2]

    def _bpe_lengths_checked(self, lengths):
        """A store whose lengths are not trusted may hold a row of more than max_chars characters: its batch raises (one read-back)."""
        if not self._trusted_lengths and bool((lengths < 0).any()):
            raise RuntimeError("a sequence is longer than the %d characters bpe= was set up for (the store's maxseqlen)" % self._bpe_max_chars)

    def _encode_bpe_mlm(self, chars, offs, mask_seed, first_row):
        inputs, labels, lengths = bpe_ids.bpe_mlm_tokenize_packed(self.bpe, chars, offs, self.max_seq_len, self.token_dtype, True,
                                                                  frac=self.maskfrac, seed=mask_seed, first_row=first_row,
                                                                  max_chars=self._bpe_max_chars)
        self._bpe_lengths_checked(lengths)
        return inputs, labels

    def _encode(self, chars, offs):
        """augment_seq, then encode (bioseq/loaders.py:83-84, :102-103) on the batch's own copy.  Token rows go through the
        one-call entry `blosum.augment_tokenize_packed` (one launch for int8 rows; the entry runs the two launches for the
        other types); the one-hot form augments, then encodes."""
        trusted = self._trusted_lengths
        if self.pack is not None:
            return tuple(packing.pack_tokenize_packed(self.tokenizer, chars, offs, self.max_seq_len, self.token_dtype, mode=self.pack,
                                                      validate=not trusted)[:3])
        if self.kmer is not None:
            return kmers.kmer_tokenize_packed(self.tokenizer, chars, offs, self.kmer, self.max_seq_len, self.token_dtype, True,
                                              stride=self.kmer_stride, validate=not trusted)
        if self.bpe is not None:
            tokens, lengths = bpe_ids.bpe_tokenize_packed(self.bpe, chars, offs, self.max_seq_len, self.token_dtype, True, max_chars=self._bpe_max_chars)
            self._bpe_lengths_checked(lengths)
            return tokens
        if self.spectrum is not None:
            return kmers.kmer_spectrum_packed(self.tokenizer, chars, offs, self.spectrum, "f", stride=self.spectrum_stride,
                                              both_strands=self.spectrum_both_strands, normalize=self.spectrum_normalize, validate=not trusted)
        if self.augment:
            self._calls += 1
            seed = self._seed + self._calls
            if not self.cnn and trusted:
                return blosum.augment_tokenize_packed(self.tokenizer, chars, offs, self.max_seq_len, self.token_dtype, True,
                                                      chain_len=self.augment, augment_frac=self.augment_frac, seed=seed)
            blosum.augment_packed(chars, offs, self.augment, self.augment_frac, seed)
        # validate=False only when no stored sequence is longer than ff.maxseqlen (= max_seq_len - bos - eos): every batch cut or
        # gathered from the store then has well-formed offsets and legal lengths, and the device-side check would only add a
        # synchronising read-back (~30 us) per batch.  A store opened with a smaller maxseqlen is validated and raises.
        if self.cnn:
            return self.tokenizer.onehot_packed(chars, offs, self.max_seq_len, "f", layout="bcl", validate=not trusted)
        # int64 rows written by the kernel itself ('q'), not int8 + a .to(torch.long) pass over the matrix
        return self.tokenizer.tokenize_packed(chars, offs, self.max_seq_len, self.token_dtype, True, validate=not trusted)

    def get_batch(self, start, stop):
        """Sequences [start, stop) as one encoded batch on the device."""
        if self.masked:
            return self._encode_masked(*self._packed_device(start, stop), self._mask_key(), 0)
        if self.pack_mlm:
            return self._encode_pack_mlm(*self._packed_device(start, stop), self._mask_key(), 0)
        if self.kmer_mlm:
            return self._encode_kmer_mlm(*self._packed_device(start, stop), self._mask_key(), 0)
        if self.bpe_mlm:
            return self._encode_bpe_mlm(*self._packed_device(start, stop), self._mask_key(), 0)
        if self.span_corrupt:
            return self._encode_span_corrupt(*self._packed_device(start, stop), self._mask_key(), 0)
        return self._encode(*self._packed_device(start, stop))

    def _index(self, i):
        """Python indexing: -len <= i < len, else IndexError (the reference's ff.access raises out_of_range; a silent
        wrap would also make `for x in ds` -- the legacy iteration protocol -- run forever)."""
        n = len(self)
        i = int(i)
        if not -n <= i < n:
            raise IndexError("index %d is out of range for %d sequences" % (i, n))
        return i + n if i < 0 else i

    def __getitems__(self, indices):
        """One encoded batch ON THE DEVICE for the whole index list -- a single stacked tensor, not a list of samples:
        use `DataLoader(ds, batch_size=..., collate_fn=lambda batch: batch, num_workers=0)` (the default collate would
        re-stack it with a copy, and device tensors cannot cross worker processes).  A list of host integers costs one
        upload of 8 bytes per index; an int64 tensor on the device (see `batches`) costs none."""
        if isinstance(indices, torch.Tensor) and indices.is_cuda:
            packed = self._packed_device(0, 0, indices)
        else:
            idx = [self._index(i) for i in indices]
            if idx and idx == list(range(idx[0], idx[0] + len(idx))):
                return self.get_batch(idx[0], idx[-1] + 1)
            packed = self._packed_device(0, 0, idx)
        if self.masked:
            return self._encode_masked(*packed, self._mask_key(), 0)
        if self.pack_mlm:
            return self._encode_pack_mlm(*packed, self._mask_key(), 0)
        if self.kmer_mlm:
            return self._encode_kmer_mlm(*packed, self._mask_key(), 0)
        if self.bpe_mlm:
            return self._encode_bpe_mlm(*packed, self._mask_key(), 0)
        if self.span_corrupt:
            return self._encode_span_corrupt(*packed, self._mask_key(), 0)
        return self._encode(*packed)

    def batches(self, batch_size, shuffle=True, drop_last=False, generator=None, prefetch=None, group=1):
        """One epoch of encoded batches with the sampler ON THE DEVICE: a `torch.randperm` drawn on `self.device` (or the
        identity), cut into index tensors that never leave HBM.  Nothing is copied host -> device per batch: the store is
        resident (FlatFile.to_device), the indices are device tensors, the batch is gathered, augmented and encoded there.
        Yields (B, P) int64 tokens or (B, C, P) float32 one-hots, like `__getitems__` (masked=True: the (inputs, labels) pairs, one
        mask key per epoch, rows keyed by their index in the epoch's order).

        Consecutive batches are independent, and this loop is the one place that knows it (round 6):

        group = G > 1   G consecutive batches are gathered and encoded as ONE super-batch (one gather launch, one encode launch) and
                        handed out as its row blocks -- both layouts are batch-first, so batch k is rows [k * batch_size, (k + 1) *
                        batch_size) of the super-batch, a view.  A batch step of <= 4096 sequences is bound by the host's ~20 us of
                        launches, not by the GPU: G = 4 brings the epoch of 4096-sequence batches from 23 to ~8 us per batch.  The
                        batches are bit for bit those of G = 1, except with `augment`: the mutations are then one draw over the
                        super-batch (seeded like its first batch) instead of G draws -- the same law, other random numbers.
        prefetch = k > 0 (None: the dataset's `prefetch` attribute)  the gather + augmentation + encode of the next k (super-)batches
                        are issued on two SIDE STREAMS that take turns while the consumer still holds the current one; a batch is
                        handed over with an event the consumer's current stream waits for (no host synchronisation) and
                        `record_stream`.  Same tensors bit for bit as prefetch = 0.  The hand-off costs ~14 us of host time per
                        (super-)batch: it pays when the encode is long enough to hide under the consumer's own kernels (large
                        batches, one-hot outputs), and LOSES in a host-bound loop of small batches (profiles/r06/loader_prefetch.txt)
                        -- hence off by default."""
        n = len(self)
        order = (torch.randperm(n, device=self.device, generator=generator) if shuffle
                 else torch.arange(n, device=self.device))
        fused = bool(self.augment) and not self.cnn and not self.masked and str(self.token_dtype)[:1].lower() == "b"  # int8 rows take the one-launch entry, whose in-kernel wait can (in theory) expire
        depth = int(self.prefetch if prefetch is None else prefetch)
        batch_size = int(batch_size)
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        if self.pack is not None and int(group) > 1:
            raise ValueError("group > 1 cannot be combined with pack=: a super-batch's row blocks are not the batches' own packings")
        if self.spectrum is not None and int(group) > 1:
            raise ValueError("group > 1 cannot be combined with spectrum=")
        pairs = self.masked or self.pack is not None or self.kmer_mlm or self.bpe_mlm or self.span_corrupt  # a batch is a tuple of tensors
        span = batch_size * max(1, int(group))
        n_eff = n - n % batch_size if drop_last else n
        firsts = list(range(0, n_eff, span))
        mask_seed = self._mask_key() if self.masked or self.pack_mlm or self.kmer_mlm or self.bpe_mlm or self.span_corrupt else None
        crop_seed = self._crop_key() if self._views else None

        def encode(first):
            stop = min(n_eff, first + span)
            view = (crop_seed, first) if self._views else None
            packed = (self._packed_device(0, 0, order[first:stop], trusted=True, view=view) if shuffle
                      else self._packed_device(first, stop, view=view))
            if self.masked:
                return self._encode_masked(*packed, mask_seed, first)
            if self.pack_mlm:
                return self._encode_pack_mlm(*packed, mask_seed, first)
            if self.kmer_mlm:
                return self._encode_kmer_mlm(*packed, mask_seed, first)
            if self.bpe_mlm:
                return self._encode_bpe_mlm(*packed, mask_seed, first)
            if self.span_corrupt:
                return self._encode_span_corrupt(*packed, mask_seed, first)
            return self._encode(*packed)

        def hand_out(big):
            rows = big[0].shape[0] if pairs else big.shape[0]
            if rows <= batch_size or self.pack is not None:
                yield big
            elif self.masked or self.kmer_mlm or self.bpe_mlm or self.span_corrupt:
                for r in range(0, rows, batch_size):
                    yield big[0][r:r + batch_size], big[1][r:r + batch_size]
            else:
                for r in range(0, rows, batch_size):
                    yield big[r:r + batch_size]

        try:
            if depth <= 0:
                for first in firsts:
                    big = encode(first)
                    if fused:
                        blosum.check_fused()  # host memory only: the launches that have completed so far (a poisoned batch raises here or below)
                    yield from hand_out(big)
                return
            import collections
            with torch.cuda.device(self.device):
                self.ff.to_device(self.device)  # (the store goes up once, before any side stream reads it)
                consumer = torch.cuda.current_stream()
                if self._side is None:
                    self._side = (torch.cuda.Stream(), torch.cuda.Stream())
                for side in self._side:  # whatever produced the store and `order` on the consumer's stream comes first
                    side.wait_stream(consumer)
                order.record_stream(self._side[0]), order.record_stream(self._side[1])
                queue = collections.deque()
                it = iter(enumerate(firsts))
                events = [torch.cuda.Event() for _ in range(depth + 1)]  # reused in turn: at most depth + 1 batches are in flight
                set_stream = torch.cuda.set_stream  # (cheaper than entering a `torch.cuda.stream` context per batch)

                def issue():
                    k, first = next(it, (None, None))
                    if first is None:
                        return
                    side = self._side[k & 1]
                    back = torch.cuda.current_stream()
                    set_stream(side)
                    try:
                        big = encode(first)
                        ready = events[k % (depth + 1)]
                        ready.record(side)
                    finally:
                        set_stream(back)
                    queue.append((big, ready))

                for _ in range(depth):
                    issue()
                while queue:
                    big, ready = queue.popleft()
                    issue()  # the next one goes out BEFORE this one is handed over: it runs under whatever the consumer does with it
                    now = torch.cuda.current_stream()
                    now.wait_event(ready)
                    for t in (big if pairs else (big,)):
                        t.record_stream(now)
                    if fused:
                        blosum.check_fused()
                    yield from hand_out(big)
        finally:
            if fused:  # the epoch's last batches: the one synchronising check, where an epoch synchronises anyway
                blosum.check_fused(synchronize=True)

    def __getitem__(self, index):
        if isinstance(index, slice):
            s, e, st = index.indices(len(self))
            return self.__getitems__(list(range(s, e, st)))
        index = self._index(index)
        if self.masked or self.pack is not None or self.kmer_mlm or self.bpe_mlm or self.span_corrupt:
            return tuple(t[0] for t in self.get_batch(index, index + 1))
        return self.get_batch(index, index + 1)[0]

    def fetch(self, index, return_items=False):
        """The reference's `fetch` (loaders.py:65-84) with its return shapes, on top of the batch encode:

        cnn=True   `index` a slice / index array / list -> (B, C, max_seq_len) float32 on the device ('length batch emb ->
                   batch emb length' + .float(), written directly); a single int -> the single-sequence one-hot
                   `tokenizer.onehot_encode(seq, padlen=max_seq_len)` as float32, (max(L, padlen) + bos + eos, C) -- no
                   rearrangement, as in the reference.  return_items=True -> `(tensor, items)` with the (augmented) sequences
                   as bytearrays.  (The reference returns None here unless return_items is set -- it only `return`s inside
                   `if return_items:`; this returns the tensor.)
        cnn=False  `index` an int: the token row (max_seq_len,) of that sequence (`return_items` is ignored, as in the reference)."""
        if not self.cnn:
            return self[index]
        single = not isinstance(index, (slice, list, tuple, np.ndarray, torch.Tensor))
        if single:
            i = self._index(index)
            chars, offs = self._packed_device(i, i + 1)
        elif isinstance(index, slice):
            s, e, st = index.indices(len(self))
            idx = list(range(s, e, st))
            contiguous = st == 1 and idx
            chars, offs = self._packed_device(s, e) if contiguous else self._packed_device(0, 0, idx)
        else:
            on_dev = isinstance(index, torch.Tensor) and index.is_cuda
            chars, offs = self._packed_device(0, 0, index if on_dev else [self._index(i) for i in np.asarray(index.cpu() if isinstance(index, torch.Tensor) else index).ravel()])
        if self.augment:
            self._calls += 1
            blosum.augment_packed(chars, offs, self.augment, self.augment_frac, self._seed + self._calls)
        items = None
        if single or return_items:
            ho = offs.cpu().numpy()
            hc = chars[:int(ho[-1])].cpu().numpy()
            items = [bytearray(hc[ho[k]:ho[k + 1]].tobytes()) for k in range(len(ho) - 1)]
        if single:
            ret = self.tokenizer.onehot_encode(items[0], padlen=self.max_seq_len, destchar="f", device=self.device)
            items = items[0]
        else:
            ret = self.tokenizer.onehot_packed(chars, offs, self.max_seq_len, "f", layout="bcl", validate=not self._trusted_lengths)
        return (ret, items) if return_items else ret

    def access(self, slc, stop=None, step=None):
        """Range accessor with the reference's convention (loaders.py:105-111): an int `slc` is the START of
        slice(slc, stop, step) -- so access(i) alone runs from i to the end --, a slice is used as it is."""
        rng_ = slc if isinstance(slc, slice) else slice(slc, stop, step)
        return self[rng_]

    def cleanup(self):
        """Nothing to release (the reference's loader closes its memmap here)."""


class AugmentedSeqDataset(FlatFileDataset):
    def __init__(self, ff, tokenizer, augment=1, augment_frac=.5, **kw):
        super().__init__(ff, tokenizer, augment=augment, augment_frac=augment_frac, **kw)
