"""CPU: masked-LM batches over BPE ids (include/bsq.h, "BPE masked-LM") -- the declared symbols, the header's known answers, the
library's host twin bsq_bpe_mlm_tokenize_host against the independent statement of tests/bpe_mlm_twin.py byte for byte (fuzzed rows,
random legal tables, every flag set), frac 0 and 1, shards, what a token's fate must not depend on, cut and too-long rows, every
refusal with the outputs untouched, and the law of the draw.  No device is needed."""
import ctypes
import functools

import numpy as np
import pytest

import bpe_mlm_twin as mtwin
import bpe_twin as twin

LETTERS = {"DNA4": "ACGT", "AMINO20": "ACDEFGHIKLMNPQRSTVWY"}
KNOWN_ROWS = [b"AAAAAAA", b"ACGTACGT", b"AAACGTNAAAA", b"TTTTT"]  # plain ids 8 6 / 0 7 0 7 / 6 7 10 8 / 9 9 3
I = -100
KNOWN = {  # (frac, first_row): (inputs, labels) with mask_token written as "M"
    (0.5, 0): ([["M", "M"], [0, 7, "M", 7], [6, "M", 10, "M"], [2, 9, 3]], [[8, 6], [I, I, 0, 7], [I, 7, I, 8], [9, I, I]]),
    (0.5, 100): ([[8, "M"], [0, "M", 0, "M"], ["M", 7, 10, "M"], ["M", 9, 3]], [[I, 6], [I, 7, I, 7], [6, I, I, 8], [9, I, I]]),
    (1.0, 0): ([["M", "M"], ["M", "M", "M", 7], [6, "M", 10, "M"], [2, "M", "M"]], [[8, 6], [0, 7, 0, 7], [6, 7, I, 8], [9, 9, 3]]),
}


def _tok(key, eos=False, bos=False, padchar=False):
    import bioseq_amd
    return bioseq_amd.Tokenizer(key, eos, bos, padchar)


def _lut(tok):
    from bioseq_amd import capi
    d = capi.desc_of(tok)
    return np.array(list(d.lut), np.int64), d.nchars


@functools.lru_cache(maxsize=None)
def _trained(key="DNA4", n_merges=200, flags=(False, False, False)):
    from bioseq_amd import bpe
    rng = np.random.default_rng(len(key) + n_merges)
    rows = [twin.random_row(rng, 300, LETTERS[key]) for _ in range(40)] + [twin.low_complexity_row(rng, 300, LETTERS[key]) for _ in range(20)]
    return bpe.bpe_train_host(_tok(key, *flags), *twin.pack(rows), n_merges)


def _same(got, exp):
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape and g.tobytes() == e.tobytes()


def test_new_symbols_are_declared_and_exported():
    from bioseq_amd import bpe, capi
    L = capi.load()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_bpe_mlm_tokenize_device", "bsq_bpe_mlm_tokenize_host", "bsq_bpe_mlm_kernel_name"):
        assert n in names and hasattr(L, n), n
    assert "typedef struct bsq_bpe_mlm" in open(capi.HEADER_PATH).read()
    assert L.bsq_abi_version() == 7 and ctypes.sizeof(capi.BpeMlm) == 56
    for n in ("bpe_mlm_tokenize_packed", "bpe_mlm_tokenize_host", "bpe_mlm_kernel_name"):
        assert n in bpe.__all__ and callable(getattr(bpe, n))
    assert bpe.bpe_mlm_kernel_name() == "k_bpe_mlm_block" and bpe.bpe_mlm_kernel_name(max_chars=1024) == "k_bpe_mlm_wave"
    assert bpe.bpe_mlm_kernel_name(max_chars=300, form=2) == "k_bpe_mlm_block"
    with pytest.raises(ValueError):
        bpe.bpe_mlm_kernel_name(max_chars=1025, form=1)


@pytest.mark.parametrize("flags", [(False, False, False), (True, True, True)])
@pytest.mark.parametrize("case", sorted(KNOWN))
def test_known_answers_of_the_header(flags, case):
    """The three lines of the header; with BOS, EOS and PAD the mask token is 14 and the same tokens are selected."""
    from bioseq_amd import bpe
    frac, first_row = case
    eos, bos, padchar = (int(f) for f in flags)
    v = bpe.BPEVocab.from_merges(_tok("DNA4", *flags), twin.KNOWN_MERGES)
    mask = 11 + bos + eos + padchar
    assert bpe.bpe_vocab_size(v) == mask and mask == (14 if bos else 11)
    chars, offs = twin.pack(KNOWN_ROWS)
    P = 4 + bos + eos
    kw = dict(frac=frac, mask_prob=0.8, random_prob=0.1, seed=7, first_row=first_row)
    got = bpe.bpe_mlm_tokenize_host(v, chars, offs, P, "i", label_destchar="i", **kw)
    assert got[2].tolist() == [2, 4, 4, 3]
    want_in, want_lab = KNOWN[case]
    for k in range(4):
        n = len(want_in[k])
        ins = ([11] if bos else []) + [mask if x == "M" else x for x in want_in[k]] + ([12] if eos else [])
        labs = ([I] if bos else []) + want_lab[k]
        assert got[0][k].tolist() == (ins + [13 if padchar else 0] * P)[:P], (k, got[0][k])
        assert got[1][k].tolist() == (labs + [I] * P)[:P], (k, got[1][k])
        assert n == got[2][k]
    lut, C = _lut(v.tok)
    _same(got, mtwin.tokenize(lut, C, v.merges, flags, chars, offs, P, "i", label_destchar="i", **kw))


def test_the_headers_census_of_65536_tokens():
    """65 536 tokens of id 0 at seed 1, row 0, frac 0.15, V = 10: 9847 selected, 7888 masked, 858 random ids other than 0 (the twin's
    draw; the library's is held to the twin by every other test)."""
    ins, labs = mtwin.draw_row([0] * 65536, 10, 0, 0.15, 0.8, 0.1, 11, I, 1)
    ins, labs = np.array(ins), np.array(labs)
    assert (labs != I).sum() == 9847 and (ins == 11).sum() == 7888 and ((ins != 11) & (ins != 0)).sum() == 858


@pytest.mark.parametrize("key", ["DNA4", "AMINO20"])
@pytest.mark.parametrize("M", [0, 3, 17, 300])
def test_host_twin_equals_the_independent_draw_on_random_legal_tables(key, M):
    from bioseq_amd import bpe
    rng = np.random.default_rng(2000 * len(key) + M)
    flags = (True, True, True) if M != 3 else (False, True, False)
    tok = _tok(key, *flags)
    lut, C = _lut(tok)
    v = bpe.BPEVocab(tok, twin.random_table(rng, C, M))
    chars, offs = twin.pack(twin.fuzz_rows(rng, LETTERS[key], 48))
    P = 40  # (cuts some rows)
    for destchar, label_destchar, batch_first, frac in (("i", "q", True, 0.15), ("q", "h", False, 0.5), ("d", "f", True, 0.9)):
        kw = dict(label_destchar=label_destchar, frac=frac, seed=M + 5, first_row=3 * M, ignore_index=-1 if label_destchar == "h" else -100)
        exp = mtwin.tokenize(lut, C, v.merges, flags, chars, offs, P, destchar, batch_first, **kw)
        _same(bpe.bpe_mlm_tokenize_host(v, chars, offs, P, destchar, batch_first, **kw), exp)
    assert (exp[2] + 2 > P).any() and (exp[1] != -100).any() and (exp[1] == -100).any()


def test_frac_zero_is_the_plain_encode_and_frac_one_selects_every_token():
    from bioseq_amd import bpe
    v = _trained()
    rng = np.random.default_rng(9)
    chars, offs = twin.pack(twin.fuzz_rows(rng, "ACGT", 40, 300))
    for destchar, batch_first in (("h", True), ("q", False)):
        plain_t, plain_l = bpe.bpe_tokenize_host(v, chars, offs, 90, destchar, batch_first)
        ins, labs, lens = bpe.bpe_mlm_tokenize_host(v, chars, offs, 90, destchar, batch_first, frac=0.0, seed=3)
        assert ins.tobytes() == plain_t.tobytes() and lens.tobytes() == plain_l.tobytes() and (labs.view(np.int64) == -100).all()
        ins, labs, lens = bpe.bpe_mlm_tokenize_host(v, chars, offs, 90, destchar, batch_first, frac=1.0, seed=3, label_destchar="i")
        t = plain_t.astype(np.int64) if batch_first else plain_t.astype(np.int64).T
        lab = labs if batch_first else labs.T
        pos = np.arange(90)[None, :] < np.minimum(plain_l, 90)[:, None]
        token = pos & (t != v.M + 4)
        assert token.sum() > 1000 and (~token & pos).sum() > 5, "the batch needs tokens and UNKs"
        assert (lab[token] == t[token]).all() and (lab[~token] == -100).all()


def test_shards_with_first_row_concatenate_to_the_whole():
    from bioseq_amd import bpe
    v = _trained()
    rng = np.random.default_rng(10)
    rows = twin.fuzz_rows(rng, "ACGT", 30, 200)
    whole = bpe.bpe_mlm_tokenize_host(v, *twin.pack(rows), 70, "i", frac=0.3, seed=11, first_row=5)
    for cut in (1, 13):
        a = bpe.bpe_mlm_tokenize_host(v, *twin.pack(rows[:cut]), 70, "i", frac=0.3, seed=11, first_row=5)
        b = bpe.bpe_mlm_tokenize_host(v, *twin.pack(rows[cut:]), 70, "i", frac=0.3, seed=11, first_row=5 + cut)
        for w, x, y in zip(whole, a, b):
            assert np.concatenate([x, y]).tobytes() == w.tobytes()
    other = bpe.bpe_mlm_tokenize_host(v, *twin.pack(rows), 70, "i", frac=0.3, seed=11, first_row=6)
    assert other[1].tobytes() != whole[1].tobytes()


def test_a_tokens_fate_does_not_depend_on_padlen_layout_types_form_or_max_chars():
    from bioseq_amd import bpe
    v = _trained(n_merges=100)  # vocab 105: int8 holds it and the mask token
    rng = np.random.default_rng(12)
    chars, offs = twin.pack(twin.fuzz_rows(rng, "ACGT", 25, 120))
    kw = dict(frac=0.4, seed=21, first_row=2)
    base_in, base_lab, base_len = bpe.bpe_mlm_tokenize_host(v, chars, offs, 120, "q", **kw)
    base_in, base_lab = base_in.view(np.int64), base_lab.view(np.int64)
    assert (base_len <= 120).all() and (base_lab != -100).sum() > 100
    for P, destchar, label_destchar, batch_first, max_chars, form in ((120, "b", "b", False, 8192, 2), (333, "h", "d", True, 1024, 1),
                                                                      (121, "f", "i", False, 120, None), (200, "d", "h", True, 5000, None)):
        ins, labs, lens = bpe.bpe_mlm_tokenize_host(v, chars, offs, P, destchar, batch_first, label_destchar=label_destchar, max_chars=max_chars,
                                                    form=form, **kw)
        ins, labs = (ins, labs) if batch_first else (ins.T, labs.T)
        assert lens.tobytes() == base_len.tobytes()
        assert (ins[:, :120].astype(np.int64) == base_in).all() and (labs[:, :120].astype(np.int64) == base_lab).all()
        assert (labs[:, 120:] == -100).all()


@pytest.mark.parametrize("flags", [(False, False, False), (True, True, True), (True, False, False), (False, True, False)])
def test_cut_rows_and_a_matrix_of_one_position(flags):
    from bioseq_amd import bpe
    v = _trained(flags=flags)
    lut, C = _lut(v.tok)
    rng = np.random.default_rng(13)
    rows = [twin.random_row(rng, 200, "ACGT"), twin.random_row(rng, 30, "ACGT", 0.1), np.zeros(0, np.uint8)]
    chars, offs = twin.pack(rows)
    eos, bos, _ = (int(f) for f in flags)
    n = int(bpe.bpe_tokenize_host(v, chars, offs, 300)[1][0])
    for P in (1, 2, n + bos + eos - 1, n + bos + eos, n + bos + eos + 1):
        kw = dict(frac=0.5, seed=4)
        got = bpe.bpe_mlm_tokenize_host(v, chars, offs, P, "i", **kw)
        _same(got, mtwin.tokenize(lut, C, v.merges, flags, chars, offs, P, "i", **kw))
        assert got[2][0] == n
    if bos:
        got = bpe.bpe_mlm_tokenize_host(v, chars, offs, 1, "i", frac=1.0)
        assert got[0].ravel().tolist() == [v.M + 5] * 3 and (got[1].view(np.int64) == -100).all()  # BOS alone: nothing to select


def test_a_row_of_more_than_max_chars_characters():
    from bioseq_amd import bpe
    v = _trained(flags=(True, True, True))
    lut, C = _lut(v.tok)
    rng = np.random.default_rng(14)
    chars, offs = twin.pack([twin.random_row(rng, n, "ACGT") for n in (50, 51, 8193, 10)])
    for max_chars, k in ((50, 1), (8192, 2)):  # k: the first too-long row of this bound -- the inputs of an empty row, no label
        kw = dict(frac=1.0, seed=8, max_chars=max_chars)
        got = bpe.bpe_mlm_tokenize_host(v, chars, offs, 12, "h", **kw)
        _same(got, mtwin.tokenize(lut, C, v.merges, (True, True, True), chars, offs, 12, "h", **kw))
        assert got[2][k] == -1 and got[0][k, :3].tolist() == [v.M + 5, v.M + 6, v.M + 7] and (got[1][k].view(np.int64) == -100).all()
        assert got[2][3] > 0 and (got[1][3].view(np.int64) != -100).any()


def test_refused_calls_leave_the_outputs_untouched():
    from bioseq_amd import bpe, capi
    L = capi.load()
    v = _trained()  # V 204, vocab 205
    chars, offs = twin.pack(twin.fuzz_rows(np.random.default_rng(15), "ACGT", 6, 60))
    B, P = len(offs) - 1, 16
    nan = float("nan")

    def call(in_dt=capi.I16, lab_dt=capi.I16, max_chars=1024, form=0, reserved=0, M=v.M, tab=v.table.ctypes.data, padlen=P, rows=B, m="default",
             frac=0.15, mask_prob=0.8, random_prob=0.1, mask_token=205, ignore=-100, first_row=0, no_in=False, no_lab=False, no_len=False):
        ins, labs = np.full(B * P * 8, 0x5A, np.uint8), np.full(B * P * 8, 0x5A, np.uint8)
        lens = np.full(B * 4, 0x5A, np.uint8)
        mm = capi.BpeMlm(frac, mask_prob, random_prob, mask_token, ignore, 1, first_row)
        st = L.bsq_bpe_mlm_tokenize_host(ctypes.byref(v.desc), chars.ctypes.data, offs.ctypes.data, rows, padlen, 1, tab, M,
                                         ctypes.byref(capi.Bpe(max_chars, form, reserved)), ctypes.byref(mm) if m == "default" else None, in_dt,
                                         None if no_in else ins.ctypes.data, lab_dt, None if no_lab else labs.ctypes.data,
                                         None if no_len else lens.ctypes.data)
        return st, bool((ins == 0x5A).all()), bool((labs == 0x5A).all()), bool((lens == 0x5A).all())

    assert call() == (capi.OK, False, False, False)
    assert call(no_in=True) == (capi.OK, True, False, False) and call(no_lab=True) == (capi.OK, False, True, False)
    assert call(rows=0) == (capi.OK, True, True, True)  # B == 0: nothing is written
    for kw in (dict(max_chars=0), dict(max_chars=8193), dict(max_chars=1025, form=1), dict(form=3), dict(reserved=1), dict(M=70000), dict(tab=None),
               dict(padlen=0), dict(rows=-1), dict(no_len=True),  # what bsq_bpe_tokenize_host refuses
               dict(m=None), dict(frac=-0.1), dict(frac=1.5), dict(frac=nan), dict(mask_prob=nan), dict(random_prob=1.01), dict(mask_prob=-1.0),
               dict(mask_prob=0.7, random_prob=0.4), dict(first_row=-1), dict(mask_token=-1), dict(no_in=True, no_lab=True)):
        assert call(**kw) == (capi.ERR_INVALID_ARG, True, True, True), kw
        assert L.bsq_last_error()
    for kw in (dict(in_dt=capi.I8), dict(in_dt=capi.I16, mask_token=40000), dict(in_dt=capi.F32, mask_token=2 ** 24 + 1), dict(lab_dt=capi.I8),
               dict(lab_dt=capi.I16, ignore=-40000), dict(lab_dt=capi.I8, ignore=-100, M=v.M), dict(lab_dt=9), dict(in_dt=-1)):
        assert call(**kw) == (capi.ERR_DTYPE, True, True, True), kw
    assert call(in_dt=capi.I8, no_in=True)[0] == capi.ERR_DTYPE  # the input type is judged whether or not the inputs are asked for
    # the Python surface turns the same rules into ValueError
    for kw in (dict(frac=1.5), dict(mask_prob=0.7, random_prob=0.4), dict(first_row=-1), dict(mask_token=-2), dict(destchar="b"),
               dict(label_destchar="b"), dict(max_chars=1025, form=1), dict(destchar="h", mask_token=40000)):
        kw.setdefault("destchar", "h")
        with pytest.raises(ValueError):
            bpe.bpe_mlm_tokenize_host(v, chars, offs, P, kw.pop("destchar"), **kw)
    with pytest.raises(ValueError):
        bpe.bpe_mlm_tokenize_host(v, chars, offs, 0)


def test_the_law_of_the_draw():
    """At least 50 000 non-UNK tokens in rows of up to 1024 characters at frac 0.15, fixed seeds: the selected share, the mask share of
    the selected and the random share of the selected lie within 5 binomial standard deviations of 0.15, 0.8 and 0.1.  A random draw is
    counted as input != label and input != mask_token, corrected by (V - 1) / V for the draws that hit the token's own id."""
    from bioseq_amd import bpe
    v = _trained()
    V = v.M + 4
    rng = np.random.default_rng(16)
    rows = [twin.random_row(rng, int(n), "ACGT", 0.01) for n in rng.integers(600, 1025, 260)]
    chars, offs = twin.pack(rows)
    ins, labs, lens = bpe.bpe_mlm_tokenize_host(v, chars, offs, 1024, "i", label_destchar="i", frac=0.15, seed=2024, max_chars=1024)
    plain = bpe.bpe_tokenize_host(v, chars, offs, 1024, "i", max_chars=1024)[0]
    token = (np.arange(1024)[None, :] < lens[:, None]) & (plain != V)
    N = int(token.sum())
    assert N >= 50000 and (lens <= 1024).all()
    sel = labs != -100
    assert (sel & ~token).sum() == 0 and (labs[sel] == plain[sel]).all()
    S = int(sel.sum())
    masked = int((ins[sel] == V + 1).sum())
    random = ((ins[sel] != labs[sel]) & (ins[sel] != V + 1)).sum() / ((V - 1) / V)
    assert ((ins[sel] != V + 1) & (ins[sel] >= V)).sum() == 0, "a random id is a class or a merge product"
    assert abs(S / N - 0.15) <= 5 * np.sqrt(0.15 * 0.85 / N), (S, N)
    assert abs(masked / S - 0.8) <= 5 * np.sqrt(0.8 * 0.2 / S), (masked, S)
    assert abs(random / S - 0.1) <= 5 * np.sqrt(0.1 * 0.9 / S), (random, S)
    # the twin's draw over the same ids, row by row: the same selected set and inputs
    for b in (0, 100, 259):
        t_in, t_lab = mtwin.draw_row(plain[b, :lens[b]].tolist(), V, b, 0.15, 0.8, 0.1, V + 1, -100, 2024)
        assert ins[b, :lens[b]].tolist() == t_in and labs[b, :lens[b]].tolist() == t_lab
