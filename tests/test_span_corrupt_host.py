"""CPU: span-corruption (T5) batches (include/bsq.h, "span corruption") -- the declared symbols, the header's known answers, the
library's host twin bsq_span_corrupt_host against the independent statement of tests/span_corrupt_twin.py bit for bit (both tokenizers,
every flag set, spans 1 / 3 / 16, both sentinel steps, the max_sentinels cutoff, all 36 type pairs), every refusal, shards, what a
character's fate must not depend on, anchor_prob 0 against the tokenizer's rows as the header states them (the device encode itself is
compared in tests/test_span_corrupt_gpu.py), and span_restore.  No device is needed."""
import ctypes
import itertools

import numpy as np
import pytest

import span_corrupt_twin as twin

I = -100
KNOWN_ROWS = [b"ACGTACGTACGTACGTACGT", b"ACGNNCGTACGTAC", b"AC", b"", b"TTTTTTTTTTTTTTTTTTTTTTTT"]
KNOWN_KW = dict(anchor_prob=0.2, span=3, seed=7, first_row=0)
# flags, sentinel_first, max_sentinels -> row: (inputs, labels, in_len, tgt_len); the header's table
KNOWN = [
    ((False, False, False), 4, 100, {
        0: ([0, 1, 2, 3, 4, 3, 0, 5, 1, 2, 3, 0, 6, 0, 0, 0], [4, 0, 1, 2, 5, 1, 2, 3, 0, 6], 13, 13),
        1: ([4, 0, 0, 5, 3, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0], [4, 0, 1, 2, 5, 1, 2, 6, 1, 2], 7, 13),
        4: ([3, 3, 4, 3, 5, 3, 3, 3, 3, 6, 3, 0, 0, 0, 0, 0], [4, 3, 3, 3, 3, 5, 3, 3, 3, 6], 11, 19)}),
    ((False, False, False), 4, 1, {
        0: ([0, 1, 2, 3, 4, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1], [4, 0, 1, 2, I, I, I, I, I, I], 18, 4)}),
    ((True, True, True), 7, 100, {
        0: ([4, 0, 1, 2, 3, 7, 3, 0, 8, 1, 2, 3, 0, 9, 5, 6], [7, 0, 1, 2, 8, 1, 2, 3, 0, 5], 13, 13)}),
]
NP_OF = {"b": np.int8, "h": np.int16, "i": np.int32, "q": np.uint64, "f": np.float32, "d": np.float64}
POOLS = {"DNA4": np.frombuffer(b"ACGTACGTACGTACGTACGTACGTNacgt*\xff", np.uint8),
         "AMINO20": np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQRSTVWYXBZ*acd", np.uint8)}


def _tok(key, eos=False, bos=False, padchar=False):
    import bioseq_amd
    return bioseq_amd.Tokenizer(key, eos, bos, padchar)


def _desc(tok):
    from bioseq_amd import capi
    return capi.desc_of(tok)


def _pack(rows):
    chars = np.frombuffer(b"".join(rows), np.uint8)
    return chars, np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)


def _batch(rng, key, B, max_len):
    """Packed batch of random rows (some unmapped bytes), with an empty row, a one-character row and an all-unmapped row."""
    lens = rng.integers(0, max_len + 1, B).astype(np.int64)
    lens[:3] = (0, 1, 9)
    chars = rng.choice(POOLS[key], int(lens.sum())).astype(np.uint8)
    offs = np.zeros(B + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    chars[offs[2]:offs[3]] = ord("*")
    return chars, offs


def _same(got, exp):
    """The library's four results against the twin's, bit for bit, through the element types"""
    for g, e in zip(got[:2], exp[:2]):
        assert g.shape == e.shape and np.array_equal(twin.as_int64(g), e)
    assert got[2].dtype == np.int32 and got[3].dtype == np.int32
    assert np.array_equal(got[2], exp[2]) and np.array_equal(got[3], exp[3])


def test_new_symbols_are_declared_and_exported():
    from bioseq_amd import capi, masking
    L = capi.load()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_span_corrupt_device", "bsq_span_corrupt_host", "bsq_span_corrupt_kernel_name"):
        assert n in names and hasattr(L, n), n
    header = open(capi.HEADER_PATH).read()
    assert "typedef struct bsq_span_corrupt" in header and "span corruption" in header
    assert L.bsq_abi_version() == 7 and ctypes.sizeof(capi.SpanCorrupt) == 56
    for n in ("span_corrupt_packed", "span_corrupt_host", "span_corrupt_kernel_name", "span_restore"):
        assert n in masking.__all__ and callable(getattr(masking, n))
    assert masking.span_corrupt_kernel_name(_tok("DNA4"), 9, 16, 10) == "k_span_corrupt"


def test_known_answers_of_the_header():
    from bioseq_amd import masking
    chars, offs = _pack(KNOWN_ROWS)
    for flags, first, cutoff, rows in KNOWN:
        tok = _tok("DNA4", *flags)
        kw = dict(KNOWN_KW, sentinel_first=first, max_sentinels=cutoff)
        got = masking.span_corrupt_host(tok, chars, offs, 16, 10, "i", label_dtype="h", **kw)
        _same(got, twin.corrupt_batch(_desc(tok), chars, offs, 16, 10, **kw))
        for r, (inputs, labels, in_len, tgt_len) in rows.items():
            assert got[0][r].tolist() == inputs and got[1][r].tolist() == labels and (got[2][r], got[3][r]) == (in_len, tgt_len), (flags, cutoff, r)


@pytest.mark.parametrize("key", ["DNA4", "AMINO20"])
def test_c_twin_equals_the_numpy_twin(key):
    from bioseq_amd import masking
    cut_after_sentinel = cut_in_run = uncut = cutoff_hit = 0
    for n, (flags, span, step, cutoff) in enumerate(itertools.product(itertools.product((False, True), repeat=3), (1, 3, 16), (1, -1), (1, 2, 100))):
        rng = np.random.default_rng(17 * n + len(key))
        tok = _tok(key, *flags)
        chars, offs = _batch(rng, key, 12, 90)
        P_in, P_tgt = (int(v) for v in rng.choice([1, 2, 8, 31, 64, 100], 2))
        first = tok.alphabet_size() + (0 if step == 1 else cutoff - 1) + int(rng.integers(0, 3))
        kw = dict(anchor_prob=float(rng.choice([0.05, 0.2, 0.6, 1.0])), span=span, max_sentinels=cutoff, sentinel_first=first, sentinel_step=step,
                  ignore_index=int(rng.choice([-100, -1, 30000])), seed=int(rng.integers(0, 2 ** 63)), first_row=int(rng.integers(0, 2 ** 40)))
        exp = twin.corrupt_batch(_desc(tok), chars, offs, P_in, P_tgt, **kw)
        _same(masking.span_corrupt_host(tok, chars, offs, P_in, P_tgt, "i", label_dtype="q", **kw), exp)
        room = max(P_tgt - int(flags[0]), 0)
        for det, tgt_len in zip(exp[4], exp[3]):
            body = det["tgt_body"]
            sent = set(first + g * step for g in range(cutoff))
            cut_after_sentinel += int(0 < room < tgt_len and body[room - 1] in sent)
            cut_in_run += int(0 < room < tgt_len and body[room - 1] not in sent)
            uncut += int(tgt_len <= room)
            cutoff_hit += int(len(det["runs"]) > cutoff)
    assert cut_after_sentinel > 0 and cut_in_run > 0 and uncut > 0 and cutoff_hit > 0


def test_all_36_type_pairs_on_one_small_batch():
    from bioseq_amd import masking
    tok = _tok("AMINO20", True, True, True)
    chars, offs = _batch(np.random.default_rng(5), "AMINO20", 7, 60)
    kw = dict(anchor_prob=0.15, span=3, seed=11, sentinel_first=126, sentinel_step=-1, ignore_index=-100)
    exp = twin.corrupt_batch(_desc(tok), chars, offs, 40, 16, **kw)
    assert (exp[3] > 15).any() and (0 < exp[3]).any() and (exp[3] <= 15).any()  # cut and uncut label rows
    for dc, ldc in itertools.product("bhiqfd", repeat=2):
        got = masking.span_corrupt_host(tok, chars, offs, 40, 16, dc, label_dtype=ldc, **kw)
        assert got[0].dtype == NP_OF[dc] and got[1].dtype == NP_OF[ldc]
        _same(got, exp)


def _raw(tok, m, B=1, P_in=8, P_tgt=8, dt=3, ldt=3, inputs=True, labels=True, chars=b"ACGTACGT"):
    """bsq_span_corrupt_host on raw buffers: (status, inputs, labels); the buffers are filled with 99 before the call"""
    from bioseq_amd import capi
    L = capi.load()
    desc = capi.desc_of(tok)
    c = np.frombuffer(chars, np.uint8)
    offs = np.array([0] + [len(chars)] * B, np.int64)
    inp, lab = np.full((max(B, 1), max(P_in, 1)), 99, np.int64), np.full((max(B, 1), max(P_tgt, 1)), 99, np.int64)
    st = L.bsq_span_corrupt_host(ctypes.byref(desc), c.ctypes.data, offs.ctypes.data, B, P_in, P_tgt, ctypes.byref(m) if m is not None else None, dt,
                                 inp.ctypes.data if inputs else None, ldt, lab.ctypes.data if labels else None, None, None)
    return st, inp, lab


def test_every_refusal_leaves_the_outputs_untouched():
    from bioseq_amd import capi
    tok = _tok("DNA4", True, True, True)  # alphabet size 7

    def m(anchor_prob=0.2, span=3, max_sentinels=100, sentinel_first=7, sentinel_step=1, ignore_index=-100, seed=1, first_row=0):
        return capi.SpanCorrupt(anchor_prob, span, max_sentinels, sentinel_first, sentinel_step, ignore_index, seed, first_row)

    invalid = [dict(m=m(anchor_prob=-0.1)), dict(m=m(anchor_prob=1.5)), dict(m=m(anchor_prob=float("nan"))), dict(m=m(span=0)), dict(m=m(span=17)),
               dict(m=m(max_sentinels=0)), dict(m=m(max_sentinels=65536)), dict(m=m(sentinel_step=0)), dict(m=m(sentinel_step=2)),
               dict(m=m(sentinel_first=2 ** 31 - 50)), dict(m=m(sentinel_first=50, sentinel_step=-1)), dict(m=m(sentinel_first=-1)),
               dict(m=m(sentinel_first=6)), dict(m=m(sentinel_first=105, sentinel_step=-1)), dict(m=m(first_row=-1)), dict(m=m(), P_in=0),
               dict(m=m(), P_tgt=0), dict(m=m(), P_in=-3), dict(m=m(), inputs=False, labels=False), dict(m=None)]
    for kw in invalid:
        st, inp, lab = _raw(tok, **kw)
        assert st == capi.ERR_INVALID_ARG, kw
        assert (inp == 99).all() and (lab == 99).all()
    # sentinel_first 106 counting down reaches 7: the smallest legal range; 2^31 - 100 counting up reaches 2^31 - 1
    assert _raw(tok, m(sentinel_first=106, sentinel_step=-1))[0] == capi.OK and _raw(tok, m(sentinel_first=2 ** 31 - 100))[0] == capi.OK
    # by bsq_dtype_holds: the largest sentinel into the input type; ignore_index and the largest sentinel into the label type
    dtype = [dict(m=m(sentinel_first=100), dt=capi.I8), dict(m=m(sentinel_first=32700), dt=capi.I16), dict(m=m(sentinel_first=2 ** 24), dt=capi.F32),
             dict(m=m(ignore_index=-200), ldt=capi.I8), dict(m=m(ignore_index=40000), ldt=capi.I16), dict(m=m(sentinel_first=32700), ldt=capi.I16),
             dict(m=m(ignore_index=2 ** 24 + 1), ldt=capi.F32), dict(m=m(), dt=6), dict(m=m(), ldt=-1)]
    for kw in dtype:
        st, inp, lab = _raw(tok, **kw)
        assert st == capi.ERR_DTYPE, kw
        assert (inp == 99).all() and (lab == 99).all()
    assert _raw(tok, m(sentinel_first=127, sentinel_step=-1), dt=capi.I8, ldt=capi.I8)[0] == capi.OK  # 28 .. 127 and -100 into int8
    assert _raw(tok, m(max_sentinels=10), dt=capi.I8, ldt=capi.I8)[0] == capi.OK
    # the type of a matrix that is left out is not asked
    assert _raw(tok, m(ignore_index=-200), ldt=capi.I8, labels=False)[0] == capi.OK and _raw(tok, m(sentinel_first=100), dt=capi.I8, inputs=False)[0] == capi.OK
    assert _raw(tok, m(), ldt=7, labels=False)[0] == capi.ERR_DTYPE
    # B == 0 is OK and writes nothing; either matrix may be left out
    st, inp, lab = _raw(tok, m(), B=0)
    assert st == capi.OK and (inp == 99).all() and (lab == 99).all()
    st, inp, lab = _raw(tok, m(), inputs=False)
    assert st == capi.OK and (inp == 99).all() and not (lab == 99).any()
    st, inp, lab = _raw(tok, m(), labels=False)
    assert st == capi.OK and (lab == 99).all() and not (inp == 99).any()


def test_python_checks_its_arguments_first():
    from bioseq_amd import masking
    tok = _tok("DNA4", True, True, True)
    chars, offs = _pack(KNOWN_ROWS)
    bad = [dict(frac=1.5), dict(anchor_prob=-0.5), dict(anchor_prob=float("nan")), dict(frac=0.3, anchor_prob=0.1), dict(span=0), dict(span=17),
           dict(span=2.5), dict(max_sentinels=0), dict(max_sentinels=65536), dict(sentinel_step=0), dict(sentinel_step=2), dict(sentinel_first=6),
           dict(sentinel_first=50, sentinel_step=-1), dict(sentinel_first=2 ** 31 - 5), dict(first_row=-1), dict(destchar="b", sentinel_first=100),
           dict(label_dtype="b", ignore_index=-200), dict(destchar="x"), dict(label_dtype="h", sentinel_first=40000)]
    for kw in bad:
        with pytest.raises(ValueError):
            masking.span_corrupt_host(tok, chars, offs, 16, 10, **kw)
        with pytest.raises(ValueError):  # (before the batch is looked at: these are no device tensors)
            masking.span_corrupt_packed(tok, chars, offs, 16, 10, **kw)
    for widths in ((0, 10), (16, 0), (-1, 10)):
        with pytest.raises(ValueError):
            masking.span_corrupt_host(tok, chars, offs, *widths)
    with pytest.raises(ValueError):
        masking.span_corrupt_kernel_name(tok, 4, 16, 10, "b", sentinel_first=100)
    with pytest.raises(ValueError):  # a packed batch on the host is not what the device call takes
        masking.span_corrupt_packed(tok, chars, offs, 16, 10)


def test_shards_drawn_with_their_first_row_equal_the_whole():
    from bioseq_amd import masking
    tok = _tok("AMINO20", True, False, True)
    chars, offs = _batch(np.random.default_rng(3), "AMINO20", 11, 120)
    kw = dict(frac=0.3, span=3, seed=5)
    whole = masking.span_corrupt_host(tok, chars, offs, 100, 60, first_row=40, **kw)
    h = 5
    head = masking.span_corrupt_host(tok, chars[:offs[h]], offs[:h + 1], 100, 60, first_row=40, **kw)
    tail = masking.span_corrupt_host(tok, chars[offs[h]:], offs[h:] - offs[h], 100, 60, first_row=40 + h, **kw)
    for w, a, b in zip(whole, head, tail):
        assert np.array_equal(w, np.concatenate([a, b]))
    other = masking.span_corrupt_host(tok, chars, offs, 100, 60, first_row=41, **kw)
    assert not np.array_equal(whole[0], other[0])


def test_the_head_of_a_row_does_not_depend_on_the_widths_or_types():
    from bioseq_amd import masking
    tok = _tok("DNA4", False, True, False)
    chars, offs = _batch(np.random.default_rng(9), "DNA4", 8, 3000)
    kw = dict(frac=0.15, span=3, seed=21, max_sentinels=100)
    wide = masking.span_corrupt_host(tok, chars, offs, 4096, 4096, **kw)
    small = masking.span_corrupt_host(tok, chars, offs, 8, 8, "h", label_dtype="f", **kw)
    assert np.array_equal(twin.as_int64(small[0]), twin.as_int64(wide[0])[:, :8])
    assert np.array_equal(twin.as_int64(small[1]), twin.as_int64(wide[1])[:, :8])
    assert np.array_equal(small[2], wide[2]) and np.array_equal(small[3], wide[3])
    assert (small[2] > 7).any() and (small[3] > 8).any()  # rows that P = 8 cuts


@pytest.mark.parametrize("flags", list(itertools.product((False, True), repeat=3)))
def test_anchor_prob_0_equals_tokenize(flags):
    """anchor_prob = 0: the inputs are the rows the tokenizer writes for the same batch -- here as include/bsq.h states them ([BOS] ids
    [EOS] PAD, 0 for an unmapped byte and for a pad position without padchar; the encode itself runs on the device, and
    tests/test_span_corrupt_gpu.py compares with tokenize_packed there) -- and the labels hold only [EOS]"""
    from bioseq_amd import masking
    tok = _tok("AMINO20", *flags)
    d = _desc(tok)
    rng = np.random.default_rng(2)
    chars, offs = _batch(rng, "AMINO20", 9, 50)
    P = 53
    inputs, labels, in_len, tgt_len = masking.span_corrupt_host(tok, chars, offs, P, 4, "b", anchor_prob=0.0)
    plain = np.full((9, P), d.nchars + int(flags[0]) + int(flags[1]) if flags[2] else 0, np.int8)
    for b in range(9):
        ids = [max(int(d.lut[c]), 0) for c in chars[offs[b]:offs[b + 1]]]
        row = [d.nchars] * int(flags[1]) + ids + [d.nchars + int(flags[1])] * int(flags[0])
        plain[b, :len(row)] = row
    assert plain.shape == inputs.shape and np.array_equal(plain, inputs)
    eos = int(flags[0])
    assert np.array_equal(in_len, np.diff(offs)) and not tgt_len.any()
    assert (twin.as_int64(labels)[:, eos:] == -100).all() and (not eos or (twin.as_int64(labels)[:, 0] == 20 + int(flags[1])).all())


def test_anchor_prob_1_cuts_every_run_of_mapped_characters():
    from bioseq_amd import masking
    tok = _tok("DNA4")
    chars, offs = _pack([b"ACGTNNACNT", b"NNNN", b"A"])
    inputs, labels, in_len, tgt_len = masking.span_corrupt_host(tok, chars, offs, 8, 12, anchor_prob=1.0, span=1)
    assert twin.as_int64(inputs).tolist() == [[4, 0, 0, 5, 0, 6, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0], [4, 0, 0, 0, 0, 0, 0, 0]]
    assert twin.as_int64(labels).tolist() == [[4, 0, 1, 2, 3, 5, 0, 1, 6, 3, I, I], [I] * 12, [4, 0] + [I] * 10]
    assert in_len.tolist() == [6, 4, 1] and tgt_len.tolist() == [10, 0, 2]


@pytest.mark.parametrize("flags", [(False, False, False), (True, True, True), (False, True, False), (True, False, True)])
def test_span_restore_of_uncut_rows_is_the_plain_body(flags):
    from bioseq_amd import masking
    tok = _tok("AMINO20", *flags)
    d = _desc(tok)
    chars, offs = _batch(np.random.default_rng(4), "AMINO20", 10, 80)
    for step, first, cutoff in ((1, None, 100), (-1, 200, 100), (1, 50, 3)):
        kw = dict(sentinel_first=first, sentinel_step=step, max_sentinels=cutoff)
        inputs, labels, in_len, tgt_len = masking.span_corrupt_host(tok, chars, offs, 90, 130, frac=0.3, seed=8, **kw)
        assert (in_len <= 90 - int(flags[0]) - int(flags[1])).all() and (tgt_len <= 130 - int(flags[0])).all() and (tgt_len > 0).any()
        bodies = masking.span_restore(twin.as_int64(inputs), twin.as_int64(labels), tok, in_len=in_len, **kw)
        for b, body in enumerate(bodies):
            plain = [max(int(d.lut[c]), 0) for c in chars[offs[b]:offs[b + 1]]]
            assert body.tolist() == plain, (flags, step, b)
        if flags[0]:  # with an EOS the body ends there: in_len is not needed
            again = masking.span_restore(twin.as_int64(inputs), twin.as_int64(labels), tok, **kw)
            assert all(np.array_equal(a, b) for a, b in zip(again, bodies))
    cut = masking.span_corrupt_host(tok, chars, offs, 90, 6, frac=0.3, seed=8)
    with pytest.raises(ValueError):
        masking.span_restore(twin.as_int64(cut[0]), twin.as_int64(cut[1]), tok, in_len=cut[2])
