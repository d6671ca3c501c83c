"""CPU: BPE ids of packed batches (include/bsq.h, "BPE ids of a packed batch") -- the declared symbols, the header's known answers,
the library's host twin bsq_bpe_tokenize_host (the step form) against the one-merge-at-a-time programme of tests/bpe_twin.py on fuzzed
rows over trained and random legal tables, every refusal with the outputs untouched, the largest legal table, the Python surface
(from_merges, from_tokenizers_json, strings, decode, external ids, the trainer) and token strings against Hugging Face's BPE where the
`tokenizers` package is present.  No device is needed."""
import ctypes
import functools
import json

import numpy as np
import pytest

import bpe_twin as twin

LETTERS = {"DNA4": "ACGT", "AMINO20": "ACDEFGHIKLMNPQRSTVWY"}


def _tok(key, eos=False, bos=False, padchar=False):
    import bioseq_amd
    return bioseq_amd.Tokenizer(key, eos, bos, padchar)


def _lut(tok):
    from bioseq_amd import capi
    d = capi.desc_of(tok)
    return np.array(list(d.lut), np.int64), d.nchars


def _known_vocab():
    from bioseq_amd import bpe
    return bpe.BPEVocab.from_merges(_tok("DNA4"), twin.KNOWN_MERGES)


@functools.lru_cache(maxsize=None)
def _trained(key, n_merges):
    from bioseq_amd import bpe
    rng = np.random.default_rng(len(key) + n_merges)
    rows = [twin.random_row(rng, 300, LETTERS[key]) for _ in range(40)] + [twin.low_complexity_row(rng, 300, LETTERS[key]) for _ in range(20)]
    return bpe.bpe_train_host(_tok(key), *twin.pack(rows), n_merges)


def test_new_symbols_are_declared_and_exported():
    import bioseq_amd
    from bioseq_amd import bpe, capi
    L = capi.load()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_bpe_table_bytes", "bsq_bpe_table_build", "bsq_bpe_vocab_size", "bsq_bpe_unk_id", "bsq_bpe_bos_id", "bsq_bpe_eos_id",
              "bsq_bpe_pad_id", "bsq_bpe_tokenize_device", "bsq_bpe_tokenize_host", "bsq_bpe_kernel_name"):
        assert n in names and hasattr(L, n), n
    assert "typedef struct bsq_bpe" in open(capi.HEADER_PATH).read()
    assert L.bsq_abi_version() == 7 and ctypes.sizeof(capi.Bpe) == 12
    assert "bpe" in bioseq_amd.__all__
    for n in ("BPEVocab", "bpe_tokenize_packed", "bpe_tokenize_host", "bpe_vocab_size", "bpe_special_ids", "bpe_strings", "bpe_decode",
              "bpe_external_ids", "bpe_kernel_name", "bpe_train_host"):
        assert n in bpe.__all__ and callable(getattr(bpe, n))
    assert bpe.TOO_LONG == -1


def test_known_answers_of_the_header():
    from bioseq_amd import bpe
    v = _known_vocab()
    assert v.M == 6 and bpe.bpe_vocab_size(v) == 11 and bpe.bpe_special_ids(v) == {"unk": 10, "bos": -1, "eos": -1, "pad": 11}
    assert bpe.bpe_strings(v) == ["A", "C", "G", "T", "AA", "CG", "AAA", "CGT", "AAAA", "TT", "<UNK>"]
    chars, offs = twin.pack([r for r, _ in twin.KNOWN])
    tokens, lengths = bpe.bpe_tokenize_host(v, chars, offs, 5, "i")
    assert tokens.dtype == np.int32 and lengths.dtype == np.int32
    lut, C = _lut(v.tok)
    for k, (row, ids) in enumerate(twin.KNOWN):
        assert lengths[k] == len(ids) and tokens[k].tolist() == ids + [0] * (5 - len(ids)), row
        assert twin.row_ids(lut, C, v.merges, row) == ids, row  # (the independent programme agrees with the header too)


@pytest.mark.parametrize("flags", [(False, False, False), (True, True, True), (True, False, False), (False, True, True)])
def test_specials_follow_the_kmer_order(flags):
    from bioseq_amd import bpe, kmers
    tok = _tok("DNA4", *flags)
    v = bpe.BPEVocab.from_merges(tok, twin.KNOWN_MERGES)
    eos, bos, padchar = flags
    sp = bpe.bpe_special_ids(v)
    assert sp["unk"] == 10 and sp["bos"] == (11 if bos else -1) and sp["eos"] == (11 + bos if eos else -1) and sp["pad"] == 11 + bos + eos
    assert bpe.bpe_vocab_size(v) == 11 + bos + eos + padchar
    ksp = kmers.kmer_special_ids(tok, 1)  # the same order behind UNK, whatever V is
    assert {k: (x - sp["unk"] if x >= 0 else x) for k, x in sp.items()} == {k: (x - ksp["unk"] if x >= 0 else x) for k, x in ksp.items()}


@pytest.mark.parametrize("key", ["DNA4", "AMINO20"])
@pytest.mark.parametrize("M", [0, 1, 2, 3, 17, 300, 3000])
def test_host_twin_equals_one_merge_at_a_time_on_random_legal_tables(key, M):
    from bioseq_amd import bpe
    rng = np.random.default_rng(1000 * len(key) + M)
    tok = _tok(key, True, True, True)
    lut, C = _lut(tok)
    v = bpe.BPEVocab(tok, twin.random_table(rng, C, M))
    chars, offs = twin.pack(twin.fuzz_rows(rng, LETTERS[key], 48))
    P = 40  # (cuts some rows: lengths keep the clamp-free count)
    for destchar, batch_first in (("i", True), ("q", False)):
        exp_t, exp_l = twin.tokenize(lut, C, v.merges, (True, True, True), chars, offs, P, destchar, batch_first)
        got_t, got_l = bpe.bpe_tokenize_host(v, chars, offs, P, destchar, batch_first)
        assert got_t.dtype == exp_t.dtype and got_t.shape == exp_t.shape and got_t.tobytes() == exp_t.tobytes()
        assert got_l.tobytes() == exp_l.tobytes()
    if M >= 17:
        assert (exp_l + 2 > P).any() and (exp_l < np.diff(offs)).any(), "no row is cut or no merge fires: the case shows nothing"


@pytest.mark.parametrize("key,n_merges", [("DNA4", 200), ("AMINO20", 150)])
def test_host_twin_equals_one_merge_at_a_time_on_trained_tables(key, n_merges):
    from bioseq_amd import bpe
    v = _trained(key, n_merges)
    assert v.M == n_merges
    rng = np.random.default_rng(77)
    lut, C = _lut(v.tok)
    rows = twin.fuzz_rows(rng, LETTERS[key], 60, 260) + [np.full(n, ord("A"), np.uint8) for n in (1, 2, 3, 63, 64, 65, 127, 128, 129, 200)]
    chars, offs = twin.pack(rows)
    exp_t, exp_l = twin.tokenize(lut, C, v.merges, (False, False, False), chars, offs, 260, "h")
    got_t, got_l = bpe.bpe_tokenize_host(v, chars, offs, 260, "h")
    assert got_t.tobytes() == exp_t.tobytes() and got_l.tobytes() == exp_l.tobytes()
    assert (exp_l < np.diff(offs)).sum() > len(rows) // 2, "merges should fire in most rows: the case shows nothing otherwise"


def test_run_parity_on_poly_a_rows_of_every_length():
    """(A,A), (AA,AA), (AA,A): runs of equal candidates across the 64-position words of the twin."""
    from bioseq_amd import bpe
    v = bpe.BPEVocab.from_merges(_tok("DNA4"), [("A", "A"), ("AA", "AA"), ("AA", "A")])
    lut, C = _lut(v.tok)
    chars, offs = twin.pack([np.full(n, ord("A"), np.uint8) for n in range(1, 201)])
    exp_t, exp_l = twin.tokenize(lut, C, v.merges, (False, False, False), chars, offs, 64, "b")
    got_t, got_l = bpe.bpe_tokenize_host(v, chars, offs, 64, "b")
    assert got_t.tobytes() == exp_t.tobytes() and got_l.tobytes() == exp_l.tobytes()
    assert got_l[6] == 2 and got_t[6, :2].tolist() == [5, 6]  # AAAAAAA = AAAA AAA


def test_largest_legal_table_on_a_poly_a_row():
    """C + M + 4 == 65536 as the chain (A,A), (AA,A), (AAA,A) ...: the table is 1 MiB, every id fits 16 bits."""
    from bioseq_amd import bpe, capi
    tok = _tok("DNA4", True, True, True)
    M = 65536 - 4 - 4
    merges = np.zeros((M, 2), np.int64)
    merges[1:, 0] = 4 + np.arange(M - 1)
    v = bpe.BPEVocab(tok, merges)
    assert v.table.nbytes == 1 << 20 == capi.load().bsq_bpe_table_bytes(4, M)
    assert bpe.bpe_vocab_size(v) == 65536 and bpe.bpe_special_ids(v) == {"unk": 65532, "bos": 65533, "eos": 65534, "pad": 65535}
    lut, C = _lut(tok)
    chars, offs = twin.pack([np.full(n, ord("A"), np.uint8) for n in (301, 300, 3)] + [b"AANAAA"])
    exp_t, exp_l = twin.tokenize(lut, C, v.merges, (True, True, True), chars, offs, 160, "i")
    got_t, got_l = bpe.bpe_tokenize_host(v, chars, offs, 160, "i")
    assert got_t.tobytes() == exp_t.tobytes() and got_l.tolist() == exp_l.tolist() == [150, 150, 1, 3]
    assert got_t[0, :3].tolist() == [65533, 4, 4] and got_t[0, 150:153].tolist() == [5, 65534, 65535] and got_t[3, 1:4].tolist() == [4, 65532, 5]
    with pytest.raises(ValueError):
        bpe.bpe_tokenize_host(v, chars, offs, 160, "h")  # int16 does not hold 65535
    with pytest.raises(ValueError):
        bpe.BPEVocab(tok, np.vstack([merges, [[0, 1]]]))  # V + 4 > 65536
    assert capi.load().bsq_bpe_table_bytes(4, M + 1) == -capi.ERR_INVALID_ARG


def _raw_host(v, chars, offs, P, dt, np_t, max_chars=8192, form=0, reserved=0, M=None, table=True):
    """bsq_bpe_tokenize_host itself on guarded buffers: (status, tokens untouched, lengths untouched)."""
    from bioseq_amd import capi
    L = capi.load()
    B = len(offs) - 1
    tokens = np.full(B * P, 0xAB, np.uint8).repeat(np.dtype(np_t).itemsize)
    lengths = np.full(B * 4, 0xAB, np.uint8)
    bpe = capi.Bpe(max_chars, form, reserved)
    st = L.bsq_bpe_tokenize_host(ctypes.byref(v.desc), chars.ctypes.data, offs.ctypes.data, B, P, 1, v.table.ctypes.data if table else None,
                                 v.M if M is None else M, ctypes.byref(bpe), dt, tokens.ctypes.data, lengths.ctypes.data)
    return st, bool((tokens == 0xAB).all()), bool((lengths == 0xAB).all())


def test_every_refusal_leaves_the_outputs_untouched():
    from bioseq_amd import bpe, capi
    L = capi.load()
    tok = _tok("DNA4")
    d = capi.desc_of(tok)
    out = np.full(bpe.BPEVocab(tok, [(0, 0)]).table.nbytes, 0xAB, np.uint8)

    def build(pairs):
        m = np.ascontiguousarray(np.array(pairs, np.int32).reshape(-1, 2))
        return L.bsq_bpe_table_build(ctypes.byref(d), m.ctypes.data, len(m), out.ctypes.data)

    for pairs in ([(4, 0)], [(0, 4)], [(0, 0), (5, 0)], [(-1, 0)], [(0, 1), (2, 3), (0, 1)]):  # forward references, a negative id, a duplicate
        assert build(pairs) == capi.ERR_INVALID_ARG and (out == 0xAB).all(), pairs
        assert L.bsq_last_error()
        with pytest.raises(ValueError):
            bpe.BPEVocab(tok, pairs)
    assert build([(0, 0), (4, 0)]) == capi.OK and not (out == 0xAB).all()
    assert L.bsq_bpe_table_build(ctypes.byref(d), None, 1, out.ctypes.data) == capi.ERR_INVALID_ARG
    assert L.bsq_bpe_vocab_size(ctypes.byref(d), 65529) == -capi.ERR_INVALID_ARG and L.bsq_bpe_vocab_size(ctypes.byref(d), -1) == -capi.ERR_INVALID_ARG

    v = bpe.BPEVocab(tok, twin.random_table(np.random.default_rng(5), 4, 200))  # vocab 205: beyond int8
    chars, offs = twin.pack([b"ACGTACGT", b"AAAA"])
    assert _raw_host(v, chars, offs, 8, capi.I16, np.int16) == (capi.OK, False, False)
    assert _raw_host(v, chars, offs, 8, capi.I8, np.int8) == (capi.ERR_DTYPE, True, True)
    assert _raw_host(v, chars, offs, 8, 6, np.int16) == (capi.ERR_DTYPE, True, True)
    for kw in (dict(max_chars=0), dict(max_chars=8193), dict(form=1, max_chars=1025), dict(form=3), dict(form=-1), dict(reserved=1), dict(M=65529),
               dict(table=False)):
        assert _raw_host(v, chars, offs, 8, capi.I16, np.int16, **kw) == (capi.ERR_INVALID_ARG, True, True), kw
    assert _raw_host(v, chars, offs, 0, capi.I16, np.int16)[0] == capi.ERR_INVALID_ARG
    assert _raw_host(v, chars, offs, 8, capi.I16, np.int16, form=1, max_chars=1024)[0] == capi.OK
    # the Python surface: ValueError before anything is called
    for kw in (dict(destchar="b"), dict(max_chars=0), dict(max_chars=8193), dict(form=1, max_chars=1025), dict(form=3)):
        with pytest.raises(ValueError):
            bpe.bpe_tokenize_host(v, chars, offs, 8, **kw)
    assert (bpe.bpe_kernel_name(v, max_chars=1024), bpe.bpe_kernel_name(v, max_chars=1025), bpe.bpe_kernel_name(v),
            bpe.bpe_kernel_name(v, max_chars=100, form=2)) == ("k_bpe_wave", "k_bpe_block", "k_bpe_block", "k_bpe_block")
    with pytest.raises(ValueError):
        bpe.bpe_kernel_name(v, max_chars=1025, form=1)


def test_too_long_rows_negative_lengths_and_empty_batches():
    from bioseq_amd import bpe
    v = _known_vocab()
    chars, offs = twin.pack([b"AAAA", b"AAAAA", b"", b"CG"])
    tokens, lengths = bpe.bpe_tokenize_host(v, chars, offs, 3, "q", max_chars=4)
    assert lengths.tolist() == [1, -1, 0, 1] and tokens.tolist() == [[8, 0, 0], [0, 0, 0], [0, 0, 0], [5, 0, 0]]
    bad = np.array([0, 4, 2, 6], np.int64)  # the middle row reads as -2 characters: it counts as 0
    tokens, lengths = bpe.bpe_tokenize_host(v, chars, bad, 3, "q")
    assert lengths.tolist() == [1, 0, 1] and tokens[1].tolist() == [0, 0, 0]
    tokens, lengths = bpe.bpe_tokenize_host(v, np.zeros(0, np.uint8), np.zeros(1, np.int64), 3)
    assert tokens.shape == (0, 3) and lengths.shape == (0,)
    # P = 1 with BOS and EOS: room for no id, BOS alone
    vb = bpe.BPEVocab.from_merges(_tok("DNA4", True, True, True), twin.KNOWN_MERGES)
    tokens, lengths = bpe.bpe_tokenize_host(vb, chars, offs, 1, "i")
    assert tokens.ravel().tolist() == [11] * 4 and lengths.tolist() == [1, 2, 0, 1]


def test_from_merges_folds_case_and_aliases_and_finds_duplicates(tmp_path):
    from bioseq_amd import bpe
    tok = _tok("DNA4")
    v = bpe.BPEVocab.from_merges(tok, [("a", "A"), ("aa", "c"), ("AAC", "g")])
    assert v.merges.tolist() == [[0, 0], [4, 1], [5, 2]] and v.merges.dtype == np.int32
    with pytest.raises(ValueError, match="fold to one pair"):
        bpe.BPEVocab.from_merges(tok, [("A", "C"), ("a", "c")])
    with pytest.raises(ValueError, match="neither a class"):
        bpe.BPEVocab.from_merges(tok, [("AC", "G")])
    with pytest.raises(ValueError, match="does not map"):
        bpe.BPEVocab.from_merges(tok, [("A", "N")])
    doc = {"model": {"type": "BPE", "merges": ["A A", ["AA", "C"]]}}
    assert bpe.BPEVocab.from_tokenizers_json(tok, doc).merges.tolist() == [[0, 0], [4, 1]]
    path = tmp_path / "tokenizer.json"
    path.write_text(json.dumps(doc))
    assert bpe.BPEVocab.from_tokenizers_json(tok, str(path)).merges.tolist() == [[0, 0], [4, 1]]
    with pytest.raises(ValueError):
        bpe.BPEVocab.from_tokenizers_json(tok, {"model": {"merges": ["A A C"]}})


def test_decode_round_trip_and_external_ids():
    from bioseq_amd import bpe
    v = _trained("DNA4", 200)
    rng = np.random.default_rng(3)
    rows = [twin.random_row(rng, int(n), "ACGT") for n in rng.integers(0, 300, 30)]
    chars, offs = twin.pack(rows)
    tokens, lengths = bpe.bpe_tokenize_host(v, chars, offs, 300, "i")
    for k, row in enumerate(rows):
        assert "".join(bpe.bpe_decode(v, tokens[k, :lengths[k]])) == bytes(row).decode()
    assert bpe.bpe_decode(v, np.int64(4)) == bpe.bpe_strings(v)[4]
    with pytest.raises(ValueError):
        bpe.bpe_decode(v, [bpe.bpe_vocab_size(v)])
    strings = bpe.bpe_strings(v)
    foreign = {s: 1000 + i for i, s in enumerate(strings[:50])}
    foreign["[UNK]"] = 7
    ext = bpe.bpe_external_ids(v, foreign, unk="[UNK]")
    assert ext.dtype == np.int64 and ext.shape == (bpe.bpe_vocab_size(v),)
    assert ext[:50].tolist() == list(range(1000, 1050)) and ext[bpe.bpe_special_ids(v)["unk"]] == 7
    assert all(ext[i] == foreign.get(strings[i], -1) for i in range(50, 204))


def test_trainer_is_deterministic_and_counts_without_overlap():
    from bioseq_amd import bpe
    tok = _tok("DNA4")
    rng = np.random.default_rng(9)
    chars, offs = twin.pack([twin.random_row(rng, 200, "ACGT", 0.02) for _ in range(30)])
    a, b = bpe.bpe_train_host(tok, chars, offs, 64), bpe.bpe_train_host(tok, chars.copy(), offs.copy(), 64)
    assert a.M == 64 and a.merges.tobytes() == b.merges.tobytes() and a.table.tobytes() == b.table.tobytes()
    assert bpe.bpe_train_host(tok, chars, offs, 10).merges.tolist() == a.merges[:10].tolist()
    # AAA AAA: (A,A) occurs twice without overlap, (C,G) three times -> CG first, then AA, then (AA, A); CG CG CG holds (CG, CG) once
    v = bpe.bpe_train_host(tok, *twin.pack([b"AAA", b"AAA", b"CGCGCG"]), 10)
    assert v.merges.tolist() == [[1, 2], [0, 0], [5, 0]]
    # ties go to the smallest (l, r); a best count below 2 stops; rows and unmapped bytes are barriers
    assert bpe.bpe_train_host(tok, *twin.pack([b"TGTGACAC"]), 1).merges.tolist() == [[0, 1]]
    assert bpe.bpe_train_host(tok, *twin.pack([b"AC", b"GT", b"ANC"]), 5).M == 0


def test_token_strings_equal_hugging_face_bpe():
    """models.BPE over our strings and merges, no pre-tokenizer: a row is one word.  (Comparable only while no two merges spell one
    string -- Hugging Face keys its vocabulary by string -- which the trained table is asserted to satisfy.)"""
    tokenizers = pytest.importorskip("tokenizers")
    from bioseq_amd import bpe
    v = _trained("DNA4", 200)
    strings = bpe.bpe_strings(v)
    assert len(set(strings)) == len(strings)
    hf = tokenizers.Tokenizer(tokenizers.models.BPE(vocab={s: i for i, s in enumerate(strings)},
                                                    merges=[(strings[l], strings[r]) for l, r in v.merges.tolist()], unk_token="<UNK>"))
    rng = np.random.default_rng(11)
    rows = [twin.random_row(rng, int(n), "ACGT", 0.03) for n in rng.integers(1, 400, 40)] + [twin.low_complexity_row(rng, 300, "ACGT") for _ in range(10)]
    chars, offs = twin.pack(rows)
    tokens, lengths = bpe.bpe_tokenize_host(v, chars, offs, 400, "i")
    assert any(ord("N") in r for r in rows)
    for k, row in enumerate(rows):
        assert bpe.bpe_decode(v, tokens[k, :lengths[k]]) == hf.encode(bytes(row).decode()).tokens, k
