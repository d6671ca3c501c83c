"""CPU: the edit distance of row pairs (include/bsq.h, "edit distance of row pairs") -- the declared symbols, the header's known
answers, the library's host twin bsq_edit_pairs_host against the plain dynamic programme of tests/edit_twin.py on generated pairs of
three alphabets, the symmetry of the two stores, the unmapped class, the codes -1 and -2, every refusal, and the integer identity rule
at its exact boundary.  No device is needed."""
import ctypes

import numpy as np
import pytest

import edit_twin as twin

LETTERS = {"DNA4": "ACGT", "DNA5": "ACGTN", "AMINO20": "ACDEFGHIKLMNPQRSTVWY"}
BATCH = [b"ACGTAC", b"ACGNACGT", b"AC", b"", b"TTTTTTT"]


def _tok(key):
    import bioseq_amd
    return bioseq_amd.Tokenizer(key, False, False, False)


def _lut(tok):
    from bioseq_amd import capi
    d = capi.desc_of(tok)
    return np.array(list(d.lut), np.int64), d.nchars


def _rows(rows):
    return twin.pack([np.frombuffer(r, np.uint8) for r in rows])


def test_new_symbols_are_declared_and_exported():
    import bioseq_amd.align as align
    from bioseq_amd import capi
    L = capi.load()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_edit_pairs_device", "bsq_edit_pairs_host", "bsq_edit_pairs_kernel_name"):
        assert n in names and hasattr(L, n), n
    assert L.bsq_abi_version() == 7 and ctypes.sizeof(capi.Edit) == 8
    for n in ("edit_distance_pairs", "edit_distance_host", "edit_kernel_name", "pair_lengths", "pair_identity", "verify_pairs", "verify_pairs_host"):
        assert n in align.__all__ and callable(getattr(align, n))
    assert (align.TOO_LONG, align.BAD_INDEX) == (-1, -2)


@pytest.mark.parametrize("key", ["DNA4", "DNA5", "AMINO20"])
def test_host_twin_equals_the_plain_dp(key):
    """Unrelated rows, mutated copies and shifted poly-A rows around the block edges; the related pairs are not vacuous."""
    from bioseq_amd import align
    tok = _tok(key)
    lut, nchars = _lut(tok)
    pairs = twin.cases(len(key) * 7 + 1, LETTERS[key])
    ca, oa, cb, ob, row, col = twin.store_of(pairs)
    exp = twin.edit_pairs(lut, nchars, ca, oa, cb, ob, row, col)
    got = align.edit_distance_host(tok, ca, oa, row, col, cb, ob)
    assert got.dtype == np.int32 and got.tobytes() == exp.tobytes()
    assert align.edit_distance_host(tok, cb, ob, col, row, ca, oa).tobytes() == exp.tobytes(), "the stores swapped"
    lengths = np.maximum(np.diff(oa), np.diff(ob))
    assert ((exp > 0) & (exp < lengths)).sum() > len(pairs) // 4 and (exp == lengths).any()
    for form in (1, 2, 3):  # (checked, and changes nothing on the host)
        assert align.edit_distance_host(tok, ca, oa, row, col, cb, ob, max_len=256, form=form).tobytes() == exp.tobytes()


def test_known_answers():
    """The answers of include/bsq.h from the numpy twin and from the host twin."""
    from bioseq_amd import align
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    chars, offs = _rows(BATCH)
    row, col = [a.ravel().astype(np.int64) for a in np.meshgrid(np.arange(5), np.arange(5), indexing="ij")]
    want = [0, 3, 4, 6, 6, 3, 0, 6, 8, 7, 4, 6, 0, 2, 7, 6, 8, 2, 0, 7, 6, 7, 7, 7, 0]
    assert twin.edit_pairs(lut, nchars, chars, offs, chars, offs, row, col).tolist() == want
    assert align.edit_distance_host(tok, chars, offs, row, col).tolist() == want
    c2, o2 = _rows([b"acgtNN-", b"ACGTnxA"])
    one = np.array([0], np.int64)
    assert twin.edit_pairs(lut, nchars, c2, o2, c2, o2, one, one + 1).tolist() == [1]
    assert align.edit_distance_host(tok, c2, o2, one, one + 1).tolist() == [1]
    r, c = np.array([0, 0, 5, 0], np.int64), np.array([1, 2, 0, -1], np.int64)
    assert twin.edit_pairs(lut, nchars, chars, offs, chars, offs, r, c, max_len=5).tolist() == [-1, 4, -2, -2]
    assert align.edit_distance_host(tok, chars, offs, r, c, max_len=5).tolist() == [-1, 4, -2, -2]
    r, c = np.array([0], np.int64), np.array([1], np.int64)
    assert align.verify_pairs_host(tok, chars, offs, r, c, min_identity=0.625)[0].tolist() == [True]
    assert align.verify_pairs_host(tok, chars, offs, r, c, min_identity=40961 / 65536)[0].tolist() == [False]
    assert twin.identity_threshold(0.625) == 40960


def test_unmapped_bytes_share_one_class():
    """N matches N and mismatches A in DNA4; '-' and bytes >= 0x80 are N's class; DNA5 maps N and keeps '-' apart from it."""
    from bioseq_amd import align
    chars, offs = _rows([b"ACNNGT", b"ACNNGT", b"ACANGT", b"AC-\xffGT", b"acnngt", b"\x80\x90\xa0"])
    row, col = np.array([0, 0, 0, 0, 5, 5], np.int64), np.array([1, 2, 3, 4, 5, 0], np.int64)
    for key, want in (("DNA4", [0, 1, 0, 0, 0, 4]), ("DNA5", [0, 1, 2, 0, 0, 6])):
        tok = _tok(key)
        lut, nchars = _lut(tok)
        assert twin.edit_pairs(lut, nchars, chars, offs, chars, offs, row, col).tolist() == want, key
        assert align.edit_distance_host(tok, chars, offs, row, col).tolist() == want, key


def test_codes_and_refusals():
    from bioseq_amd import align, capi
    tok = _tok("DNA4")
    rng = np.random.default_rng(5)
    rows = [twin.random_row(rng, n, "ACGT") for n in (100, 101, 102, 300, 4096, 4097, 5000)]
    chars, offs = twin.pack(rows)
    lut, nchars = _lut(tok)
    row = np.array([0, 1, 2, 1, 3, 2, -1, 0, 7, 1 << 40, 0], np.int64)
    col = np.array([3, 3, 3, 1, 3, 0, 0, 7, 7, 0, -(1 << 40)], np.int64)
    exp = twin.edit_pairs(lut, nchars, chars, offs, chars, offs, row, col, max_len=100)
    assert exp[:6].tolist()[1:5] == [-1, -1, -1, -1] and exp[0] > 0 and exp[5] > 0 and exp[6:].tolist() == [-2] * 5
    assert align.edit_distance_host(tok, chars, offs, row, col, max_len=100).tobytes() == exp.tobytes()
    row, col = np.array([4, 5, 5, 6, 4], np.int64), np.array([5, 6, 0, 4, 4], np.int64)
    exp = twin.edit_pairs(lut, nchars, chars, offs, chars, offs, row, col)
    assert exp[1] == -1 and (exp[[0, 2, 3]] > 0).all() and exp[4] == 0
    assert align.edit_distance_host(tok, chars, offs, row, col).tobytes() == exp.tobytes()
    empty = np.zeros(0, np.int64)
    assert align.edit_distance_host(tok, chars, offs, empty, empty).shape == (0,)
    assert align.edit_distance_host(tok, np.zeros(0, np.uint8), np.zeros(1, np.int64), row[:2], col[:2]).tolist() == [-2, -2]  # a store without rows
    for kw in ({"max_len": 0}, {"max_len": 4097}, {"max_len": 2.5}, {"max_len": 257, "form": 1}, {"max_len": 1025, "form": 2}, {"form": 4},
               {"form": -1}, {"form": True}):
        with pytest.raises(ValueError):
            align.edit_distance_host(tok, chars, offs, row, col, **kw)
    with pytest.raises(ValueError):
        align.edit_distance_host(_tok("BYTES"), chars, offs, row, col)
    with pytest.raises(ValueError):
        align.edit_distance_host(tok, chars, offs, row.astype(np.int32), col)
    with pytest.raises(ValueError):
        align.edit_distance_host(tok, chars, offs, row, col[:2])
    with pytest.raises(ValueError):
        align.edit_distance_host(tok, chars, offs, row, col, chars_b=chars)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            align.verify_pairs_host(tok, chars, offs, row, col, min_identity=bad)
    assert [align.edit_kernel_name(m) for m in (1, 256, 257, 1024, 1025, 4096)] == ["k_edit_pairs<4>"] * 2 + ["k_edit_pairs<16>"] * 2 + ["k_edit_pairs<64>"] * 2
    assert align.edit_kernel_name(100, 3) == "k_edit_pairs<64>" and align.edit_kernel_name(257, 1) == "" and align.edit_kernel_name(4097) == ""
    # the C ABI itself: a refusal writes nothing and leaves a reason
    L = capi.load()
    desc = capi.desc_of(tok)
    dist = np.full(5, 7, np.int32)
    for e in (capi.Edit(0, 0), capi.Edit(4097, 0), capi.Edit(257, 1), capi.Edit(100, 4), capi.Edit(100, -1)):
        st = L.bsq_edit_pairs_host(ctypes.byref(desc), chars.ctypes.data, offs.ctypes.data, 7, chars.ctypes.data, offs.ctypes.data, 7, row.ctypes.data,
                                   col.ctypes.data, 5, ctypes.byref(e), dist.ctypes.data)
        assert st == capi.ERR_INVALID_ARG and L.bsq_last_error() and (dist == 7).all()
    for args in ((None, offs.ctypes.data, 7, row.ctypes.data, 5), (chars.ctypes.data, offs.ctypes.data, -1, row.ctypes.data, 5),
                 (chars.ctypes.data, offs.ctypes.data, 7, None, 5), (chars.ctypes.data, offs.ctypes.data, 7, row.ctypes.data, -1)):
        st = L.bsq_edit_pairs_host(ctypes.byref(desc), args[0], args[1], args[2], chars.ctypes.data, offs.ctypes.data, 7, args[3], col.ctypes.data, args[4],
                                   None, dist.ctypes.data)
        assert st == capi.ERR_INVALID_ARG and (dist == 7).all()
    assert L.bsq_edit_pairs_host(ctypes.byref(desc), None, None, 0, None, None, 0, None, None, 0, None, None) == capi.OK  # nothing to do
    # a null bsq_edit is {4096, 0}
    assert L.bsq_edit_pairs_host(ctypes.byref(desc), chars.ctypes.data, offs.ctypes.data, 7, chars.ctypes.data, offs.ctypes.data, 7, row.ctypes.data,
                                 col.ctypes.data, 5, None, dist.ctypes.data) == capi.OK and dist.tobytes() == exp.tobytes()


def test_identity_rule_at_its_exact_boundary():
    """L = 128, T = 0.75 * 65536: dist * 65536 == (65536 - T) * L at dist 32, which passes; 33 fails.  Substitutions at every fourth
    character of a row without repeats nearby give exactly those distances."""
    from bioseq_amd import align
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    base = np.frombuffer(b"ACGT" * 32, np.uint8)

    def edited(k):  # k substitutions, 'A' -> 'T' at positions 0, 4, 8, ...
        x = base.copy()
        x[0:4 * k:4] = ord("T")
        return x

    rows = [base, edited(32), edited(31), np.concatenate([edited(32)[:-1], [ord("A")]]), np.zeros(0, np.uint8), np.zeros(0, np.uint8)]
    chars, offs = twin.pack(rows)
    row, col = np.array([0, 0, 0, 4, 0, 9], np.int64), np.array([1, 2, 3, 5, 4, 0], np.int64)
    dist = twin.edit_pairs(lut, nchars, chars, offs, chars, offs, row, col)
    assert dist.tolist() == [32, 31, 33, 0, 128, -2]
    T = twin.identity_threshold(0.75)
    assert 32 * 65536 == (65536 - T) * 128
    keep, got = align.verify_pairs_host(tok, chars, offs, row, col, min_identity=0.75)
    assert got.tobytes() == dist.tobytes() and keep.dtype == np.bool_
    assert keep.tolist() == [True, True, False, True, False, False]
    la, lb = np.diff(offs)[np.clip(row, 0, 5)], np.diff(offs)[col]
    assert keep[:5].tolist() == twin.passes(dist[:5], la[:5], lb[:5], 0.75).tolist()
    assert align.verify_pairs_host(tok, chars, offs, row, col, min_identity=1.0)[0].tolist() == [False, False, False, True, False, False]
    assert align.verify_pairs_host(tok, chars, offs, row, col, min_identity=0.0)[0].tolist() == [True] * 5 + [False]
    assert align.verify_pairs_host(tok, chars, offs, row, col, min_identity=0.75, max_len=100)[0].tolist() == [False, False, False, True, False, False]
