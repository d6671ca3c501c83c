"""tests/decode_twin.py pinned before it judges kernels (tests/test_validate_gate_gpu.py, tests/test_decode_edges_gpu.py): `decode`
against the committed reference fixture and against the host `Tokenizer.decode_tokens` on the ids no fixture holds (negative ones, ids
past 32 bits -- tokenize.h:107-124 loads unsigned, narrows to uint32 and looks the value up as int32), `validate` against the host
`bsq_validate_lengths`, `argmax` against numpy's on float64.  CPU only; every comparison is exact."""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest

import decode_twin as twin


@pytest.fixture(scope="module")
def decode_fixture(golden_dir):
    with gzip.open(os.path.join(golden_dir, "decode.json.gz")) as f:
        cases = json.load(f)
    return cases, np.load(os.path.join(golden_dir, "decode_tokens.npz"))


def bytes_table(alphabets_golden, key, flags):
    return twin.golden_bytes_table(alphabets_golden, key, flags)


def lut_of(alphabets_golden, key, flags):
    return twin.golden_table(alphabets_golden, key, flags)


def outcome(fn, *args):
    """("ok", result) or ("raise", type name, text)"""
    try:
        return ("ok", fn(*args))
    except Exception as e:  # noqa: BLE001 -- the outcome IS what is compared
        return ("raise", type(e).__name__, str(e))


def test_status_codes_are_the_librarys():
    from bioseq_amd import capi
    assert (twin.OK, twin.ERR_INVALID_ARG, twin.ERR_DTYPE, twin.ERR_SEQ_TOO_LONG) == \
        (capi.OK, capi.ERR_INVALID_ARG, capi.ERR_DTYPE, capi.ERR_SEQ_TOO_LONG)


def test_twin_decode_matches_reference_fixture(alphabets_golden, decode_fixture):
    cases, arrays = decode_fixture
    assert len(cases) == 7 * 8 * 5
    for c in cases:
        lut = lut_of(alphabets_golden, c["key"], "%d%d%d" % (c["eos"], c["bos"], c["padchar"]))
        toks = arrays[c["name"]]
        for dt in ("int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64"):
            if toks.max() <= np.iinfo(dt).max:
                assert twin.decode(lut, toks.astype(dt)) == c["decoded"], (c["name"], dt)
        assert [twin.decode(lut, toks[r]) for r in range(toks.shape[0])] == c["decoded"]
        assert twin.decode(lut, toks.astype(np.int16).T) == c["transposed"]
        assert twin.decode(lut, toks.astype(np.int32)[:, ::2]) == c["strided"]


def test_bytes_table_from_the_character_list(alphabets_golden):
    """`table_from_chars` restates tokenize.h:83-99; where the reference dumped its table as text, the two agree."""
    for key in ("DNA", "AMINO20", "SEB8"):
        for flags in ("000", "111", "010", "101"):
            m = alphabets_golden["meta"][key][flags]
            assert bytes_table(alphabets_golden, key, flags) == {k: v.encode("latin-1") for k, v in twin.table(m["lut"]).items()}, (key, flags)
    lut = bytes_table(alphabets_golden, "BYTES", "111")
    assert sorted(lut) == list(range(-128, 128)) + [256, 257, 258]
    assert lut[-1] == b"\xff" and lut[-128] == b"\x80" and lut[65] == b"A" and lut[257] == b"<EOS>"


@pytest.mark.parametrize("key,flags", [("DNA", "111"), ("DNA", "000"), ("AMINO20", "111"), ("SEB8", "010")])
def test_negative_and_wide_ids_twin_equals_host(bsq, alphabets_golden, key, flags):
    lut = lut_of(alphabets_golden, key, flags)
    assert lut["-1"] == "\x00"  # the reference's own dump: every character outside the alphabet maps to -1, NUL is the first
    tok = bsq.Tokenizer(key, int(flags[0]), int(flags[1]), int(flags[2]))
    top = max(int(k) for k in lut)
    rng = np.random.default_rng(11)
    base = rng.integers(0, top + 1, size=(9, 14))
    i32 = base.astype(np.int32)
    i32[0, 0] = i32[3, 13] = i32[8, 5] = -1
    i64 = base.astype(np.int64)
    i64[0, 1] = -1
    i64[2, 2] = 2 ** 32 + 1          # narrows to 1
    i64[4, 0] = 2 ** 32 - 1          # narrows to 0xFFFFFFFF, looked up as -1
    i64[8, 13] = 2 ** 32 + top
    i64[5, 5] = -(2 ** 32) + 1       # low 32 bits: 1
    for a in (i32, i64, i32.T, i64.T, i32[:, ::3], i64[::2], i32[0], i64[4], i64.view(np.uint64)):
        want = twin.decode(lut, a)
        assert tok.decode_tokens(a) == want
    assert twin.decode(lut, i32[0, :1]) == twin.decode(lut, i64[4, :1]) == "\x00"
    assert twin.decode(lut, i64[2, 2:3]) == twin.decode(lut, i64[5, 5:6]) == lut["1"]


@pytest.mark.parametrize("dtype,value,text", [
    ("int8", -1, 255), ("int16", -1, 65535), ("int32", 2 ** 31 - 1, 2 ** 31 - 1), ("int32", -2 ** 31, 2 ** 31),
    ("int32", -5, 4294967291), ("int64", -5, 4294967291), ("int64", 2 ** 32 + 99, 99), ("int64", 2 ** 31 - 1, 2 ** 31 - 1),
    ("int64", -2 ** 31, 2 ** 31), ("uint8", 200, 200), ("int16", 640, 640), ("int16", -129, 65407), ("int32", -129, 4294967167)])
def test_invalid_ids_twin_and_host_agree_in_outcome_and_text(bsq, alphabets_golden, dtype, value, text):
    lut = lut_of(alphabets_golden, "DNA", "111")
    tok = bsq.Tokenizer("DNA", 1, 1, 1)
    a = np.zeros((3, 6), dtype=dtype)
    a[2, 0] = 99             # later in row-major order: not the one named
    a[1, 4] = value
    want = outcome(twin.decode, lut, a)
    assert want == ("raise", "RuntimeError", "Unexpected/invalid token %d" % text)
    assert outcome(tok.decode_tokens, a) == want
    assert outcome(tok.decode_tokens, a[1]) == outcome(twin.decode, lut, a[1]) == want
    # by the VIEW's row-major order: in the transpose (0, 2) = 99 comes before (4, 1)
    assert outcome(tok.decode_tokens, a.T) == outcome(twin.decode, lut, a.T) == ("raise", "RuntimeError", "Unexpected/invalid token 99")


def test_twin_validate_equals_host_length_rule():
    from bioseq_amd import capi
    lib = capi.load()
    rng = np.random.default_rng(5)
    n_bad = 0
    for trial in range(300):
        B = int(rng.integers(1, 40))
        P = int(rng.integers(1, 12))
        bos, eos = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        offs = np.concatenate([[0], np.cumsum(rng.integers(0, P + 2, size=B))]).astype(np.int64)
        bad = ctypes.c_int64(-7)
        st = lib.bsq_validate_lengths(offs.ctypes.data, B, P, bos, eos, ctypes.byref(bad))
        assert (st, bad.value) == twin.validate(offs, B, P - bos - eos, -1), (trial, offs, P, bos, eos)
        n_bad += st != capi.OK
    assert 20 < n_bad < 280
    # exactly `room` passes, one more does not; bos and eos take one each
    offs = np.array([0, 3, 8, 8], dtype=np.int64)
    assert twin.validate(offs, 3, 5, -1) == (twin.OK, -1) and twin.validate(offs, 3, 4, -1) == (twin.ERR_SEQ_TOO_LONG, 1)
    for bos, eos, want in ((0, 0, twin.OK), (1, 0, twin.ERR_SEQ_TOO_LONG), (0, 1, twin.ERR_SEQ_TOO_LONG), (1, 1, twin.ERR_SEQ_TOO_LONG)):
        bad = ctypes.c_int64(-7)
        assert lib.bsq_validate_lengths(offs.ctypes.data, 3, 5, bos, eos, ctypes.byref(bad)) == want == twin.validate(offs, 3, 5 - bos - eos, -1)[0]


def test_twin_validate_malformed_rules():
    """The rules of include/bsq.h that have no host entry point, on hand-made offsets."""
    v = twin.validate
    assert v([0, 5, 3, 6], 3, 10, 6) == (twin.ERR_INVALID_ARG, 1)
    assert v([0, 5, 3, 6], 3, 10, -1) == (twin.OK, -1)                     # not looked for without nchars
    assert v([0, 5, 3, 6], 3, 2, -1) == (twin.ERR_SEQ_TOO_LONG, 0)         # ... the length rule still holds
    assert v([0, 5, 3, 6], 3, 2, 6) == (twin.ERR_INVALID_ARG, 1)           # malformed wins over a too-long entry in front of it
    assert v([-1, 2, 3], 2, 10, 3) == (twin.ERR_INVALID_ARG, 0)
    assert v([0, 2, 3], 2, 10, 2) == (twin.ERR_INVALID_ARG, 2)
    assert v([0, 2, 3], 2, 10, 3) == (twin.OK, -1)
    assert v([0, 2, 1, 3], 3, 10, 2) == (twin.ERR_INVALID_ARG, 1)          # the smallest of the three kinds
    assert v([0, 0, 9, 4, 2], 4, 10, 100) == (twin.ERR_INVALID_ARG, 2)


def test_twin_argmax_equals_numpy_on_float64():
    rng = np.random.default_rng(9)
    for C in (1, 2, 23, 300):
        x = rng.standard_normal((500, C))
        x[rng.random(x.shape) < 0.05] = np.nan
        x[rng.random(x.shape) < 0.05] = np.inf
        x[rng.random(x.shape) < 0.05] = -np.inf
        x[rng.random(x.shape) < 0.05] = 0.0
        x[rng.random(x.shape) < 0.05] = -0.0
        x[7] = -np.inf
        x[8] = np.nan
        x[9] = 1.5
        assert twin.argmax(x).tolist() == np.argmax(x, axis=1).tolist()
    hand = np.array([[-0.0, 0.0, -1.0], [0.0, -0.0, -1.0], [np.nan, np.inf, 0.0], [1.0, 3.0, np.nan], [np.inf, 2.0, np.inf],
                     [1.0, 1.0 + 2.0 ** -40, 1.0], [1e300, 1e301, 1e301]])
    assert twin.argmax(hand).tolist() == [0, 0, 0, 2, 0, 1, 1] == np.argmax(hand, axis=1).tolist()
