"""CPU: MinHash sketches and their comparison (include/bsq.h, "MinHash sketch") -- the declared symbols, the header's known answers, the
library's host twins bsq_minhash_host / bsq_sketch_compare_host against the numpy twin (tests/minhash_twin.py) byte for byte, every
refusal with `out` left untouched, the exact properties of the rule (strand invariance, mergeability, empty rows, Jaccard 1 and 0), and
the new host unit once under ASan / UBSan as a stand-alone program.  No device is needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import minhash_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, U64 = 2, 3
E = 4294967295
# (about 4 % unmapped bytes -- N, lower case, * and \xff: at k = 32 a quarter of the windows is still whole)
POOLS = {
    "DNA4": b"ACGT" * 25 + b"Na*\xff",
    "DNA5": b"ACGTN" * 20 + b"ag*\xff",
    "AMINO20": b"ACDEFGHIKLMNPQRSTVWY" * 5 + b"XBZ*a",
    "PURPYR": b"ACGTRY" * 12 + b"*N\xc1",
}
ALPHABET_CASES = [("DNA4", k) for k in (1, 3, 16, 17, 21, 31, 32)] + [("DNA5", 27)] + [("AMINO20", k) for k in (1, 7, 14)] + [("PURPYR", 32)]


def _lib():
    from bioseq_amd import capi
    return capi, capi.load()


def _lut(key):
    capi, L = _lib()
    lut = (ctypes.c_int8 * 256)()
    n = ctypes.c_int32(0)
    assert L.bsq_lut_get(key.encode(), lut, ctypes.byref(n)) == capi.OK
    return np.array(lut, dtype=np.int8), n.value


def _tok(key):
    import bioseq_amd
    return bioseq_amd.Tokenizer(key, False, False, False)


def _batch(rng, key, lens):
    lens = np.asarray(lens, dtype=np.int64)
    chars = rng.choice(np.frombuffer(POOLS[key], np.uint8), int(lens.sum())).astype(np.uint8)
    offs = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return chars, offs


def _packed(rows):
    chars = np.frombuffer(b"".join(rows), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return chars, offs


def test_new_symbols_are_declared_and_exported():
    import bioseq_amd
    capi, L = _lib()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_minhash_device", "bsq_minhash_host", "bsq_minhash_kernel_name", "bsq_sketch_compare_device", "bsq_sketch_compare_host"):
        assert n in names and hasattr(L, n), n
    assert L.bsq_abi_version() == 7
    assert "sketch" in bioseq_amd.__all__ and bioseq_amd.sketch.EMPTY == -1
    for n in ("minhash_packed", "minhash_host", "minhash_kernel_name", "sketch_compare", "sketch_compare_host", "sketch_jaccard"):
        assert n in bioseq_amd.sketch.__all__ and callable(getattr(bioseq_amd.sketch, n))
    assert ctypes.sizeof(capi.MinHash) == 40


def test_known_answers():
    """The answers of include/bsq.h, from the numpy twin and from the library's host twin."""
    from bioseq_amd import sketch
    assert twin.salt(0) == 0x680def4ba05b88ed
    lut, A = _lut("DNA4")
    chars, offs = _packed([b"ACGTAC", b"ACGNACGT", b"AC", b"", b"TTTTTTT"])
    want = {False: [[1282424135, 2136608625, E, E], [1282424135, 2136608625, E, E], [E] * 4, [E] * 4, [E, E, 1516739009, E]],
            True: [[1955840499, 2136608625, E, E], [E, 2136608625, E, E], [E] * 4, [E] * 4, [773537092, E, E, E]]}
    for canonical in (False, True):
        exp = np.array(want[canonical], dtype=np.uint32)
        assert np.array_equal(twin.sketch(lut, A, chars, offs, 3, 4, I32, canonical).view(np.uint32), exp)
        got = sketch.minhash_host(_tok("DNA4"), chars, offs, 3, 4, "i", canonical=canonical)
        assert got.dtype == np.int32 and np.array_equal(got.view(np.uint32), exp)
        got = sketch.minhash_host(_tok("DNA4"), chars, offs, 3, 4, "q", canonical=canonical)
        assert got.dtype == np.uint64 and np.array_equal(got.view(np.int64), np.where(exp == E, -1, exp.astype(np.int64)))
    chars, offs = _packed([b"ACGTACGTACGTACGTACGTACGTACGTACGTA"])
    assert twin.sketch(lut, A, chars, offs, 31, 2, U64, False, 1).tolist() == [[1033262189, 1590760883]]
    assert sketch.minhash_host(_tok("DNA4"), chars, offs, 31, 2, "q", seed=1).tolist() == [[1033262189, 1590760883]]


@pytest.mark.parametrize("key, k", ALPHABET_CASES)
def test_host_twin_equals_numpy_twin(key, k):
    from bioseq_amd import sketch
    lut, A = _lut(key)
    rng = np.random.default_rng(k * 100 + A)
    lens = rng.integers(0, 300, 40)
    lens[:6] = (0, k - 1, k, k + 1, 1500, 2 * k)
    chars, offs = _batch(rng, key, lens)
    for S in (1, 7, 64, 1024):
        for dc, code in (("i", I32), ("q", U64)):
            exp = twin.sketch(lut, A, chars, offs, k, S, code)
            got = sketch.minhash_host(_tok(key), chars, offs, k, S, dc)
            assert got.dtype == exp.dtype and got.tobytes() == exp.tobytes(), (key, k, S, dc)
    if key == "DNA4":
        for seed in (0, 5):
            exp = twin.sketch(lut, A, chars, offs, k, 64, I32, True, seed)
            assert sketch.minhash_host(_tok(key), chars, offs, k, 64, "i", canonical=True, seed=seed).tobytes() == exp.tobytes(), (k, seed)
        filled = (twin.sketch(lut, A, chars, offs, k, 64, I32)[4] != -1).sum()
        assert filled > 30 if k >= 16 else filled >= 3  # (the long row fills most buckets, or one per word: the comparison is not vacuous)


@pytest.mark.parametrize("seed", [0, 1, 2 ** 64 - 1])
def test_seeds(seed):
    from bioseq_amd import sketch
    lut, A = _lut("DNA4")
    chars, offs = _batch(np.random.default_rng(3), "DNA4", [200, 0, 37, 1000])
    exp = twin.sketch(lut, A, chars, offs, 21, 128, U64, True, seed)
    got = sketch.minhash_host(_tok("DNA4"), chars, offs, 21, 128, "q", canonical=True, seed=seed)
    assert got.tobytes() == exp.tobytes()
    other = sketch.minhash_host(_tok("DNA4"), chars, offs, 21, 128, "q", canonical=True, seed=(seed + 1) % 2 ** 64)
    assert not np.array_equal(got[3], other[3])  # another seed is another hash family


def test_refusals_leave_out_untouched():
    capi, L = _lib()
    chars, offs = _packed([b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT", b"ACGT"])
    descs = {key: capi.make_desc(key) for key in ("DNA4", "DNA5", "AMINO20")}
    out = np.full(2 * (2 ** 14 + 1) * 8, 0x5A, np.uint8)
    cases = [("DNA4", dict(k=0), I32), ("DNA4", dict(k=33), I32), ("DNA4", dict(k=-1), I32), ("DNA5", dict(k=28), I32), ("AMINO20", dict(k=15), I32),
             ("AMINO20", dict(k=32), I32), ("DNA4", dict(buckets=0), I32), ("DNA4", dict(buckets=2 ** 14 + 1), I32),
             ("AMINO20", dict(k=3, canonical=1), I32), ("DNA5", dict(k=3, canonical=1), I32), ("DNA4", dict(canonical=2), I32),
             ("DNA4", dict(), 0), ("DNA4", dict(), 1), ("DNA4", dict(), 4), ("DNA4", dict(), 5), ("DNA4", dict(), 6), ("DNA4", dict(), -1),
             ("DNA4", dict(reserved=1), I32), ("DNA4", dict(form=3), I32), ("DNA4", dict(form=-1), I32), ("DNA4", dict(form=1, buckets=1025), I32),
             ("DNA4", dict(total_chars=-1), I32)]
    for key, change, dt in cases:
        f = dict(k=3, buckets=16, canonical=0, form=0, seed=0, total_chars=0, reserved=0)
        f.update(change)
        m = capi.MinHash(f["k"], f["buckets"], f["canonical"], f["form"], f["seed"], f["total_chars"], f["reserved"])
        st = L.bsq_minhash_host(ctypes.byref(descs[key]), chars.ctypes.data, offs.ctypes.data, 2, ctypes.byref(m), dt, out.ctypes.data)
        assert st == (capi.ERR_DTYPE if dt != I32 else capi.ERR_INVALID_ARG), (key, change, dt)
        assert L.bsq_last_error() != b"" and (out == 0x5A).all(), (key, change, dt)
        assert L.bsq_minhash_kernel_name(ctypes.byref(descs[key]), ctypes.byref(m), 2, dt) == b""
        # the device entry point refuses before it touches a device: the same status without one
        assert L.bsq_minhash_device(ctypes.byref(descs[key]), chars.ctypes.data, offs.ctypes.data, 2, ctypes.byref(m), dt, out.ctypes.data, None) == st
    ok = capi.MinHash(3, 16, 0, 0, 0, 0, 0)
    d = descs["DNA4"]
    for args in ((None, offs.ctypes.data, out.ctypes.data), (chars.ctypes.data, None, out.ctypes.data), (chars.ctypes.data, offs.ctypes.data, None)):
        assert L.bsq_minhash_host(ctypes.byref(d), args[0], args[1], 2, ctypes.byref(ok), I32, args[2]) == capi.ERR_INVALID_ARG
    assert L.bsq_minhash_host(ctypes.byref(d), chars.ctypes.data, offs.ctypes.data, -1, ctypes.byref(ok), I32, out.ctypes.data) == capi.ERR_INVALID_ARG
    assert L.bsq_minhash_host(None, chars.ctypes.data, offs.ctypes.data, 2, ctypes.byref(ok), I32, out.ctypes.data) == capi.ERR_INVALID_ARG
    assert L.bsq_minhash_host(ctypes.byref(d), chars.ctypes.data, offs.ctypes.data, 2, None, I32, out.ctypes.data) == capi.ERR_INVALID_ARG
    assert L.bsq_minhash_host(ctypes.byref(d), None, None, 0, ctypes.byref(ok), I32, None) == capi.OK  # B == 0: nothing to do
    assert (out == 0x5A).all()
    # the top of the range is accepted: A^k = 2^64 exactly, and the largest k of the other alphabets
    for key, k in (("DNA4", 32), ("DNA5", 27), ("AMINO20", 14)):
        m = capi.MinHash(k, 16, 0, 0, 0, 0, 0)
        assert L.bsq_minhash_kernel_name(ctypes.byref(descs[key]), ctypes.byref(m), 2, I32) == b"k_minhash_wave"
    # the comparison's rules
    a = np.zeros((2, 4), np.int32)
    mm = np.full((2, 2), 0x5A5A5A5A, np.int32)
    for Ba, Bb, S, dt, pa, pm in ((-1, 2, 4, I32, a, mm), (2, -1, 4, I32, a, mm), (2, 2, 0, I32, a, mm), (2, 2, 2 ** 14 + 1, I32, a, mm), (2, 2, 4, 4, a, mm),
                                  (2, 2, 4, 0, a, mm), (2, 2, 4, I32, None, mm), (2, 2, 4, I32, a, None)):
        st = L.bsq_sketch_compare_host(pa.ctypes.data if pa is not None else None, Ba, a.ctypes.data, Bb, S, dt,
                                       pm.ctypes.data if pm is not None else None, None)
        assert st == (capi.ERR_DTYPE if dt != I32 else capi.ERR_INVALID_ARG) and (mm == 0x5A5A5A5A).all(), (Ba, Bb, S, dt)
    assert L.bsq_sketch_compare_host(None, 0, a.ctypes.data, 2, 4, I32, None, None) == capi.OK


def test_python_refusals_are_value_errors():
    from bioseq_amd import sketch
    chars, offs = _packed([b"ACGTACGTACGT"])
    dna, amino, dna5 = _tok("DNA4"), _tok("AMINO20"), _tok("DNA5")
    for call in (lambda: sketch.minhash_host(dna, chars, offs, 0), lambda: sketch.minhash_host(dna, chars, offs, 33),
                 lambda: sketch.minhash_host(dna5, chars, offs, 28), lambda: sketch.minhash_host(amino, chars, offs, 15),
                 lambda: sketch.minhash_host(dna, chars, offs, 3, 0), lambda: sketch.minhash_host(dna, chars, offs, 3, 2 ** 14 + 1),
                 lambda: sketch.minhash_host(amino, chars, offs, 3, canonical=True), lambda: sketch.minhash_host(dna, chars, offs, 3, 16, "f"),
                 lambda: sketch.minhash_host(dna, chars, offs, 3, 16, "b"), lambda: sketch.minhash_host(dna, chars, offs, 3, 16, "?"),
                 lambda: sketch.minhash_kernel_name(dna, 3, 5, 2048, form=1), lambda: sketch.minhash_kernel_name(dna, 3, 5, form=3),
                 lambda: sketch.minhash_packed(dna, chars, offs, 3),  # host arrays
                 lambda: sketch.sketch_compare(np.zeros((2, 4), np.int32)),
                 lambda: sketch.sketch_compare_host(np.zeros((2, 4), np.int32), np.zeros((2, 5), np.int32)),
                 lambda: sketch.sketch_compare_host(np.zeros((2, 4), np.int32), np.zeros((2, 4), np.int64)),
                 lambda: sketch.sketch_compare_host(np.zeros((2, 4), np.float32)), lambda: sketch.sketch_compare_host(np.zeros(4, np.int32))):
        with pytest.raises(ValueError):
            call()


def test_kernel_name_follows_the_predicate():
    from bioseq_amd import sketch
    tok = _tok("DNA4")
    name = sketch.minhash_kernel_name
    wave, block = "k_minhash_wave", "k_minhash_block<%d>"
    assert name(tok, 21, 41, 1024) == wave and name(tok, 21, 41, 1) == wave and name(tok, 21, 41, 1024, form=2) == block % 1024
    assert name(tok, 21, 41, 1025) == block % 4096 and name(tok, 21, 41, 4096) == block % 4096 and name(tok, 21, 41, 4097) == block % 16384
    assert name(tok, 21, 41, 16384, "q", canonical=True) == block % 16384 and name(tok, 21, 41, 64, form=2) == block % 1024
    assert name(tok, 21, 41, 128, total_chars=41 * 2047) == wave and name(tok, 21, 41, 128, total_chars=41 * 2048) == block % 1024
    assert name(tok, 21, 4096, 128, total_chars=4096 * 4095) == wave and name(tok, 21, 4096, 128, total_chars=4096 * 4096) == block % 1024
    assert name(tok, 21, 4095, 128, total_chars=4095 * 2048) == block % 1024  # (fewer than 4096 rows: from 2048 characters on)
    assert name(tok, 21, 41, 128, total_chars=41 * 2048, form=1) == wave and name(tok, 21, 0, 128) == wave


def test_exact_properties():
    from bioseq_amd import sketch
    tok = _tok("DNA4")
    rng = np.random.default_rng(17)
    rows = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in (0, 20, 21, 300, 5000)]
    rows.append(b"ACGT" * 30 + b"N" + b"TTGCA" * 40)
    for k in (4, 21, 32):
        # a row and its reverse complement have equal canonical sketches
        chars, offs = _packed(rows)
        rc_chars, rc_offs = _packed([bytes(twin.revcomp(np.frombuffer(r, np.uint8))) for r in rows])
        fwd = sketch.minhash_host(tok, chars, offs, k, 256, "i", canonical=True, seed=9)
        assert np.array_equal(fwd, sketch.minhash_host(tok, rc_chars, rc_offs, k, 256, "i", canonical=True, seed=9)), k
        assert (fwd[4] != -1).sum() > (200 if k > 4 else 50)  # (k = 4 has 136 canonical words, many their own reverse complement)
        # mergeability: the pieces [0, 2000 + k - 1) and [2000, end) of the long row overlap by k - 1 characters and cover every window once
        long_row = rows[4]
        pieces = sketch.minhash_host(tok, *_packed([long_row[:2000 + k - 1], long_row[2000:]]), k, 256, "i", canonical=True, seed=9)
        assert np.array_equal(twin.merge(pieces[0].view(np.uint32), pieces[1].view(np.uint32)), fwd[4].view(np.uint32)), k
        three = sketch.minhash_host(tok, *_packed([long_row[:100 + k - 1], long_row[100:4000 + k - 1], long_row[4000:]]), k, 256, "q", seed=9)
        whole = sketch.minhash_host(tok, *_packed([long_row]), k, 256, "q", seed=9)
        assert three.dtype == np.uint64  # (EMPTY is all bits set: the unsigned minimum of the elements is the merge)
        assert np.array_equal(twin.merge(twin.merge(three[0], three[1]), three[2]), whole[0]), k
    # an all-N row is all EMPTY, in both types
    chars, offs = _packed([b"N" * 500, b"", b"nnnn\xff*"])
    assert (sketch.minhash_host(tok, chars, offs, 5, 64, "i") == -1).all()
    assert (sketch.minhash_host(tok, chars, offs, 5, 64, "q").view(np.int64) == -1).all()
    # identical rows: Jaccard 1; rows without a common k-mer: 0; empty against anything: 0 (either = the other's buckets, or 0)
    chars, offs = _packed([rows[3], rows[3], b"A" * 300, b"C" * 300, b"NNNN", b""])
    sk = sketch.minhash_host(tok, chars, offs, 21, 128, "i")
    jac = sketch.sketch_jaccard(sk)
    assert jac.dtype == np.float32 and jac.shape == (6, 6)
    assert jac[0, 1] == 1.0 and jac[0, 0] == 1.0 and jac[2, 2] == 1.0 and jac[3, 3] == 1.0
    assert jac[2, 3] == 0.0 and jac[0, 2] == 0.0 and jac[4, 4] == 0.0 and jac[4, 5] == 0.0 and jac[0, 4] == 0.0
    match, either = sketch.sketch_compare_host(sk)
    assert match[2, 2] == 1 and either[2, 3] == 2 and either[4, 5] == 0 and either[0, 4] == (sk[0] != -1).sum()
    # near-duplicates: a row with 2 % substitutions stays close to its source, an unrelated row does not
    base = np.frombuffer(rows[4], np.uint8).copy()
    edited = base.copy()
    at = rng.choice(base.size, 20, replace=False)
    edited[at] = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), base[at]) + 1) % 4]
    other = rng.choice(np.frombuffer(b"ACGT", np.uint8), 5000).astype(np.uint8)
    sk = sketch.minhash_host(tok, *_packed([base.tobytes(), edited.tobytes(), other.tobytes()]), 11, 1024, "q", canonical=True)
    jac = sketch.sketch_jaccard(sk)
    assert 0.4 < jac[0, 1] < 1.0 and jac[0, 2] < 0.05  # 20 edits destroy at most 220 of 4990 windows: J >= 0.91 in expectation


COMPARE_CASES = [(1, 1, 1), (3, 5, 7), (65, 130, 100)]
VALUES = np.array([E, 0, 1, 2, 3, 4, 5, 2 ** 31, 2 ** 32 - 2], dtype=np.uint64)


def _sketch_like(rng, B, S, dtype):
    """values drawn from {EMPTY, 0 .. 5, 2^31, 2^32 - 2} as the element type stores them"""
    v = VALUES[rng.integers(0, VALUES.size, (B, S))]
    if dtype == np.int32:
        return v.astype(np.uint32).view(np.int32)
    out = v.copy()
    out[v == E] = np.uint64(2 ** 64 - 1)
    return out if dtype == np.uint64 else out.view(np.int64)


@pytest.mark.parametrize("Ba, Bb, S", COMPARE_CASES)
@pytest.mark.parametrize("dtype", [np.int32, np.uint64, np.int64])
def test_compare_host_equals_numpy_broadcast(Ba, Bb, S, dtype):
    from bioseq_amd import sketch
    rng = np.random.default_rng(Ba * 1000 + S)
    a, b = _sketch_like(rng, Ba, S, dtype), _sketch_like(rng, Bb, S, dtype)
    exp_m, exp_e = twin.compare(a, b)
    got_m, got_e = sketch.sketch_compare_host(a, b)
    assert got_m.dtype == np.int32 and got_m.shape == (Ba, Bb) and np.array_equal(got_m, exp_m) and np.array_equal(got_e, exp_e)
    assert exp_m.sum() > 0 or S == 1
    only_m, none = sketch.sketch_compare_host(a, b, either=False)
    assert none is None and np.array_equal(only_m, exp_m)
    self_m, self_e = sketch.sketch_compare_host(a)  # a is b
    exp_m, exp_e = twin.compare(a, a)
    assert np.array_equal(self_m, exp_m) and np.array_equal(self_e, exp_e)
    assert np.array_equal(np.diag(self_m), (a.astype(np.uint64) & np.uint64(0xFFFFFFFF) != E).sum(-1))
    empty_m, empty_e = sketch.sketch_compare_host(a[:0], b)
    assert empty_m.shape == (0, Bb) and empty_e.shape == (0, Bb)


def test_host_unit_under_address_and_ub_sanitizers(tmp_path):
    """bsq_sketch_host.cpp with g++ -fsanitize=address,undefined in a stand-alone program (tests/native/sketch_host_check.cpp: its own
    main, its own plain-loop reference, exact-size heap arrays so that a read past a row's batch or a write past `out` is an error)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if not shutil.which("g++") or subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")],
                                                 capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link the ASan / UBSan runtimes here")
    exe = str(tmp_path / "sketch_host_check")
    csrc = os.path.join(ROOT, "bioseq_amd", "csrc")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        os.path.join(ROOT, "tests", "native", "sketch_host_check.cpp"), os.path.join(csrc, "bsq_sketch_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SKETCH_HOST_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-4000:]
