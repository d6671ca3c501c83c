"""CPU: the k-mer spectrum (include/bsq.h, "k-mer spectrum") -- the library's host twin bsq_kmer_spectrum_host against the numpy twin
(tests/kmer_spectrum_twin.py) byte for byte, the known answers of the specification, the refusals and the properties of the rule, and
the Python helpers of bioseq_amd.kmers.  No device is needed."""
import ctypes

import numpy as np
import pytest

import kmer_spectrum_twin as twin

SEQS = [b"ACGTAC", b"ACGNACGT", b"AC", b"", b"TTTTTTT"]
GUARD = 64
I8, I16, I32, U64, F32, F64 = range(6)
# (element type, normalize): the six accepted combinations
COMBOS = [(I32, 0), (U64, 0), (F32, 0), (F64, 0), (F32, 1), (F64, 1)]
POOLS = {
    "DNA4": b"ACGTACGTACGTACGTACGTNacgtn*\xff\x80",
    "DNA5": b"ACGTNACGTNACGTNacgtn*\xff\x80",
    "AMINO20": b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQRSTVWYXBZ*acd\xfe",
    "PURPYR": b"ACGTRYACGTRYacgt*N\xc1",
    "SEB8": b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQRSTVWYXBZ*\x90",
}


def _lib():
    from bioseq_amd import capi
    return capi, capi.load()


def _pack(seqs, lead=b""):
    chars = np.frombuffer(lead + b"".join(seqs), dtype=np.uint8).copy()
    offs = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=offs[1:])
    return chars, offs + len(lead)


def _lut(key):
    capi, L = _lib()
    lut = (ctypes.c_int8 * 256)()
    n = ctypes.c_int32(0)
    assert L.bsq_lut_get(key.encode(), lut, ctypes.byref(n)) == capi.OK
    return np.array(lut, dtype=np.int8), n.value


def _host(key, chars, offs, k, s, dt, both=0, normalize=0, form=0, B=None, first=0, V=None):
    """bsq_kmer_spectrum_host on rows [first, first + B) into a 0xAB-filled buffer with guards: (status, matrix, raw bytes)."""
    capi, L = _lib()
    d = capi.make_desc(key)
    km = capi.Kmer(k, s)
    o = capi.KmerSpectrum(both, normalize, form, 0, 0)
    B = len(offs) - 1 - first if B is None else B
    lut, A = _lut(key)
    V = A ** k if V is None else V
    np_t = twin.NP_DTYPES.get(dt, np.int32)
    nbytes = max(B, 0) * V * np.dtype(np_t).itemsize
    raw = np.full(nbytes + 2 * GUARD, 0xAB, dtype=np.uint8)
    st = L.bsq_kmer_spectrum_host(ctypes.byref(d), chars.ctypes.data, offs[first:].ctypes.data, B, ctypes.byref(km), ctypes.byref(o), dt,
                                  raw.ctypes.data + GUARD)
    assert (raw[:GUARD] == 0xAB).all() and (raw[GUARD + nbytes:] == 0xAB).all(), "a guard byte was overwritten"
    return st, raw[GUARD:GUARD + nbytes].view(np_t).reshape(max(B, 0), V), raw


def _sparse(m):
    return [{int(v): int(r[v]) for v in np.flatnonzero(r)} for r in m]


def test_new_symbols_are_declared_and_exported():
    capi, L = _lib()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_kmer_spectrum_width", "bsq_kmer_spectrum_device", "bsq_kmer_spectrum_host", "bsq_kmer_spectrum_kernel_name"):
        assert n in names and hasattr(L, n), n
    assert "typedef struct bsq_kmer_spectrum" in open(capi.HEADER_PATH).read()
    assert L.bsq_abi_version() == 7
    from bioseq_amd import kmers
    for n in ("kmer_spectrum_packed", "kmer_spectrum_host", "kmer_spectrum_width", "kmer_spectrum_kernel_name", "kmer_canonical_columns"):
        assert n in kmers.__all__ and callable(getattr(kmers, n)), n


KNOWN = [
    (2, 1, 0, [{1: 2, 6: 1, 11: 1, 12: 1}, {1: 2, 6: 2, 11: 1}, {1: 1}, {}, {15: 6}]),
    (2, 1, 1, [{1: 3, 6: 2, 11: 3, 12: 2}, {1: 3, 6: 4, 11: 3}, {1: 1, 11: 1}, {}, {0: 6, 15: 6}]),
    (3, 2, 0, [{6: 1, 44: 1}, {6: 2}, {}, {}, {63: 3}]),
]


@pytest.mark.parametrize("k, s, both, rows", KNOWN)
def test_known_answers_of_the_specification(k, s, both, rows):
    capi, _ = _lib()
    chars, offs = _pack(SEQS)
    lut, A = _lut("DNA4")
    for dt in (I32, U64, F32, F64):
        st, got, _ = _host("DNA4", chars, offs, k, s, dt, both=both)
        assert st == capi.OK
        assert _sparse(got) == rows, (dt, got)
    assert _sparse(twin.counts(lut, A, chars, offs, k, s, bool(both))) == rows
    # frequencies, bit for bit np.float32(c) / np.float32(S) (and the same in double); the empty rows stay zero
    want = np.zeros((5, 4 ** k), dtype=np.int64)
    for i, r in enumerate(rows):
        for v, c in r.items():
            want[i, v] = c
    for dt, T in ((F32, np.float32), (F64, np.float64)):
        st, got, _ = _host("DNA4", chars, offs, k, s, dt, both=both, normalize=1)
        assert st == capi.OK
        exp = np.zeros(want.shape, dtype=T)
        for i in range(5):
            S = want[i].sum()
            if S:
                exp[i] = want[i].astype(T) / T(S)
        assert got.tobytes() == exp.tobytes(), dt


def test_canonical_columns():
    import bioseq_amd
    from bioseq_amd import kmers
    tok = bioseq_amd.Tokenizer("DNA4", False, False, False)
    assert kmers.kmer_canonical_columns(tok, 2).tolist() == [0, 1, 2, 3, 4, 5, 6, 8, 9, 12]
    for k in range(1, 8):
        cols = kmers.kmer_canonical_columns(tok, k)
        assert cols.dtype == np.int64 and (np.diff(cols) > 0).all()
        assert cols.size == ((4 ** k + 4 ** (k // 2)) // 2 if k % 2 == 0 else 4 ** k // 2), k
        rc = twin.rc_ids(4 ** k, k)
        assert np.array_equal(cols, np.flatnonzero(np.arange(4 ** k) <= rc))
    assert kmers.kmer_canonical_columns(bioseq_amd.Tokenizer("DNA", False, False, False), 3).size == 32
    for key in ("DNA5", "AMINO20", "PURPYR"):
        with pytest.raises(ValueError):
            kmers.kmer_canonical_columns(bioseq_amd.Tokenizer(key, False, False, False), 2)


def _random_batch(rng, key, k):
    """Rows of length 0, k - 1, k, random ones up to 300; mostly mapped characters with unmapped bytes and bytes >= 0x80 among them."""
    pool = np.frombuffer(POOLS[key], dtype=np.uint8)
    lens = [0, k - 1, k, k + 1, 0] + [int(x) for x in rng.integers(0, 300, 20)]
    seqs = [bytes(rng.choice(pool, n).astype(np.uint8)) for n in lens]
    seqs.append(bytes(rng.choice(pool[:4], 200).astype(np.uint8)))  # a row without an unmapped character
    return _pack(seqs, lead=b"NNN")  # offsets do not start at zero


CASES = [("DNA4", 1), ("DNA4", 4), ("DNA4", 7), ("DNA5", 3), ("AMINO20", 2), ("AMINO20", 3), ("PURPYR", 1), ("SEB8", 4)]


@pytest.mark.parametrize("key, k", CASES)
def test_host_twin_equals_the_numpy_twin(key, k):
    capi, _ = _lib()
    lut, A = _lut(key)
    rng = np.random.default_rng(k * 7 + A)
    chars, offs = _random_batch(rng, key, k)
    assert (chars >= 0x80).any() and (lut[chars] < 0).any()
    for s in sorted({1, 2, k}):
        for both in ((0, 1) if key == "DNA4" else (0,)):
            c = twin.counts(lut, A, chars, offs, k, s, bool(both))
            # the counts of a row sum to its windows without an unmapped character, doubled with both strands
            n_ok = [twin.window_ids(lut, A, chars[offs[i]:offs[i + 1]], k, s).size for i in range(len(offs) - 1)]
            assert c.sum(axis=1).tolist() == [(1 + both) * n for n in n_ok]
            if both:
                assert np.array_equal(c, c[:, twin.rc_ids(A ** k, k)])
            for dt, norm in COMBOS:
                st, got, _ = _host(key, chars, offs, k, s, dt, both=both, normalize=norm)
                assert st == capi.OK
                exp = twin.spectrum(lut, A, chars, offs, k, s, dt, bool(both), bool(norm))
                assert got.tobytes() == exp.tobytes(), (key, k, s, both, dt, norm)
            # rows [a, b) of the batch give the slice [a, b) of the whole batch's spectrum
            st, part, _ = _host(key, chars, offs, k, s, I32, both=both, B=9, first=3)
            assert st == capi.OK and np.array_equal(part, c[3:12])


def test_python_host_twin_and_helpers():
    import bioseq_amd
    from bioseq_amd import kmers
    lut, A = _lut("DNA4")
    chars, offs = _random_batch(np.random.default_rng(3), "DNA4", 4)
    tok = bioseq_amd.Tokenizer("DNA4", True, True, True)  # BOS, EOS and PAD play no part
    for dc, dt in (("i", I32), ("q", U64), ("f", F32), ("d", F64)):
        got = kmers.kmer_spectrum_host(tok, chars, offs, 4, dc, stride=2, both_strands=True)
        assert got.shape == (len(offs) - 1, 256)
        assert got.tobytes() == twin.spectrum(lut, A, chars, offs, 4, 2, dt, True, False).tobytes()
    got = kmers.kmer_spectrum_host(tok, chars, offs, 4, normalize=True)
    assert got.dtype == np.float32 and got.tobytes() == twin.spectrum(lut, A, chars, offs, 4, 1, F32, False, True).tobytes()
    assert kmers.kmer_spectrum_host(tok, chars[:0], offs[:1], 4).shape == (0, 256)
    assert kmers.kmer_spectrum_width(tok, 7) == 16384
    amino = bioseq_amd.Tokenizer("AMINO20", False, False, False)
    assert kmers.kmer_spectrum_width(amino, 3) == 8000
    for bad in (lambda: kmers.kmer_spectrum_width(tok, 8), lambda: kmers.kmer_spectrum_width(amino, 4),
                lambda: kmers.kmer_spectrum_host(tok, chars, offs, 4, "b"), lambda: kmers.kmer_spectrum_host(tok, chars, offs, 4, "h"),
                lambda: kmers.kmer_spectrum_host(tok, chars, offs, 4, "i", normalize=True),
                lambda: kmers.kmer_spectrum_host(tok, chars, offs, 4, "?"),
                lambda: kmers.kmer_spectrum_host(amino, chars, offs, 2, both_strands=True),
                lambda: kmers.kmer_spectrum_host(tok, chars, offs, 4, stride=0),
                lambda: kmers.kmer_spectrum_kernel_name(tok, 6, 10, form=1), lambda: kmers.kmer_spectrum_kernel_name(tok, 4, 10, form=3)):
        with pytest.raises(ValueError):
            bad()
    # the choice of kernel: a pure predicate of (V, B, total_chars, form)
    name = kmers.kmer_spectrum_kernel_name
    assert name(tok, 4, 100) == "k_kmer_spectrum_wave" and name(tok, 5, 100, total_chars=100 * 2047) == "k_kmer_spectrum_wave"
    assert name(tok, 4, 100, total_chars=100 * 2048) == "k_kmer_spectrum_block<1024>" and name(tok, 4, 100, form=2) == "k_kmer_spectrum_block<1024>"
    assert name(tok, 4, 100, total_chars=100 * 2048, form=1) == "k_kmer_spectrum_wave"
    # (a batch of at least 4096 rows keeps the wave form up to a mean row of 16 384 characters)
    assert name(tok, 4, 4096, total_chars=4096 * 16383) == "k_kmer_spectrum_wave" and name(tok, 4, 4095, total_chars=4095 * 2048) == "k_kmer_spectrum_block<1024>"
    assert name(tok, 4, 4096, total_chars=4096 * 16384) == "k_kmer_spectrum_block<1024>"
    assert name(tok, 6, 100) == "k_kmer_spectrum_block<4096>" and name(amino, 3, 1, "d") == "k_kmer_spectrum_block<16384>"
    assert name(tok, 7, 0, "q", form=2) == "k_kmer_spectrum_block<16384>"


def test_refusals_leave_the_output_untouched():
    capi, L = _lib()
    chars, offs = _pack(SEQS)

    def refused(status, key="DNA4", k=2, s=1, dt=I32, V=16, **kw):
        st, _, raw = _host(key, chars, offs, k, s, dt, V=V, **kw)
        assert st == status and (raw == 0xAB).all() and L.bsq_last_error() != b"", (key, k, dt, kw)
        d, km = capi.make_desc(key), capi.Kmer(k, s)
        o = capi.KmerSpectrum(kw.get("both", 0), kw.get("normalize", 0), kw.get("form", 0), 0, 0)
        B = kw.get("B", 5)
        assert L.bsq_kmer_spectrum_kernel_name(ctypes.byref(d), ctypes.byref(km), ctypes.byref(o), B, dt) == b""

    refused(capi.ERR_INVALID_ARG, k=8)                       # V = 4^8
    refused(capi.ERR_INVALID_ARG, key="AMINO20", k=4)
    refused(capi.ERR_DTYPE, dt=I8)
    refused(capi.ERR_DTYPE, dt=I16)
    refused(capi.ERR_DTYPE, dt=7)
    refused(capi.ERR_DTYPE, dt=I32, normalize=1)
    refused(capi.ERR_DTYPE, dt=U64, normalize=1)
    for key in ("DNA5", "AMINO20", "PURPYR"):
        refused(capi.ERR_INVALID_ARG, key=key, both=1)
    refused(capi.ERR_INVALID_ARG, k=6, form=1, V=4096)       # the wave form cannot take V = 4096
    refused(capi.ERR_INVALID_ARG, form=3)
    refused(capi.ERR_INVALID_ARG, both=2)
    refused(capi.ERR_INVALID_ARG, k=0)
    refused(capi.ERR_INVALID_ARG, s=0)
    refused(capi.ERR_INVALID_ARG, B=-1)
    # null pointers
    d, km, o = capi.make_desc("DNA4"), capi.Kmer(2, 1), capi.KmerSpectrum(0, 0, 0, 0, 0)
    raw = np.full(5 * 16 * 4, 0xAB, dtype=np.uint8)
    cp, op, rp = chars.ctypes.data, offs.ctypes.data, raw.ctypes.data
    D, K, O = ctypes.byref(d), ctypes.byref(km), ctypes.byref(o)
    for args in ((None, cp, op, 5, K, O, I32, rp), (D, None, op, 5, K, O, I32, rp), (D, cp, None, 5, K, O, I32, rp),
                 (D, cp, op, 5, None, O, I32, rp), (D, cp, op, 5, K, None, I32, rp), (D, cp, op, 5, K, O, I32, None)):
        assert L.bsq_kmer_spectrum_host(*args) == capi.ERR_INVALID_ARG and (raw == 0xAB).all()
        assert L.bsq_kmer_spectrum_device(*args, None) == capi.ERR_INVALID_ARG  # refused before any device call
    assert L.bsq_kmer_spectrum_host(D, cp, op, 2 ** 31, K, O, I32, rp) == capi.ERR_INVALID_ARG and (raw == 0xAB).all()  # B beyond one launch's rows
    assert L.bsq_kmer_spectrum_device(D, cp, op, 2 ** 31, K, O, I32, rp, None) == capi.ERR_INVALID_ARG
    assert L.bsq_kmer_spectrum_width(None, K) == -capi.ERR_INVALID_ARG and L.bsq_kmer_spectrum_width(D, None) == -capi.ERR_INVALID_ARG
    assert L.bsq_kmer_spectrum_width(D, ctypes.byref(capi.Kmer(8, 1))) == -capi.ERR_INVALID_ARG
    assert L.bsq_kmer_spectrum_width(D, ctypes.byref(capi.Kmer(7, 3))) == 16384
    # B == 0: BSQ_OK, nothing written, null buffers allowed
    assert L.bsq_kmer_spectrum_host(D, None, None, 0, K, O, I32, None) == capi.OK
    assert L.bsq_kmer_spectrum_device(D, None, None, 0, K, O, I32, None, None) == capi.OK


def test_negative_lengths_count_as_empty_rows():
    capi, _ = _lib()
    chars, offs = _pack([b"ACGTACGT", b"ACGT", b"ACGTAC"])
    offs = offs.copy()
    offs[2] = offs[1] - 2  # row 1 has a negative length: it counts as empty
    st, got, _ = _host("DNA4", chars, offs, 2, 1, I32, B=2)
    assert st == capi.OK and got[1].sum() == 0 and got[0].sum() == 7
