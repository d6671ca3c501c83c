"""CPU: span-masked k-mer masked-LM batches (include/bsq.h, "k-mer masked-LM") -- the library's host twin bsq_kmer_mlm_tokenize_host
against the numpy twin (tests/kmer_mlm_twin.py) bit for bit, the known answers of the specification, the argument rules with their
statuses, the invariances of the draw, the coverage share and the span property, and the Python / loader argument rules.  No device."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import kmer_mlm_twin as twin
import kmer_twin

FLAGS = list(itertools.product((0, 1), repeat=3))  # (bos, eos, padchar)
GUARD = 64
SEQS = [b"ACGTAC", b"ACGNACGT", b"AC", b"", b"TTTTTTT"]


def _lib():
    from bioseq_amd import capi
    return capi, capi.load()


def _pack(seqs, lead=b"", tail=b""):
    chars = np.frombuffer(lead + b"".join(seqs) + tail, dtype=np.uint8).copy()
    offs = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=offs[1:])
    return chars, offs + len(lead)


def _lut(key):
    capi, L = _lib()
    lut = (ctypes.c_int8 * 256)()
    n = ctypes.c_int32(0)
    assert L.bsq_lut_get(key.encode(), lut, ctypes.byref(n)) == capi.OK
    return np.array(lut, dtype=np.int8), n.value


def _m(capi, anchor_prob=0.3, mask_prob=0.8, random_prob=0.1, span=3, mask_token=65, ignore_index=-100, seed=0, first_row=0):
    return capi.KmerMlm(anchor_prob, mask_prob, random_prob, span, mask_token, ignore_index, seed, first_row)


def _host(key, flags, chars, offs, k, s, P, m, it=3, lt=3, batch_first=True, B=None, first=0, want_in=True, want_lab=True):
    """bsq_kmer_mlm_tokenize_host on rows [first, first + B) into guarded buffers: (status, inputs, labels, guards intact)."""
    capi, L = _lib()
    bos, eos, pad = flags
    d = capi.make_desc(key, eos=eos, bos=bos, padchar=pad)
    km = capi.Kmer(k, s)
    B = len(offs) - 1 - first if B is None else B
    bufs, outs = [], []
    for t in (it, lt):
        np_t = twin.NP_DTYPES.get(t, np.uint64)
        nbytes = max(B, 0) * max(P, 0) * np.dtype(np_t).itemsize
        bufs.append((np.full(nbytes + 2 * GUARD, 0xAB, dtype=np.uint8), nbytes, np_t))
    st = L.bsq_kmer_mlm_tokenize_host(ctypes.byref(d), chars.ctypes.data, offs[first:].ctypes.data, B, P, int(batch_first), ctypes.byref(km),
                                      ctypes.byref(m), it, bufs[0][0].ctypes.data + GUARD if want_in else None, lt,
                                      bufs[1][0].ctypes.data + GUARD if want_lab else None)
    intact = True
    for raw, nbytes, np_t in bufs:
        intact &= bool((raw[:GUARD] == 0xAB).all() and (raw[GUARD + nbytes:] == 0xAB).all())
        outs.append(raw[GUARD:GUARD + nbytes].view(np_t).reshape((B, P) if batch_first else (P, B)) if B >= 0 and P > 0 else raw[:0])
    return st, outs[0], outs[1], intact


def _untouched(a):
    return bool((a.view(np.uint8) == 0xAB).all())


def test_new_symbols_are_declared_and_exported():
    capi, L = _lib()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_kmer_mlm_anchor_prob", "bsq_kmer_mlm_tokenize_device", "bsq_kmer_mlm_tokenize_host", "bsq_kmer_mlm_kernel_name"):
        assert n in names and hasattr(L, n), n
    assert "typedef struct bsq_kmer_mlm" in open(capi.HEADER_PATH).read()
    assert L.bsq_abi_version() == 7
    from bioseq_amd import kmers
    for n in ("kmer_mlm_tokenize_packed", "kmer_mlm_tokenize_host", "span_anchor_prob", "kmer_mlm_kernel_name"):
        assert n in kmers.__all__ and hasattr(kmers, n)


KNOWN = [  # (flags, anchor_prob, row of SEQS, inputs, labels) -- include/bsq.h, "-" = ignore_index
    ((0, 0, 0), 0.5, 0, "65 65 47 65 0 0 0 0", "6 27 44 49 - - - -"),
    ((0, 0, 0), 0.5, 1, "6 64 64 64 65 65 0 0", "- - - - 6 27 - -"),
    ((0, 0, 0), 0.5, 4, "65 38 63 63 65 0 0 0", "63 63 63 63 63 - - -"),
    ((1, 1, 1), 0.5, 0, "65 68 68 47 68 66 67 67", "- 6 27 44 49 - - -"),
    ((0, 0, 0), 0.3, 4, "63 38 63 63 63 0 0 0", "- 63 63 63 - - - -"),
]


@pytest.mark.parametrize("flags, ap, row, inputs, labels", KNOWN)
def test_known_answers_of_the_specification(flags, ap, row, inputs, labels):
    capi, _ = _lib()
    chars, offs = _pack(SEQS)
    lut, A = _lut("DNA4")
    vocab = kmer_twin.specials(A, 3, *flags)["vocab"]
    want_in = [int(x) for x in inputs.split()]
    want_lab = [-100 if x == "-" else int(x) for x in labels.split()]
    st, gi, gl, intact = _host("DNA4", flags, chars, offs, 3, 1, 8, _m(capi, ap, span=3, mask_token=vocab, seed=7))
    assert st == capi.OK and intact
    assert gi.view(np.int64)[row].tolist() == want_in and gl.view(np.int64)[row].tolist() == want_lab
    ti, tl = twin.mlm(lut, A, chars, offs, 3, 1, 8, *flags, anchor_prob=ap, span=3, seed=7)
    assert ti[row].tolist() == want_in and tl[row].tolist() == want_lab


def _case_batch(rng, lut, k, s, room):
    """Lengths 0, k - 1, k, exactly filling `room` windows, over-long (clamped), random ones; runs of unmapped characters."""
    mapped = np.flatnonzero(lut >= 0).astype(np.uint8)
    unmapped = np.flatnonzero(lut[:128] < 0).astype(np.uint8)
    fill = (max(room, 1) - 1) * s + k
    lens = [0, k - 1, k, fill, fill + 1, fill + 3 * s + 5, 2 * fill + 7] + [int(x) for x in rng.integers(k, fill + 1, 3)]
    seqs = []
    for n in lens:
        q = mapped[rng.integers(0, mapped.size, n)]
        if n > 4 and rng.integers(0, 3):
            for _ in range(int(rng.integers(1, 3))):
                a = int(rng.integers(0, n))
                q[a:a + int(rng.integers(1, 4))] = unmapped[rng.integers(0, unmapped.size)]
        seqs.append(bytes(q))
    return seqs


CASES = [(key, k) for key in ("DNA4", "DNA5", "AMINO20") for k in (1, 3, 6)]


@pytest.mark.parametrize("key, k", CASES)
def test_host_twin_equals_numpy_twin(key, k):
    capi, _ = _lib()
    lut, A = _lut(key)
    if A ** k > 2 ** 24:  # (AMINO20, k = 6: the vocabulary bsq_kmer refuses)
        chars, offs = _pack(SEQS)
        st, gi, gl, intact = _host(key, (0, 0, 0), chars, offs, k, 1, 8, _m(capi))
        assert st == capi.ERR_INVALID_ARG and intact and _untouched(gi) and _untouched(gl)
        return
    rng = np.random.default_rng(100 * k + A)
    P, n = 24, 0
    for s in sorted({1, k, 3}):
        for flags in FLAGS:
            room = P - flags[0] - flags[1]
            chars, offs = _pack(_case_batch(rng, lut, k, s, room), lead=b"\xffGG", tail=b"TT\xff")
            vocab = kmer_twin.specials(A, k, *flags)["vocab"]
            for span in sorted({1, 2, k, 16}):
                kw = dict(anchor_prob=0.2, span=span, mask_prob=0.7, random_prob=0.2, mask_token=vocab + 3, ignore_index=-7,
                          seed=1234 + span, first_row=5)
                det = []
                ti, tl = twin.mlm(lut, A, chars, offs, k, s, P, *flags, details=det, **kw)
                m = capi.KmerMlm(0.2, 0.7, 0.2, span, vocab + 3, -7, 1234 + span, 5)
                for bf in (True, False):
                    st, gi, gl, intact = _host(key, flags, chars, offs, k, s, P, m, batch_first=bf)
                    assert st == capi.OK and intact, (s, flags, span, bf)
                    gi, gl = gi.view(np.int64), gl.view(np.int64)
                    assert np.array_equal(gi if bf else gi.T, ti), (s, flags, span, bf)
                    assert np.array_equal(gl if bf else gl.T, tl), (s, flags, span, bf)
                n += sum(int(d[3].sum()) for d in det)
                # the batch holds what it is meant to: rows with no window, a row filled to the last position, a clamped row
                ns = [d[0] for d in det]
                assert 0 in ns and ns.count(room) >= 3
    assert n > 100  # (windows were selected)


def test_every_type_pair_on_the_host():
    capi, _ = _lib()
    lut, A = _lut("DNA4")
    chars, offs = _pack(SEQS + [b"ACGTTGCATGCATGCAAACCGGTT"])
    m = _m(capi, 0.4, seed=3)
    ti, tl = twin.mlm(lut, A, chars, offs, 3, 1, 20, 1, 1, 1, anchor_prob=0.4, span=3, mask_token=65, seed=3)
    for it, lt in itertools.product(range(6), repeat=2):
        st, gi, gl, intact = _host("DNA4", (1, 1, 1), chars, offs, 3, 1, 20, m, it, lt)
        assert st == capi.OK and intact
        for got, want, t in ((gi, ti, it), (gl, tl, lt)):
            exp = want.view(np.uint64) if t == capi.U64 else want.astype(twin.NP_DTYPES[t])
            assert got.tobytes() == exp.tobytes(), (it, lt)
            assert np.array_equal(kmer_twin.back(got), want), (it, lt)  # the values, not the twin through the type


def test_probabilities_at_their_ends():
    capi, _ = _lib()
    lut, A = _lut("DNA4")
    rng = np.random.default_rng(5)
    chars, offs = _pack(_case_batch(rng, lut, 3, 1, 38))
    V, flags, P = 64, (1, 1, 1), 40
    plain = kmer_twin.rows(lut, A, chars, offs, 3, 1, P, *flags)
    body = np.zeros_like(plain, dtype=bool)
    for i in range(len(offs) - 1):
        n = min(kmer_twin.count(int(offs[i + 1] - offs[i]), 3, 1), P - 2)
        body[i, 1:1 + n] = True
    # anchor_prob = 0: the plain ids, no label
    st, gi, gl, _ = _host("DNA4", flags, chars, offs, 3, 1, P, _m(capi, 0.0, mask_token=68))
    assert st == capi.OK and np.array_equal(gi.view(np.int64), plain) and (gl.view(np.int64) == -100).all()
    # anchor_prob = 1: every non-UNK window is selected, nothing else
    for span in (1, 3, 16):
        st, gi, gl, _ = _host("DNA4", flags, chars, offs, 3, 1, P, _m(capi, 1.0, span=span, mask_token=68))
        sel = body & (plain != V)
        assert st == capi.OK and np.array_equal(gl.view(np.int64) != -100, sel) and sel.any() and (body & (plain == V)).any()
        assert np.array_equal(gl.view(np.int64)[sel], plain[sel]) and np.array_equal(gi.view(np.int64)[~sel], plain[~sel])
    # mask_prob = 1: every selected window reads mask_token; random_prob = 1: a plain id in [0, V)
    st, gi, gl, _ = _host("DNA4", flags, chars, offs, 3, 1, P, _m(capi, 0.3, 1.0, 0.0, mask_token=68))
    sel = gl.view(np.int64) != -100
    assert st == capi.OK and sel.any() and (gi.view(np.int64)[sel] == 68).all() and np.array_equal(gi.view(np.int64)[~sel], plain[~sel])
    st, gi, gl, _ = _host("DNA4", flags, chars, offs, 3, 1, P, _m(capi, 1.0, 0.0, 1.0, mask_token=68))
    sel = gl.view(np.int64) != -100
    r = gi.view(np.int64)[sel]
    assert st == capi.OK and r.size > 100 and r.min() >= 0 and r.max() < V and len(set(r.tolist())) > 30
    # mask_prob = random_prob = 0: the inputs are the plain ids, the labels are set
    st, gi, gl, _ = _host("DNA4", flags, chars, offs, 3, 1, P, _m(capi, 0.3, 0.0, 0.0, mask_token=68))
    assert st == capi.OK and np.array_equal(gi.view(np.int64), plain) and (gl.view(np.int64) != -100).any()


def test_refusals_with_their_statuses_nothing_written():
    capi, L = _lib()
    chars, offs = _pack(SEQS)
    nan = float("nan")
    bad_arg = [dict(anchor_prob=-0.1), dict(anchor_prob=1.5), dict(anchor_prob=nan), dict(mask_prob=-0.01), dict(mask_prob=nan),
               dict(random_prob=1.01), dict(random_prob=nan), dict(mask_prob=0.6, random_prob=0.5), dict(span=0), dict(span=17), dict(span=-1),
               dict(first_row=-1), dict(mask_token=-1)]
    for kw in bad_arg:
        st, gi, gl, intact = _host("DNA4", (0, 0, 0), chars, offs, 3, 1, 8, _m(capi, **kw))
        assert st == capi.ERR_INVALID_ARG and intact and _untouched(gi) and _untouched(gl), kw
        assert L.bsq_last_error() != b""
        d, km = capi.make_desc("DNA4"), capi.Kmer(3, 1)
        assert L.bsq_kmer_mlm_kernel_name(ctypes.byref(d), ctypes.byref(km), ctypes.byref(_m(capi, **kw)), 5, 8, 1, 3, 3) == b""
        # the device call refuses the same arguments before it touches a device (host pointers are never read)
        out = np.full(5 * 8 * 8, 0xAB, dtype=np.uint8)
        assert L.bsq_kmer_mlm_tokenize_device(ctypes.byref(d), chars.ctypes.data, offs.ctypes.data, 5, 8, 1, ctypes.byref(km),
                                              ctypes.byref(_m(capi, **kw)), 3, out.ctypes.data, 3, out.ctypes.data, None) == capi.ERR_INVALID_ARG
        assert (out == 0xAB).all()
    # everything bsq_kmer_tokenize_device refuses
    for key, k, s in (("DNA4", 0, 1), ("DNA4", 17, 1), ("DNA4", 13, 1), ("AMINO20", 6, 1), ("DNA4", 3, 0), ("DNA4", 3, -2)):
        st, gi, gl, intact = _host(key, (0, 0, 0), chars, offs, k, s, 8, _m(capi))
        assert st == capi.ERR_INVALID_ARG and intact and _untouched(gi) and _untouched(gl), (key, k, s)
    for kw in (dict(B=-1), dict(P=0), dict(P=-3)):
        st, _, _, intact = _host("DNA4", (0, 0, 0), chars, offs, 3, 1, kw.get("P", 8), _m(capi), B=kw.get("B"))
        assert st == capi.ERR_INVALID_ARG and intact, kw
    st, gi, gl, intact = _host("DNA4", (0, 0, 0), chars, offs, 3, 1, 8, _m(capi), want_in=False, want_lab=False)
    assert st == capi.ERR_INVALID_ARG and intact  # both outputs NULL
    d, km, m = capi.make_desc("DNA4"), capi.Kmer(3, 1), _m(capi)
    out = np.full(5 * 8 * 8, 0xAB, dtype=np.uint8)
    call = lambda fn, d_, c, o, km_, m_, *tail: fn(d_, c, o, 5, 8, 1, km_, m_, 3, out.ctypes.data, 3, out.ctypes.data, *tail)
    for fn, tail in ((L.bsq_kmer_mlm_tokenize_host, ()), (L.bsq_kmer_mlm_tokenize_device, (None,))):
        ok = (ctypes.byref(d), chars.ctypes.data, offs.ctypes.data, ctypes.byref(km), ctypes.byref(m))
        for hole in range(5):
            args = list(ok)
            args[hole] = None
            assert call(fn, *args, *tail) == capi.ERR_INVALID_ARG, (fn, hole)
        assert (out == 0xAB).all()
    # B == 0: nothing to do
    assert L.bsq_kmer_mlm_tokenize_host(ctypes.byref(d), None, None, 0, 8, 1, ctypes.byref(km), ctypes.byref(m), 3, out.ctypes.data, 3, None) == capi.OK
    assert L.bsq_kmer_mlm_tokenize_device(ctypes.byref(d), None, None, 0, 8, 1, ctypes.byref(km), ctypes.byref(m), 3, None, 3, out.ctypes.data,
                                          None) == capi.OK
    # element types: the inputs hold max(vocab - 1, mask_token), the labels V - 1
    I8, I16, I32, U64 = capi.I8, capi.I16, capi.I32, capi.U64
    for key, flags, k, mt, it, lt, want in (("DNA4", (0, 0, 0), 3, 65, I8, I8, capi.OK),          # vocab 65, V 64
                                            ("DNA4", (1, 1, 1), 3, 127, I8, I8, capi.OK),
                                            ("DNA4", (0, 0, 0), 3, 128, I8, I8, capi.ERR_DTYPE),   # mask_token
                                            ("DNA4", (0, 0, 0), 3, 128, I16, I8, capi.OK),
                                            ("DNA4", (0, 0, 0), 4, 0, I8, U64, capi.ERR_DTYPE),    # vocab 257
                                            ("DNA4", (0, 0, 0), 4, 257, I16, I8, capi.ERR_DTYPE),  # V - 1 = 255 in int8 labels
                                            ("PURPYR", (0, 0, 0), 7, 129, I16, I8, capi.OK),       # V - 1 = 127
                                            ("PURPYR", (0, 0, 0), 7, 129, I8, I8, capi.ERR_DTYPE),  # vocab - 1 = 128
                                            ("DNA4", (0, 0, 0), 7, 32767, I16, I16, capi.OK),      # vocab 16385
                                            ("DNA4", (0, 0, 0), 7, 32768, I16, I16, capi.ERR_DTYPE),
                                            ("DNA4", (0, 0, 0), 8, 65537, I32, I16, capi.ERR_DTYPE),  # V - 1 = 65535
                                            ("DNA4", (0, 0, 0), 8, 65537, I32, I32, capi.OK),
                                            ("DNA4", (0, 0, 0), 3, 65, 6, U64, capi.ERR_DTYPE), ("DNA4", (0, 0, 0), 3, 65, U64, -1, capi.ERR_DTYPE)):
        st, gi, gl, intact = _host(key, flags, chars, offs, k, 1, 8, _m(capi, mask_token=mt), it, lt)
        assert st == want and intact, (key, flags, k, mt, it, lt)
        if want != capi.OK:
            assert _untouched(gi) and _untouched(gl)
    # either output alone
    st, gi, gl, intact = _host("DNA4", (0, 0, 0), chars, offs, 3, 1, 8, _m(capi), want_lab=False)
    st2, gi2, gl2, intact2 = _host("DNA4", (0, 0, 0), chars, offs, 3, 1, 8, _m(capi), want_in=False)
    st3, gi3, gl3, _ = _host("DNA4", (0, 0, 0), chars, offs, 3, 1, 8, _m(capi))
    assert st == st2 == st3 == capi.OK and intact and intact2 and _untouched(gl) and _untouched(gi2)
    assert np.array_equal(gi, gi3) and np.array_equal(gl2, gl3)


# (input type, label type, mask_token, ignore_index, accepted): each refusal next to its neighbour at the boundary.  DNA4, k = 3, no flags
# (vocab 65, V - 1 = 63), so only mask_token and ignore_index decide.
EDGE_RULES = [
    ("i", "q", 2 ** 31, -100, False), ("i", "q", 2 ** 31 - 1, -100, True),
    ("f", "q", 2 ** 24 + 1, -100, False), ("f", "q", 2 ** 24, -100, True),
    ("d", "q", 2 ** 53 + 1, -100, False), ("d", "q", 2 ** 53, -100, True),
    ("q", "b", 65, -129, False), ("q", "b", 65, -128, True),
    ("q", "h", 65, -32769, False), ("q", "h", 65, -32768, True),
    ("q", "f", 65, -2 ** 24 - 1, False), ("q", "f", 65, -2 ** 24, True),
    ("q", "b", 65, -1000, False),                                    # (would read as the plain id 24)
    ("q", "b", 65, 128, False), ("q", "b", 65, 127, True),           # a positive ignore_index is bounded too
    ("q", "d", 65, -2 ** 53 - 1, False), ("q", "i", 65, -2 ** 31 - 1, False), ("q", "i", 65, -2 ** 31, True),
    ("q", "q", 2 ** 63 - 1, -2 ** 63, True),                          # 64-bit elements hold every int64
]
CODE = {"b": 0, "h": 1, "i": 2, "q": 3, "f": 4, "d": 5}


@pytest.mark.parametrize("ic, lc, mask_token, ignore_index, ok", EDGE_RULES)
def test_mask_token_and_ignore_index_must_fit_their_types(ic, lc, mask_token, ignore_index, ok):
    """The rule of the element types (bsq_dtype_holds) on the inputs, [0, max(vocab - 1, mask_token)], and on the labels,
    [min(ignore_index, 0), max(ignore_index, V - 1)]: refused with both buffers untouched, accepted with exact values."""
    import bioseq_amd
    from bioseq_amd import kmers
    capi, L = _lib()
    lut, A = _lut("DNA4")
    chars, offs = _pack(SEQS + [b"ACGTTGCATGCATGCAAACCGGTT"])
    it, lt = CODE[ic], CODE[lc]
    assert ok == (kmer_twin.holds(it, 0, max(64, mask_token)) and kmer_twin.holds(lt, min(ignore_index, 0), max(ignore_index, 63)))
    m = _m(capi, 0.4, mask_prob=0.5, random_prob=0.2, mask_token=mask_token, ignore_index=ignore_index, seed=3)
    st, gi, gl, intact = _host("DNA4", (0, 0, 0), chars, offs, 3, 1, 20, m, it, lt)
    d, km = capi.make_desc("DNA4"), capi.Kmer(3, 1)
    name = L.bsq_kmer_mlm_kernel_name(ctypes.byref(d), ctypes.byref(km), ctypes.byref(m), 6, 20, 1, it, lt)
    tok = bioseq_amd.Tokenizer("DNA4")
    kw = dict(anchor_prob=0.4, span=3, mask_prob=0.5, random_prob=0.2, mask_token=mask_token, ignore_index=ignore_index, seed=3, label_destchar=lc)
    if not ok:
        assert st == capi.ERR_DTYPE and intact and _untouched(gi) and _untouched(gl)
        assert L.bsq_last_error() != b"" and name == b""
        # the device call refuses the same arguments before it touches a device (host pointers are never read)
        out = np.full(6 * 20 * 8, 0xAB, dtype=np.uint8)
        assert L.bsq_kmer_mlm_tokenize_device(ctypes.byref(d), chars.ctypes.data, offs.ctypes.data, 6, 20, 1, ctypes.byref(km), ctypes.byref(m),
                                              it, out.ctypes.data, lt, out.ctypes.data, None) == capi.ERR_DTYPE
        assert (out == 0xAB).all()
        with pytest.raises(ValueError):
            kmers.kmer_mlm_tokenize_host(tok, chars, offs, 3, 20, ic, **kw)
        return
    assert st == capi.OK and intact and name == b"k_kmer_mlm_bp<s1>"
    ti, tl = twin.mlm(lut, A, chars, offs, 3, 1, 20, anchor_prob=0.4, span=3, mask_prob=0.5, random_prob=0.2, mask_token=mask_token,
                      ignore_index=ignore_index, seed=3)
    assert (ti == mask_token).any() and (tl == ignore_index).any() and (tl != ignore_index).any()
    assert np.array_equal(kmer_twin.back(gi), ti) and np.array_equal(kmer_twin.back(gl), tl)
    pi, pl = kmers.kmer_mlm_tokenize_host(tok, chars, offs, 3, 20, ic, **kw)
    assert np.array_equal(kmer_twin.back(pi), ti) and np.array_equal(kmer_twin.back(pl), tl)


def test_float_inputs_at_the_largest_vocabulary():
    """V = 2^24 (DNA4, k = 12): f32 inputs are accepted only without BOS / EOS / PAD and with a mask_token <= 2^24 -- the default, the
    vocabulary size 2^24 + 1, is not --; f64 and the integer types take every flag."""
    import bioseq_amd
    from bioseq_amd import kmers
    capi, _ = _lib()
    lut, A = _lut("DNA4")
    chars, offs = _pack([b"T" * 14, b"A" * 13, b"ACGTACGTACGTNACGTACGTACGTA", b""])
    V = 4 ** 12
    for flags in FLAGS:
        vocab = kmer_twin.specials(A, 12, *flags)["vocab"]
        for mt in (V, vocab):
            m = _m(capi, 0.5, 0.5, 0.3, span=2, mask_token=mt, seed=5)
            ti, tl = twin.mlm(lut, A, chars, offs, 12, 1, 8, *flags, anchor_prob=0.5, span=2, mask_prob=0.5, random_prob=0.3, mask_token=mt, seed=5)
            for it, lt in ((capi.F32, capi.F32), (capi.F64, capi.F32), (capi.I32, capi.F64)):
                st, gi, gl, intact = _host("DNA4", flags, chars, offs, 12, 1, 8, m, it, lt)
                if not kmer_twin.holds(it, 0, max(vocab - 1, mt)):
                    assert it == capi.F32 and (any(flags) or mt > V)
                    assert st == capi.ERR_DTYPE and intact and _untouched(gi) and _untouched(gl), (flags, mt, it)
                    continue
                assert st == capi.OK and intact, (flags, mt, it)
                assert np.array_equal(kmer_twin.back(gi), ti) and np.array_equal(kmer_twin.back(gl), tl), (flags, mt, it)
        assert (tl == V - 1).any() and (ti == V).any()  # the top plain id is a label; UNK (the N) and / or the mask token read 2^24
    plain = bioseq_amd.Tokenizer("DNA4")
    with pytest.raises(ValueError):
        kmers.kmer_mlm_tokenize_host(plain, chars, offs, 12, 8, "f")  # the default mask_token = vocab = 2^24 + 1
    assert kmers.kmer_mlm_tokenize_host(plain, chars, offs, 12, 8, "f", mask_token=V)[0].dtype == np.float32
    with pytest.raises(ValueError):
        kmers.kmer_mlm_tokenize_host(bioseq_amd.Tokenizer("DNA4", True, True, True), chars, offs, 12, 8, "f", mask_token=V)


def test_anchor_prob_helper():
    capi, L = _lib()
    for frac, span in itertools.product((0.0, 0.15, 0.5, 1.0), (1, 2, 6, 16)):
        got = L.bsq_kmer_mlm_anchor_prob(frac, span)
        assert got == pytest.approx(1.0 - (1.0 - frac) ** (1.0 / span), abs=1e-15) and got == pytest.approx(twin.span_anchor_prob(frac, span), abs=1e-15)
        assert 1.0 - (1.0 - got) ** span == pytest.approx(frac, abs=1e-12)
    for frac, span in ((-0.1, 3), (1.1, 3), (float("nan"), 3), (0.15, 0), (0.15, 17)):
        assert L.bsq_kmer_mlm_anchor_prob(frac, span) == -float(capi.ERR_INVALID_ARG)


def test_padlen_and_shard_invariance():
    capi, _ = _lib()
    lut, A = _lut("DNA5")
    rng = np.random.default_rng(21)
    chars, offs = _pack(_case_batch(rng, lut, 4, 1, 60), lead=b"NNN")
    for s, span, flags in ((1, 4, (1, 1, 1)), (4, 1, (0, 1, 0)), (3, 2, (1, 0, 1))):
        m = _m(capi, 0.25, span=span, mask_token=700, seed=99, first_row=0)
        P1, P2 = 21, 64
        _, i1, l1, _ = _host("DNA5", flags, chars, offs, 4, s, P1, m)
        _, i2, l2, _ = _host("DNA5", flags, chars, offs, 4, s, P2, m)
        i1, l1, i2, l2 = (x.view(np.int64) for x in (i1, l1, i2, l2))
        # the windows the short row holds carry the values they have in the long one (its last positions hold EOS / PAD instead)
        for b in range(len(offs) - 1):
            n1 = min(kmer_twin.count(int(offs[b + 1] - offs[b]), 4, s), P1 - flags[0] - flags[1])
            w = slice(flags[0], flags[0] + n1)
            assert np.array_equal(i1[b, w], i2[b, w]) and np.array_equal(l1[b, w], l2[b, w]), (s, b)
        assert (l2 != -100).any()
        # a shard with first_row = r equals rows r .. of the whole
        for b0, b1 in ((0, 3), (3, 10), (4, 5), (9, 10)):
            ms = _m(capi, 0.25, span=span, mask_token=700, seed=99, first_row=b0)
            st, pi, pl, intact = _host("DNA5", flags, chars, offs, 4, s, P2, ms, B=b1 - b0, first=b0)
            assert st == capi.OK and intact
            assert np.array_equal(pi.view(np.int64), i2[b0:b1]) and np.array_equal(pl.view(np.int64), l2[b0:b1]), (s, b0, b1)
        # other rows, other masks; another seed, another mask
        _, i3, l3, _ = _host("DNA5", flags, chars, offs, 4, s, P2, _m(capi, 0.25, span=span, mask_token=700, seed=99, first_row=1))
        _, i4, l4, _ = _host("DNA5", flags, chars, offs, 4, s, P2, _m(capi, 0.25, span=span, mask_token=700, seed=100))
        assert not np.array_equal(l3, l2.view(l3.dtype)) and not np.array_equal(l4, l2.view(l4.dtype))


def _long_rows(B, n, k, seed):
    rng = np.random.default_rng(seed)
    L = n + k - 1
    chars = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, B * L)].copy()
    return chars, np.arange(B + 1, dtype=np.int64) * L


@pytest.mark.parametrize("span", [1, 6, 16])
def test_coverage_share_and_span_property(span):
    """>= 200 000 windows of mapped characters: the covered share lies within 4 sigma of 1 - (1 - p)^span, with
    sigma^2 <= f (1 - f) (2 span - 1) / N (the anchors are independent, coverage indicators correlate over 2 span - 1 neighbours), and
    the covered set of every row is exactly the union of [a, a + span) cut at n over its anchors -- on the twin first, then the library."""
    capi, _ = _lib()
    B, n, k, seed = 100, 2048, 6, 20240607
    f = 0.15
    p = twin.span_anchor_prob(f, span)
    p_eff = twin.threshold(p) / 65536.0  # (the threshold is an integer: off p by at most 2^-17, far inside sigma)
    f_eff = 1.0 - (1.0 - p) ** span
    N = B * n
    sigma = math.sqrt(f_eff * (1.0 - f_eff) * (2 * span - 1) / N)
    anch = [twin.anchors(twin.row_key(seed, r), n, p) for r in range(B)]
    cov = np.stack([twin.coverage(a, span) for a in anch])
    share = cov.mean()
    print("span %d: anchors %.5f (p %.5f), covered %.5f (aim %.5f, sigma %.5f)" % (span, np.mean(anch), p_eff, share, f_eff, sigma))
    assert N >= 200000 and abs(share - f_eff) <= 4 * sigma  # the twin, at this seed
    chars, offs = _long_rows(B, n, k, 1)
    st, gi, gl, intact = _host("DNA4", (1, 1, 0), chars, offs, k, 1, n + 2, capi.KmerMlm(p, 0.8, 0.1, span, 4097, -100, seed, 0), capi.I16, capi.I16)
    assert st == capi.OK and intact
    got = gl[:, 1:1 + n] != -100
    assert abs(got.mean() - f_eff) <= 4 * sigma
    # the span property, from the anchors alone: a plain loop per anchor, not the twin's helper
    for r in range(B):
        want = np.zeros(n, dtype=bool)
        for a in np.flatnonzero(anch[r]):
            want[a:a + span] = True
        assert np.array_equal(got[r], want[:n]), r
    assert (gl[:, 0] == -100).all() and (gl[:, n + 1] == -100).all()


def test_python_helpers():
    import bioseq_amd
    from bioseq_amd import kmers
    tok = bioseq_amd.Tokenizer("DNA4", True, True, True)  # (eos, bos, padchar)
    plain = bioseq_amd.Tokenizer("DNA4")
    chars, offs = _pack(SEQS)
    lut, A = _lut("DNA4")
    gi, gl = kmers.kmer_mlm_tokenize_host(plain, chars, offs, 3, 8, anchor_prob=0.5, seed=7)
    assert gi.dtype == np.uint64 and gl.dtype == np.uint64 and gi.shape == gl.shape == (5, 8)
    assert gi[0].tolist() == [65, 65, 47, 65, 0, 0, 0, 0] and gl.view(np.int64)[0].tolist() == [6, 27, 44, 49, -100, -100, -100, -100]
    # the defaults: span = ceil(k / stride), anchor_prob = span_anchor_prob(frac, span), mask_token = the vocabulary size
    for k, s, span in ((3, 1, 3), (3, 3, 1), (6, 4, 2), (1, 1, 1)):
        got = kmers.kmer_mlm_tokenize_host(tok, chars, offs, k, 8, "i", False, stride=s, frac=0.4, seed=11, label_destchar="h")
        assert got[0].dtype == np.int32 and got[1].dtype == np.int16 and got[0].shape == (8, 5)
        ti, tl = twin.mlm(lut, A, chars, offs, k, s, 8, 1, 1, 1, anchor_prob=twin.span_anchor_prob(0.4, span), span=span, seed=11)
        assert np.array_equal(got[0].T, ti) and np.array_equal(got[1].T, tl), (k, s)
    assert kmers.span_anchor_prob(0.15, 6) == pytest.approx(1 - 0.85 ** (1 / 6)) and kmers.span_anchor_prob(0.3, 1) == pytest.approx(0.3)
    assert kmers.kmer_mlm_kernel_name(tok, 6, 1000, 512, "h") == "k_kmer_mlm_bp<s1>"
    assert kmers.kmer_mlm_kernel_name(tok, 6, 1000, 512, "h", stride=6, label_destchar="h") == "k_kmer_mlm_bp<sk>"
    assert kmers.kmer_mlm_kernel_name(tok, 6, 1000, 512, "h", False) == "k_kmer_mlm_generic"
    assert kmers.kmer_mlm_kernel_name(tok, 6, 1000, 512, "h", stride=2) == "k_kmer_mlm_generic"
    assert kmers.kmer_mlm_kernel_name(tok, 9, 1000, 512, "i", stride=9) == "k_kmer_mlm_generic"
    assert kmers.kmer_mlm_kernel_name(tok, 6, 4, 2 ** 24 + 16, "h") == "k_kmer_mlm_generic"
    for kw in (dict(frac=0.2, anchor_prob=0.1), dict(span=0), dict(span=17), dict(frac=1.5), dict(anchor_prob=-0.5), dict(mask_prob=0.7, random_prob=0.4),
               dict(first_row=-1), dict(mask_token=-2), dict(stride=0), dict(mask_prob=float("nan"))):
        with pytest.raises(ValueError):
            kmers.kmer_mlm_tokenize_host(tok, chars, offs, 3, 8, **kw)
    with pytest.raises(ValueError):
        kmers.kmer_mlm_tokenize_host(tok, chars, offs, 3, 8, "b", mask_token=128)
    with pytest.raises(ValueError):
        kmers.kmer_mlm_tokenize_host(tok, chars, offs, 4, 8, "h", label_destchar="b")
    with pytest.raises(ValueError):
        kmers.span_anchor_prob(0.15, 17)
    assert kmers.kmer_mlm_tokenize_host(tok, chars, offs, 3, 8, "b", label_destchar="b")[1].dtype == np.int8


def test_dataset_keywords_without_a_device(tmp_path):
    import bioseq_amd
    from bioseq_amd.flatfile import FlatFile, write_flatfile
    from bioseq_amd.loaders import FlatFileDataset
    ff = FlatFile(write_flatfile([b"ACGTACGTACGT", b"ACG", b""], str(tmp_path / "k.ff")))
    tok = bioseq_amd.Tokenizer("DNA4", True, True, True)
    with pytest.raises(ValueError):
        FlatFileDataset(ff, tok, device="cpu", kmer_mlm=True)  # (only with kmer=)
    for kw in ({"cnn": True}, {"augment": 1}, {"masked": True}, {"pack": "nextfit"}, {"kmer_span": 0}, {"kmer_span": 17}, {"maskfrac": 1.5}):
        with pytest.raises(ValueError):
            FlatFileDataset(ff, tok, device="cpu", kmer=6, kmer_mlm=True, **kw)
    with pytest.raises(ValueError):
        FlatFileDataset(ff, tok, device="cpu", kmer=6, masked=True)  # (as before: the keyword is kmer_mlm)
    ds = FlatFileDataset(ff, tok, device="cpu", kmer=6, kmer_mlm=True)
    assert ds.kmer_mlm and ds.kmer_span is None and ds.max_seq_len == 7 + 2
    assert FlatFileDataset(ff, tok, device="cpu", kmer=6, kmer_mlm=True, kmer_span=3, crop=8, revcomp_frac=0.5).kmer_span == 3
    off = FlatFileDataset(ff, tok, device="cpu", kmer=6)
    assert not off.kmer_mlm  # (off by default)
