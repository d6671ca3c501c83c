"""CPU: codon translation (include/bsq.h, "codon translation") -- the NCBI tables, known answers, the library's host twin
bsq_translate_packed_host against the numpy twin (tests/translate_twin.py) exactly, statuses and cuts, and the argument rules.  No
device is needed."""
import ctypes
from collections import Counter

import numpy as np
import pytest

import translate_twin as twin

# the byte pool of tests/test_views_gpu.py plus U and u
POOL = np.frombuffer(b"ACGTNacgtnRYKMBVDHSWxX*-.\x00\xff\x80@[`{" + b"Uu", dtype=np.uint8)
KNOWN = b"ATGGCCATTGTAATGGGCCGCTGAAAGGGTGCCCGATAG"
ANSWERS = [b"MAIVMGR*KGAR*", b"WPL*WAAERVPD", b"GHCNGPLKGCPI", b"LSGTLSAAHYNGH", b"YRAPFQRPITMA", b"IGHPFSGPLQWP"]


def _lib():
    from bioseq_amd import capi
    return capi, capi.load()


def _store(rng, lens, pool=POOL):
    lens = np.asarray(lens, dtype=np.int64)
    chars = rng.choice(pool, int(lens.sum())).astype(np.uint8)
    offs = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return chars, offs


def _raw_host(chars, offs, index, frames, n, frame, capacity, tab=None, unknown=ord("X")):
    """bsq_translate_packed_host into guarded buffers: (chars, offsets, status)."""
    capi, L = _lib()
    t = capi.Translate()
    code = twin.table(1) if tab is None else np.asarray(tab, np.uint8)
    ctypes.memmove(t.code, code.ctypes.data, 64)
    t.unknown, t.frame = unknown, frame
    n_out = 6 * n if frame == twin.SIX else n
    buf = np.full(capacity + 64, 0xA5, dtype=np.uint8)
    out_offs = np.full(n_out + 1, -7, dtype=np.int64)
    status = ctypes.c_int64(-99)
    ch = chars if chars.size else np.zeros(16, np.uint8)
    capi.check(L.bsq_translate_packed_host(ch.ctypes.data, offs.ctypes.data, offs.size - 1, index.ctypes.data if index is not None else None,
                                           frames.ctypes.data if frames is not None else None, n, ctypes.byref(t), buf[32:].ctypes.data,
                                           capacity, out_offs.ctypes.data, ctypes.byref(status)))
    assert (buf[:32] == 0xA5).all() and (buf[32 + capacity:] == 0xA5).all(), "a guard byte of out_chars was overwritten"
    return buf[32:32 + capacity], out_offs, status.value


def test_new_symbols_are_exported():
    capi, L = _lib()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_codon_table", "bsq_translate_length", "bsq_translate_packed_device", "bsq_translate_packed_host",
              "bsq_translate_kernel_name"):
        assert n in names and hasattr(L, n)
    assert L.bsq_abi_version() == 7
    assert ctypes.sizeof(capi.Translate) == 72 and capi.Translate.frame.offset == 68 and capi.Translate.unknown.offset == 64


def test_tables():
    from bioseq_amd import translate
    t1 = translate.codon_table(1)
    assert t1.dtype == np.uint8 and bytes(t1) == twin.STANDARD.encode()
    counts = Counter(twin.STANDARD)
    assert counts == {"L": 6, "R": 6, "S": 6, "A": 4, "G": 4, "P": 4, "T": 4, "V": 4, "I": 3, "*": 3, "M": 1, "W": 1,
                      "C": 2, "D": 2, "E": 2, "F": 2, "H": 2, "K": 2, "N": 2, "Q": 2, "Y": 2}
    assert chr(t1[twin.codon("ATG")]) == "M" and chr(t1[twin.codon("TGG")]) == "W"
    assert all(chr(t1[twin.codon(c)]) == "*" for c in ("TAA", "TAG", "TGA"))
    changes = {11: {}, 4: {"TGA": "W"}, 2: {"TGA": "W", "ATA": "M", "AGA": "*", "AGG": "*"}}
    for tid, ch in changes.items():
        t = translate.codon_table(tid)
        assert np.array_equal(t, twin.table(tid))
        differ = sorted(np.nonzero(t != t1)[0])
        assert differ == sorted(twin.codon(c) for c in ch)
        for c, letter in ch.items():
            assert chr(t[twin.codon(c)]) == letter
    capi, L = _lib()
    out = np.zeros(64, np.uint8)
    for bad in (0, 3, 5, 12, -1):
        assert L.bsq_codon_table(bad, out.ctypes.data) == capi.ERR_INVALID_ARG
        with pytest.raises(ValueError):
            translate.codon_table(bad)
    assert L.bsq_codon_table(1, None) == capi.ERR_INVALID_ARG
    own = bytes(range(64))
    assert bytes(translate.codon_table(own)) == own


@pytest.mark.parametrize("variant", ["upper", "lower", "rna"])
def test_known_answers(variant):
    from bioseq_amd import translate
    seq = {"upper": KNOWN, "lower": KNOWN.lower(), "rna": KNOWN.replace(b"T", b"U")}[variant]
    chars = np.frombuffer(seq, np.uint8)
    offs = np.array([0, len(seq)], np.int64)
    for code, answer in enumerate(ANSWERS):
        got, go = translate.translate_host(chars, offs, frame=code)
        assert bytes(got) == answer and list(go) == [0, len(answer)], code
        assert bytes(twin.translate_row(chars, code, twin.table(1))) == answer
        assert translate.translated_length(len(seq), code) == len(answer) == twin.length(len(seq), code)
    got, go = translate.translate_host(chars, offs, frame="six")
    assert bytes(got) == b"".join(ANSWERS) and np.array_equal(np.diff(go), [len(a) for a in ANSWERS])
    src, code = translate.six_frame_origin(2)
    assert list(src) == [0] * 6 + [1] * 6 and list(code) == list(range(6)) * 2
    # stop and unknown letters, ambiguity is never resolved
    got, _ = translate.translate_host(chars, offs, frame=0, stop="$")
    assert bytes(got) == ANSWERS[0].replace(b"*", b"$")
    got, _ = translate.translate_host(np.frombuffer(b"GCNGCAgc-\x00CGACG", np.uint8), np.array([0, 15], np.int64), unknown="?")
    assert bytes(got) == b"?A??T"


def test_lengths_0_to_8_every_frame_and_six():
    rng = np.random.default_rng(1)
    lens = np.tile(np.arange(9), 40)
    chars, offs = _store(rng, lens)
    n = lens.size
    for code in list(range(6)) + [twin.SIX]:
        e_chars, e_offs, e_status = twin.translate(chars, offs, frame=code)
        got = _raw_host(chars, offs, None, None, n, code, int(e_offs[-1]))
        assert e_status == -1 and got[2] == -1
        assert np.array_equal(got[1], e_offs) and got[0].tobytes() == e_chars.tobytes(), code
    capi, L = _lib()
    for Lc in range(9):
        for code in range(6):
            assert L.bsq_translate_length(Lc, code) == twin.length(Lc, code)
    assert L.bsq_translate_length(5, 6) == -1 and L.bsq_translate_length(-1, 0) == -1 and L.bsq_translate_length(5, -1) == -1


@pytest.mark.parametrize("tid", [1, 2])
def test_host_twin_equals_numpy_twin_on_random_rows(tid):
    rng = np.random.default_rng(tid)
    # half of the rows from bases only, so that whole codons occur; the others from the full pool
    lens = rng.integers(0, 201, 300)
    chars, offs = _store(rng, lens)
    bases = np.frombuffer(b"ACGTUacgtu", np.uint8)
    for j in range(0, 300, 2):
        chars[offs[j]:offs[j + 1]] = rng.choice(bases, int(lens[j]))
    tab = twin.table(tid)
    index = rng.integers(0, 300, 500).astype(np.int64)  # repeats included
    for code in range(6):
        e = twin.translate(chars, offs, index, frame=code, tab=tab, unknown=ord("?"))
        got = _raw_host(chars, offs, index, None, 500, code, int(e[1][-1]), tab, ord("?"))
        assert got[2] == -1 and np.array_equal(got[1], e[1]) and got[0].tobytes() == e[0].tobytes(), code
    e = twin.translate(chars, offs, index[:100], frame=twin.SIX, tab=tab)
    got = _raw_host(chars, offs, index[:100], None, 100, twin.SIX, int(e[1][-1]), tab)
    assert got[2] == -1 and np.array_equal(got[1], e[1]) and got[0].tobytes() == e[0].tobytes()
    frames = rng.integers(0, 6, 500).astype(np.uint8)
    e = twin.translate(chars, offs, index, frames=frames, tab=tab)
    got = _raw_host(chars, offs, index, frames, 500, 0, int(e[1][-1]), tab)
    assert got[2] == -1 and np.array_equal(got[1], e[1]) and got[0].tobytes() == e[0].tobytes()


def test_status_bad_rows_and_cuts():
    from bioseq_amd import translate
    rng = np.random.default_rng(5)
    lens = rng.integers(3, 120, 50)
    chars, offs = _store(rng, lens)
    index = rng.integers(0, 50, 40).astype(np.int64)
    index[7], index[30] = 50, -1
    frames = rng.integers(0, 6, 40).astype(np.uint8)
    frames[3] = 6
    # per-row frames: the frame code 6 of row 3 comes before the bad index of row 7
    e = twin.translate(chars, offs, index, frames=frames)
    got = _raw_host(chars, offs, index, frames, 40, 0, int(e[1][-1]))
    assert e[2] == 3 and got[2] == 3
    assert np.array_equal(got[1], e[1]) and got[0].tobytes() == e[0].tobytes()
    assert all(np.diff(got[1])[[3, 7, 30]] == 0)
    # six frames: a bad source row is six empty rows and is reported by its own number
    e = twin.translate(chars, offs, index, frame=twin.SIX)
    got = _raw_host(chars, offs, index, None, 40, twin.SIX, int(e[1][-1]))
    assert e[2] == 7 and got[2] == 7 and np.array_equal(got[1], e[1]) and got[0].tobytes() == e[0].tobytes()
    assert not np.diff(got[1])[42:48].any()
    # a capacity one byte short: the last row is cut, nothing is written past it, n_out + its number is reported
    ok = rng.integers(0, 50, 40).astype(np.int64)
    for code in (1, twin.SIX):
        full = twin.translate(chars, offs, ok, frame=code)
        cap = int(full[1][-1]) - 1
        e = twin.translate(chars, offs, ok, frame=code, capacity=cap)
        got = _raw_host(chars, offs, ok, None, 40, code, cap)
        n_out = full[1].size - 1
        assert e[2] == got[2] == n_out + int(np.nonzero(full[1][1:] > cap)[0][0])
        assert np.array_equal(got[1], full[1]) and got[0].tobytes() == e[0].tobytes() == full[0][:cap].tobytes()
    # the Python wrapper: errors with validate, empty rows without
    with pytest.raises(IndexError):
        translate.translate_host(chars, offs, index=index, frame=2)
    got = translate.translate_host(chars, offs, index=index, frame=2, validate=False)
    e = twin.translate(chars, offs, index, frame=2)
    assert np.array_equal(got[1], e[1]) and got[0].tobytes() == e[0].tobytes()
    with pytest.raises(RuntimeError):
        translate.translate_host(chars, offs, index=ok, frame=2, capacity=5)


def test_argument_errors_before_any_launch():
    capi, L = _lib()
    offs = np.array([0, 5, 12, 21], np.int64)
    chars = np.zeros(21, np.uint8)
    out = np.zeros(64, np.uint8)
    out_offs = np.zeros(32, np.int64)
    idx = np.array([0, 2], np.int64)
    frames = np.array([0, 4], np.uint8)
    st = np.zeros(1, np.int64)

    def rule(frame=0):
        t = capi.Translate()
        ctypes.memmove(t.code, twin.table(1).ctypes.data, 64)
        t.unknown, t.frame = ord("X"), frame
        return t

    def call(fn, t, n=2, index=idx.ctypes.data, fr=None, offsets=offs.ctypes.data, out_offsets=out_offs.ctypes.data, ch=chars.ctypes.data,
             cap=64):
        # host pointers are never touched by the device entry: every one of these calls is refused before any HIP call
        args = [ch, offsets, 3, index, fr, n, ctypes.byref(t) if t is not None else None, out.ctypes.data, cap, out_offsets, st.ctypes.data]
        return fn(*args, None) if fn is L.bsq_translate_packed_device else fn(*args)

    for fn in (L.bsq_translate_packed_device, L.bsq_translate_packed_host):
        assert call(fn, rule(7)) == capi.ERR_INVALID_ARG
        assert call(fn, rule(-1)) == capi.ERR_INVALID_ARG
        assert call(fn, rule(capi.FRAME_SIX), fr=frames.ctypes.data) == capi.ERR_INVALID_ARG
        assert call(fn, None) == capi.ERR_INVALID_ARG
        assert call(fn, rule(), offsets=None) == capi.ERR_INVALID_ARG
        assert call(fn, rule(), out_offsets=None) == capi.ERR_INVALID_ARG
        assert call(fn, rule(), ch=None) == capi.ERR_INVALID_ARG
        assert call(fn, rule(), n=-1) == capi.ERR_INVALID_ARG
        assert call(fn, rule(), cap=-1) == capi.ERR_INVALID_ARG
        assert call(fn, rule(), index=None, n=4) == capi.ERR_INVALID_ARG  # no index list, n > n_store
    assert call(L.bsq_translate_packed_host, rule(), fr=frames.ctypes.data) == capi.OK and st[0] == -1
    assert L.bsq_translate_kernel_name(10, ctypes.byref(rule(7))) == b"" and L.bsq_translate_kernel_name(-1, ctypes.byref(rule())) == b""
    assert L.bsq_translate_kernel_name(4096, ctypes.byref(rule(3))) == b"k_translate_small"
    assert L.bsq_translate_kernel_name(4097, ctypes.byref(rule(3))) == b"k_translate_lengths+k_translate_place"
    assert L.bsq_translate_kernel_name(682, ctypes.byref(rule(capi.FRAME_SIX))) == b"k_translate_small"
    assert L.bsq_translate_kernel_name(683, ctypes.byref(rule(capi.FRAME_SIX))) == b"k_translate_lengths+k_translate_place"
    assert L.bsq_translate_kernel_name((1 << 20) + 1, ctypes.byref(rule())) == b"k_translate_lengths+k_translate_scan+k_translate_place"


def test_python_argument_errors_touch_no_device():
    from bioseq_amd import translate
    chars = np.frombuffer(KNOWN, np.uint8)
    offs = np.array([0, 20, len(KNOWN)], np.int64)
    for fn in (translate.translate_packed, translate.translate_host):  # (numpy arrays: translate_packed would refuse them next)
        with pytest.raises(ValueError, match="frame"):
            fn(chars, offs, frame=7)
        with pytest.raises(ValueError, match="64"):
            fn(chars, offs, table=b"F" * 63)
        with pytest.raises(ValueError, match="unknown"):
            fn(chars, offs, unknown="XX")
        with pytest.raises(ValueError):
            fn(chars, offs, frame="all")
        with pytest.raises(ValueError):
            fn(chars, offs, table=3)
    with pytest.raises(IndexError):
        translate.translate_host(chars, offs, index=[0, -1])
    with pytest.raises(ValueError):
        translate.translate_host(chars, offs, frame=[0, 6])
    with pytest.raises(ValueError):
        translate.translate_host(chars, offs, frame=[0, 1, 2])
    with pytest.raises(ValueError):
        translate.translate_packed(chars, offs)  # a host store
    with pytest.raises(ValueError):
        translate.translated_length(10, 6)
    assert list(translate.translated_length(np.array([0, 1, 2, 3, 4, 5, 6]), 4)) == [0, 0, 0, 0, 1, 1, 1]


def test_dataset_translate_arguments(tmp_path):
    import bioseq_amd
    from bioseq_amd.flatfile import FlatFile, write_flatfile
    from bioseq_amd.loaders import FlatFileDataset
    ff = FlatFile(write_flatfile([b"ACGTACGTACGTAC", b"ATGAAA"], str(tmp_path / "t.ff")))
    tok = bioseq_amd.Tokenizer("AMINO20", 1, 1, 1)
    for bad in (3, -1, "six"):
        with pytest.raises(ValueError):
            FlatFileDataset(ff, tok, device="cpu", translate=bad)
    with pytest.raises(ValueError):
        FlatFileDataset(ff, tok, device="cpu", translate=0, codon_table=3)
    # construction alone touches no device; the width is a third of the crop, or of the longest row
    assert FlatFileDataset(ff, tok, device="cpu", translate=0).max_seq_len == 14 // 3 + 2
    ds = FlatFileDataset(ff, tok, device="cpu", translate=1, crop=96, revcomp_frac=0.5)  # (the strand draw is allowed: the store holds nucleotides)
    assert ds.max_seq_len == ds.maxseqlen == 34
    assert FlatFileDataset(ff, bioseq_amd.Tokenizer("AMINO20"), device="cpu", translate=2, crop=100).max_seq_len == 33
    with pytest.raises(ValueError):  # without translation the strand draw still needs a nucleotide tokenizer
        FlatFileDataset(ff, tok, device="cpu", revcomp_frac=0.5)
