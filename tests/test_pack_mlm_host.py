"""CPU: masked-LM batches over sequence-packed rows (include/bsq.h, "sequence packing", bsq_pack_mlm_tokenize_*) -- the library's host
twin against the numpy twin (tests/pack_mlm_twin.py: pack_twin's plan and runs composed with mlm_twin's draw) bit for bit in both modes
and all six element types on each side, the frac = 0 identity with the plain packed encode, the argument rules of the C entry points
and of the Python layer, the kernel names and the dataset keyword.  No device is needed."""
import ctypes
import itertools

import numpy as np
import pytest

import pack_mlm_twin as twin

MODES = ("nextfit", "stream")
FLAGS = list(itertools.product((0, 1), repeat=3))  # (bos, eos, padchar)
GUARD = 64
DESTCHARS = "bhiqfd"
DRAWS = ((0.15, 0.8, 0.1), (1.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.5, 0.5, 0.5))  # (frac, mask_prob, random_prob)


def _lib():
    from bioseq_amd import capi
    return capi, capi.load()


def _tok(key, flags):
    import bioseq_amd
    bos, eos, pad = flags
    return bioseq_amd.Tokenizer(key, bool(eos), bool(bos), bool(pad))


def _lut(key):
    capi, _ = _lib()
    d = capi.make_desc(key)
    return np.frombuffer(bytes(d.lut), dtype=np.int8), int(d.nchars)


def _pack(seqs, lead=b"", tail=b""):
    chars = np.frombuffer(lead + b"".join(seqs) + tail, dtype=np.uint8).copy()
    offs = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=offs[1:])
    return chars, offs + len(lead)


def _guarded(nbytes, fill):
    raw = np.full(nbytes + 2 * GUARD, fill, dtype=np.uint8)
    return raw, raw[GUARD:GUARD + nbytes]


def _intact(raw, nbytes, fill):
    return bool((raw[:GUARD] == fill).all() and (raw[GUARD + nbytes:] == fill).all())


def _mlm(capi, frac, mp, rp, mask_token, seed, first_row, ignore=-100):
    return capi.Mlm(frac, mp, rp, mask_token, ignore, seed, first_row)


def _host(key, flags, chars, offs, P, mode, dt, ldt, m, rows=None, fill=0xAB):
    """bsq_pack_plan_host + bsq_pack_mlm_tokenize_host into guarded buffers pre-filled with `fill` bytes:
    (inputs, labels, seg, pos, starts, n_rows, n_placed, guards intact)."""
    capi, L = _lib()
    bos, eos, pad = flags
    d = capi.make_desc(key, eos=eos, bos=bos, padchar=pad)
    B = len(offs) - 1
    code = capi.PACK_NEXTFIT if mode == "nextfit" else capi.PACK_STREAM
    starts = np.empty(B + 1, dtype=np.int64)
    n_rows, n_placed = ctypes.c_int64(-7), ctypes.c_int64(-7)
    assert L.bsq_pack_plan_host(offs.ctypes.data, B, P, bos, eos, code, rows or 0, starts.ctypes.data, ctypes.addressof(n_rows),
                                ctypes.addressof(n_placed)) == capi.OK
    R = n_rows.value if rows is None else rows
    ti, tl = twin.NP_DTYPES[dt], twin.NP_DTYPES[ldt]
    ni, nl = R * P * np.dtype(ti).itemsize, R * P * np.dtype(tl).itemsize
    iraw, ibuf = _guarded(ni, fill)
    lraw, lbuf = _guarded(nl, fill)
    graw, gbuf = _guarded(R * P * 4, fill)
    praw, pbuf = _guarded(R * P * 4, fill)
    keep = chars if chars.size else np.zeros(16, np.uint8)
    st = L.bsq_pack_mlm_tokenize_host(ctypes.byref(d), keep.ctypes.data, offs.ctypes.data, B, starts.ctypes.data, R, P, ctypes.byref(m), dt,
                                      ibuf.ctypes.data, ldt, lbuf.ctypes.data, gbuf.ctypes.data, pbuf.ctypes.data)
    assert st == capi.OK, L.bsq_last_error()
    intact = _intact(iraw, ni, fill) and _intact(lraw, nl, fill) and _intact(graw, R * P * 4, fill) and _intact(praw, R * P * 4, fill)
    return (ibuf.view(ti).reshape(R, P), lbuf.view(tl).reshape(R, P), gbuf.view(np.int32).reshape(R, P), pbuf.view(np.int32).reshape(R, P),
            starts, n_rows.value, n_placed.value, intact)


def test_new_symbols_are_declared_and_exported():
    capi, L = _lib()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_pack_mlm_tokenize_device", "bsq_pack_mlm_tokenize_host", "bsq_pack_mlm_kernel_name"):
        assert n in names and hasattr(L, n), n
    assert L.bsq_abi_version() == 7
    from bioseq_amd import packing
    for n in ("pack_mlm_tokenize_packed", "pack_mlm_tokenize_host", "pack_mlm_kernel_name", "PackedMlm", "PackedMlmRows"):
        assert n in packing.__all__ and hasattr(packing, n)
    from bioseq_amd import masking
    assert packing._mlm_params is masking._params  # one set of MLM argument rules


def _batches(rng, P, be):
    pool = np.frombuffer(b"ACGTACGTACGTNacgt*\xff", dtype=np.uint8)
    full = max(P - be, 0)

    def seqs(lens):
        return [bytes(rng.choice(pool, int(n))) for n in lens]

    yield "random", seqs(rng.integers(0, max(2, min(P, 70)) + 1, 23))
    yield "exact", seqs([full, 3, 0, full, full, 1, max(full - 1, 0), 1])
    yield "wider", seqs([2, full + 1, 0, 1, full + 1, full + 5, 0])  # (next-fit: cut at P, without validation)
    yield "empty", seqs([0] * 9)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", (1, 15, 16, 17, 100))
def test_host_twin_equals_the_numpy_twin(mode, P):
    capi, _ = _lib()
    rng = np.random.default_rng(31 * P + len(mode))
    types = [(a, a) for a in range(6)] + [(0, 3), (3, 0), (1, 5), (4, 2)]  # every type on each side
    n = 0
    for fi, flags in enumerate(FLAGS):
        be = flags[0] + flags[1]
        for name, seqs in _batches(rng, P, be):
            chars, offs = _pack(seqs, lead=b"\xffGGGG", tail=b"TTTT\xff")  # offsets[0] = 5, junk either side
            for key in (("DNA4", "AMINO20") if name == "random" else ("DNA4",)):
                lut, nchars = _lut(key)
                frac, mp, rp = DRAWS[(fi + n) % len(DRAWS)]
                seed, first_row, mtok = 1000 + n, 7 * (n % 3), nchars + 3 + (n % 2)
                want = twin.pack_mlm(key, flags, lut, nchars, chars, offs, P, mode, frac=frac, mask_prob=mp, random_prob=rp, mask_token=mtok,
                                     seed=seed, first_row=first_row)
                if frac == 1.0 and name == "random" and P >= 15:  # (the twin itself selects something there)
                    assert (want[1] != -100).any()
                for dt, ldt in (types if name == "random" else types[n % 6::6]):
                    m = _mlm(capi, frac, mp, rp, mtok, seed, first_row)
                    got = _host(key, flags, chars, offs, P, mode, dt, ldt, m, fill=0xAB if max(dt, ldt) < 4 else 0xFF)
                    assert got[7], (name, flags, dt, ldt)
                    assert got[4].tolist() == want[4].tolist() and got[5] == want[5] and got[6] == len(seqs), (name, flags)
                    assert got[0].tobytes() == twin.as_dtype(want[0], dt).tobytes(), (name, flags, dt, "inputs")
                    assert got[1].tobytes() == twin.as_dtype(want[1], ldt).tobytes(), (name, flags, ldt, "labels")
                    assert got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[3].tobytes(), (name, flags)
                n += 1
    assert n > 0


@pytest.mark.parametrize("mode", MODES)
def test_rows_n_short_of_the_need_and_resuming(mode):
    from bioseq_amd import packing
    rng = np.random.default_rng(3)
    flags = (1, 1, 1)
    tok = _tok("DNA4", flags)
    lut, nchars = _lut("DNA4")
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), int(n))) for n in rng.integers(0, 30, 40)]
    chars, offs = _pack(seqs, lead=b"NN")
    P = 32
    kw = dict(frac=0.4, seed=99, first_row=5)
    whole = packing.pack_mlm_tokenize_host(tok, chars, offs, P, "h", mode=mode, label_dtype="i", **kw)
    need = whole.n_rows
    for N in (1, 2, need - 1, need, need + 3):
        r = packing.pack_mlm_tokenize_host(tok, chars, offs, P, "h", mode=mode, rows=N, label_dtype="i", **kw)
        t = twin.pack_mlm("DNA4", flags, lut, nchars, chars, offs, P, mode, rows=N, **kw)
        assert r.inputs.shape == (N, P) and r.n_rows == need and r.n_placed == t[6]
        assert np.array_equal(r.starts, t[4]) and np.array_equal(r.inputs, t[0]) and np.array_equal(r.labels, t[1])
        assert np.array_equal(r.segment_ids, t[2]) and np.array_equal(r.position_ids, t[3])
        k = r.n_placed
        if N < need:  # resuming at n_placed with first_row advanced gives every sequence the run of the whole-batch call
            assert 0 < k < len(seqs)
            rest = packing.pack_mlm_tokenize_host(tok, chars, offs[k:], P, "h", mode=mode, label_dtype="i", **dict(kw, first_row=5 + k))
            for i in range(k, len(seqs)):
                w = len(seqs[i]) + 2
                a, b = int(whole.starts[i]), int(rest.starts[i - k])
                assert np.array_equal(whole.inputs.reshape(-1)[a:a + w], rest.inputs.reshape(-1)[b:b + w])
                assert np.array_equal(whole.labels.reshape(-1)[a:a + w], rest.labels.reshape(-1)[b:b + w])


def test_frac_zero_is_the_plain_packed_encode():
    from bioseq_amd import packing
    rng = np.random.default_rng(11)
    for flags, mode, dc in itertools.product(((0, 0, 0), (1, 1, 1), (1, 0, 0)), MODES, "bqf"):
        tok = _tok("AMINO20", flags)
        seqs = [bytes(rng.choice(np.frombuffer(b"ACDEFGHIKLXBZ*", np.uint8), int(n))) for n in rng.integers(0, 40, 50)]
        chars, offs = _pack(seqs, lead=b"abc")
        plain = packing.pack_tokenize_host(tok, chars, offs, 48, dc, mode=mode)
        got = packing.pack_mlm_tokenize_host(tok, chars, offs, 48, dc, mode=mode, frac=0.0, seed=4, ignore_index=-7, label_dtype="h")
        assert got.inputs.dtype == plain.tokens.dtype and got.inputs.tobytes() == plain.tokens.tobytes()
        assert (got.labels == -7).all() and got.labels.dtype == np.int16
        assert np.array_equal(got.segment_ids, plain.segment_ids) and np.array_equal(got.position_ids, plain.position_ids)
        assert np.array_equal(got.starts, plain.starts) and got.n_rows == plain.n_rows


def test_layout_independence_of_the_draw():
    """The run of sequence i equals the head of row i of the padded masked batch (mlm_twin.mlm on the oracle's padded tokens)."""
    import mlm_twin
    import pack_twin
    from bioseq_amd import packing
    rng = np.random.default_rng(12)
    flags = (1, 1, 0)
    tok = _tok("AMINO20", flags)
    lut, nchars = _lut("AMINO20")
    seqs = [bytes(rng.choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYXbz", np.uint8), int(n))) for n in rng.integers(0, 60, 80)]
    chars, offs = _pack(seqs)
    runs = pack_twin.runs("AMINO20", flags, chars, offs)
    padded = np.zeros((len(seqs), 64), dtype=np.int64)
    for i, r in enumerate(runs):
        padded[i, :len(r)] = r
    ei, el = mlm_twin.mlm(padded, lut, nchars, 1, 1, chars, offs, 0.3, 0.8, 0.1, 99, -100, 21, 4)
    for mode, P in (("nextfit", 64), ("stream", 64), ("nextfit", 131), ("stream", 7)):
        got = packing.pack_mlm_tokenize_host(tok, chars, offs, P, mode=mode, frac=0.3, mask_token=99, seed=21, first_row=4)
        fi, fl = got.inputs.reshape(-1).astype(np.int64), got.labels.reshape(-1).astype(np.int64)
        for i, r in enumerate(runs):
            s = int(got.starts[i])
            assert np.array_equal(fi[s:s + len(r)], ei[i, :len(r)]) and np.array_equal(fl[s:s + len(r)], el[i, :len(r)]), (mode, P, i)


def test_argument_rules_nothing_written():
    capi, L = _lib()
    from bioseq_amd import packing
    chars, offs = _pack([b"ACG", b"", b"AC", b"ACGTAC", b"T"])
    tok = _tok("DNA4", (1, 1, 1))
    d = capi.make_desc("DNA4", 1, 1, 1)
    starts = packing.pack_plan_host(tok, offs, 8)[0]
    ins, labs = np.full(64, 0xAB, dtype=np.uint8), np.full(64, 0xAB, dtype=np.uint8)
    seg, pos = np.full(64, 0x5A5A, dtype=np.int32), np.full(64, 0x5A5A, dtype=np.int32)
    good = _mlm(capi, 0.15, 0.8, 0.1, 7, 1, 0)
    base = dict(d=ctypes.byref(d), chars=chars.ctypes.data, offs=offs.ctypes.data, B=5, starts=starts.ctypes.data, rows=1, P=8,
                m=ctypes.byref(good), dt=capi.I8, ins=ins.ctypes.data, ldt=capi.I8, labs=labs.ctypes.data)

    def enc(dev, **kw):
        a = dict(base, **kw)
        args = [a["d"], a["chars"], a["offs"], a["B"], a["starts"], a["rows"], a["P"], a["m"], a["dt"], a["ins"], a["ldt"], a["labs"],
                seg.ctypes.data, pos.ctypes.data]
        return L.bsq_pack_mlm_tokenize_device(*args, None) if dev else L.bsq_pack_mlm_tokenize_host(*args)

    bad_mlm = [_mlm(capi, *a) for a in ((-0.1, 0.8, 0.1, 7, 1, 0), (1.5, 0.8, 0.1, 7, 1, 0), (0.15, 1.1, 0.0, 7, 1, 0), (0.15, 0.8, -0.2, 7, 1, 0),
                                        (0.15, 0.8, 0.3, 7, 1, 0), (float("nan"), 0.8, 0.1, 7, 1, 0), (0.15, 0.8, 0.1, 7, 1, -1))]
    for dev in (False, True):  # (the device entry: stream argument None; every refusal comes before any launch)
        for kw in ({"d": None}, {"chars": None}, {"offs": None}, {"starts": None}, {"B": -1}, {"rows": -1}, {"P": 0}, {"P": 2 ** 30 + 1},
                   {"rows": 2 ** 31 + 1}, {"rows": 2 ** 31, "P": 2 ** 10}, {"m": None}, {"ins": None, "labs": None}):
            assert enc(dev, **kw) == capi.ERR_INVALID_ARG, (dev, kw)
        for m in bad_mlm:
            assert enc(dev, m=ctypes.byref(m)) == capi.ERR_INVALID_ARG
        assert L.bsq_last_error() != b""
        for bad in (-1, 6):
            assert enc(dev, dt=bad) == capi.ERR_DTYPE and enc(dev, ldt=bad) == capi.ERR_DTYPE
        assert enc(dev, rows=0) == capi.OK and enc(dev, B=0) == capi.OK  # nothing to write, nothing launched
        assert (ins == 0xAB).all() and (labs == 0xAB).all() and (seg == 0x5A5A).all() and (pos == 0x5A5A).all()
    if L.bsq_device_count() == 0:
        assert enc(True) in (capi.ERR_NO_DEVICE, capi.ERR_HIP)
    # one output alone is fine on the host
    assert enc(False, ins=None) == capi.OK and (ins == 0xAB).all() and not (labs[:8] == 0xAB).all()
    assert L.bsq_pack_mlm_kernel_name(ctypes.byref(d), 5, 4, 8, capi.I8) == b"k_pack_mlm_flat<perm>"
    assert L.bsq_pack_mlm_kernel_name(ctypes.byref(capi.make_desc("BYTES")), 5, 4, 8, capi.U64) == b"k_pack_mlm_flat<lut>"
    assert L.bsq_pack_mlm_kernel_name(ctypes.byref(d), 5, 4, 0, capi.I8) == b"" and L.bsq_pack_mlm_kernel_name(None, 5, 4, 8, capi.I8) == b""
    assert L.bsq_pack_mlm_kernel_name(ctypes.byref(d), 5, 4, 8, 6) == b""
    assert packing.pack_mlm_kernel_name(tok, 100, 10, 1024, "q") == "k_pack_mlm_flat<perm>"
    # the Python layer: ValueError before any device work
    for kw in (dict(mode="bestfit"), dict(padlen=0), dict(padlen=-4), dict(rows=0), dict(rows=-2), dict(padlen=2 ** 30 + 1), dict(frac=1.5),
               dict(frac=-0.1), dict(mask_prob=0.9, random_prob=0.2), dict(random_prob=2.0), dict(first_row=-1)):
        a = dict(dict(padlen=8), **kw)
        P = a.pop("padlen")
        with pytest.raises(ValueError):
            packing.pack_mlm_tokenize_host(tok, chars, offs, P, **a)
        with pytest.raises(ValueError):
            packing.pack_mlm_tokenize_packed(tok, chars, offs, P, **a)
    with pytest.raises(ValueError):
        packing.pack_mlm_tokenize_packed(tok, chars, offs, 8)  # host arrays: the device call takes resident batches
    none = packing.pack_mlm_tokenize_host(tok, np.zeros(0, np.uint8), np.zeros(1, np.int64), 4, rows=2)
    assert (none.inputs == tok.pad()).all() and (none.labels.astype(np.int64) == -100).all() and none.n_placed == 0


def test_dataset_keyword_without_a_device(tmp_path):
    import bioseq_amd
    from bioseq_amd.flatfile import FlatFile, write_flatfile
    from bioseq_amd.loaders import FlatFileDataset
    ff = FlatFile(write_flatfile([b"ACGTACGTACGT", b"ACG", b""], str(tmp_path / "p.ff")))
    tok = bioseq_amd.Tokenizer("DNA4", True, True, True)
    with pytest.raises(ValueError, match="pack="):
        FlatFileDataset(ff, tok, device="cpu", pack_mlm=True)
    for mode in MODES:
        for kw in ({"cnn": True}, {"augment": 1}, {"kmer": 3}, {"masked": True}):
            with pytest.raises(ValueError):
                FlatFileDataset(ff, tok, device="cpu", pack=mode, pack_mlm=True, **kw)
        with pytest.raises(ValueError, match="pack_mlm"):
            FlatFileDataset(ff, tok, device="cpu", pack=mode, masked=True)
        ds = FlatFileDataset(ff, tok, device="cpu", pack=mode, pack_mlm=True)
        assert ds.pack_mlm and ds.pack == mode and ds.max_seq_len == 14
        with pytest.raises(ValueError):
            next(iter(ds.batches(2, shuffle=False, group=2)))
        assert FlatFileDataset(ff, tok, device="cpu", pack=mode, pack_mlm=True, crop=8, revcomp_frac=0.5).max_seq_len == 10
        assert not FlatFileDataset(ff, tok, device="cpu", pack=mode).pack_mlm  # (off by default)


@pytest.mark.parametrize("mode", MODES)
def test_an_alphabet_whose_special_ids_exceed_a_byte(mode):
    """BYTES: 256 classes, BOS / EOS / PAD = 256 / 257 / 258 and random ids up to 255."""
    from bioseq_amd import packing
    rng = np.random.default_rng(9)
    flags = (1, 1, 1)
    tok = _tok("BYTES", flags)
    lut, nchars = _lut("BYTES")
    assert nchars == 256
    seqs = [bytes(rng.integers(0, 256, int(n)).astype(np.uint8)) for n in rng.integers(0, 50, 30)]
    chars, offs = _pack(seqs, lead=b"xy")
    for frac, mp, rp in DRAWS:
        got = packing.pack_mlm_tokenize_host(tok, chars, offs, 64, "q", mode=mode, frac=frac, mask_prob=mp, random_prob=rp, seed=2)
        want = twin.pack_mlm("BYTES", flags, lut, nchars, chars, offs, 64, mode, frac=frac, mask_prob=mp, random_prob=rp, seed=2)
        assert np.array_equal(got.inputs.astype(np.int64), want[0]) and np.array_equal(got.labels.astype(np.int64), want[1])
        assert want[0].max() >= 256 and np.array_equal(got.segment_ids, want[2])
