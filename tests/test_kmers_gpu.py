"""GPU: k-mer ids of packed batches (bioseq_amd.kmers, bsq_kmer_tokenize_device) against the numpy twin (tests/kmer_twin.py) bit for
bit on shapes that reach each kernel, the fast kernel against the generic one, the composition with the views, and the k-mer
FlatFileDataset."""
import ctypes

import numpy as np
import pytest

import kmer_twin as twin
import views_twin

pytestmark = pytest.mark.gpu

DNA_POOL = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTNacgtn*\xff", dtype=np.uint8)  # mostly mapped, some N / lower case / junk


def _lut(key):
    from bioseq_amd import capi
    lut = (ctypes.c_int8 * 256)()
    n = ctypes.c_int32(0)
    assert capi.load().bsq_lut_get(key.encode(), lut, ctypes.byref(n)) == capi.OK
    return np.array(lut, dtype=np.int8), n.value


def _batch(rng, B, maxlen, k, pool=DNA_POOL, fixed=False, pins=()):
    """Packed batch whose LAST row ends at the last byte of chars; rows of length 0, < k and == k among the first ones.
    pins: (length, byte or None) for rows 4, 5, ...: rows of that length, filled with that byte (None: drawn from the pool)."""
    lens = np.full(B, maxlen, dtype=np.int64) if fixed else rng.integers(0, maxlen + 1, B).astype(np.int64)
    if B > 4 and not fixed:
        lens[:4] = (0, max(k - 1, 0), k, 0)
        lens[-1] = maxlen
    for r, (n, _) in enumerate(pins):
        lens[4 + r] = n
    chars = rng.choice(pool, int(lens.sum())).astype(np.uint8)
    offs = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    for r, (_, byte) in enumerate(pins):
        if byte is not None:
            chars[offs[4 + r]:offs[5 + r]] = byte
    return chars, offs


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _tok(bsq, key, flags):
    bos, eos, pad = flags
    return bsq.Tokenizer(key, bool(eos), bool(bos), bool(pad))


def _expect(key, flags, chars, offs, k, s, P, batch_first, np_dtype):
    lut, A = _lut(key)
    m = twin.rows_fast(lut, A, chars, offs, k, s, P, *flags)
    return np.ascontiguousarray(m if batch_first else m.T).astype(np_dtype)


NP_OF = {"b": np.int8, "h": np.int16, "i": np.int32, "q": np.int64, "f": np.float32, "d": np.float64}

# (kernel, key, k, stride, B, P, flags, destchars, maxlen): P % 16 == 0 and != 0, B * ceil(P / 16) a multiple of 256 and not
FAST_CASES = [
    ("k_kmer_bp<s1>", "DNA4", 6, 1, 1024, 512, (1, 1, 1), "hiqfd", 517),   # whole blocks: every store staged; over-long rows clamped
    ("k_kmer_bp<s1>", "DNA4", 6, 1, 1001, 512, (0, 0, 0), "hq", 512),      # a partial last block (unstaged stores), no BOS
    ("k_kmer_bp<s1>", "DNA4", 3, 1, 777, 100, (1, 1, 1), "bhiqfd", 100),   # P % 16 != 0: row pieces, every element size
    ("k_kmer_bp<s1>", "DNA4", 3, 1, 300, 17, (0, 1, 0), "bq", 30),
    ("k_kmer_bp<s1>", "DNA4", 1, 1, 513, 64, (1, 0, 1), "bh", 70),         # k = 1: both loads are the same 16 bytes
    ("k_kmer_bp<s1>", "DNA4", 12, 1, 300, 48, (1, 1, 1), "iq", 64),
    ("k_kmer_bp<s1>", "AMINO20", 5, 1, 400, 96, (1, 1, 1), "iqf", 110),    # an alphabet that is not a power of two
    ("k_kmer_bp<s1>", "PURPYR", 16, 1, 200, 32, (0, 0, 1), "iq", 60),
    ("k_kmer_bp<s1>", "BYTES", 3, 1, 100, 33, (1, 1, 0), "iq", 40),        # ids up to 2^24
    ("k_kmer_bp<sk>", "DNA4", 6, 6, 1024, 96, (1, 1, 1), "hiqfd", 600),    # whole blocks; over-long rows clamped
    ("k_kmer_bp<sk>", "DNA4", 6, 6, 1001, 87, (0, 0, 0), "hq", 512),
    ("k_kmer_bp<sk>", "DNA4", 3, 3, 555, 40, (1, 0, 1), "bhiqfd", 115),
    ("k_kmer_bp<sk>", "DNA4", 8, 8, 300, 16, (0, 1, 1), "iq", 130),
    ("k_kmer_bp<sk>", "DNA4", 2, 2, 300, 50, (1, 1, 0), "bq", 101),
    ("k_kmer_bp<sk>", "AMINO20", 5, 5, 300, 32, (1, 1, 1), "iq", 170),
]


@pytest.mark.parametrize("kernel, key, k, s, B, P, flags, destchars, maxlen", FAST_CASES)
def test_fast_kernels_equal_the_twin_and_the_generic_kernel(gpu, bsq, kernel, key, k, s, B, P, flags, destchars, maxlen):
    import torch
    from bioseq_amd import kmers
    rng = np.random.default_rng(B * 31 + P + k)
    pool = np.arange(256, dtype=np.uint8) if key == "BYTES" else (
        np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQRSTVWYXBZ*acd", np.uint8) if key == "AMINO20" else DNA_POOL)
    chars, offs = _batch(rng, B, maxlen, k, pool)
    assert offs[-1] == chars.size  # the last row ends at the last byte of the buffer: the guarded tail loads
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    tok = _tok(bsq, key, flags)
    for dc in destchars:
        assert kmers.kmer_kernel_name(tok, k, B, P, dc, True, stride=s) == kernel
        assert kmers.kmer_kernel_name(tok, k, B, P, dc, False, stride=s) == "k_kmer_generic"
        got = kmers.kmer_tokenize_packed(tok, dch, dof, k, P, dc, True, stride=s, validate=False)
        slow = kmers.kmer_tokenize_packed(tok, dch, dof, k, P, dc, False, stride=s, validate=False)
        torch.cuda.synchronize()
        assert got.shape == (B, P) and slow.shape == (P, B) and got.is_contiguous()
        exp = _expect(key, flags, chars, offs, k, s, P, True, NP_OF[dc])
        assert got.cpu().numpy().tobytes() == exp.tobytes(), (kernel, dc)
        assert torch.equal(got, slow.t()), (kernel, dc)
        # the library's CPU twin says the same
        host = kmers.kmer_tokenize_host(tok, chars, offs, k, P, dc, True, stride=s)
        assert host.tobytes() == exp.tobytes()


@pytest.mark.parametrize("k, s, B, P, bf, flags", [(6, 1, 500, 100, False, (1, 1, 1)), (6, 6, 500, 32, False, (0, 0, 0)),
                                                   (6, 2, 500, 64, True, (1, 1, 1)), (4, 7, 300, 33, True, (0, 1, 0)),
                                                   (9, 9, 300, 16, True, (1, 1, 1)), (3, 5, 64, 1, True, (1, 1, 1))])
def test_generic_kernel_equals_the_twin(gpu, bsq, k, s, B, P, bf, flags):
    import torch
    from bioseq_amd import kmers
    rng = np.random.default_rng(k * 100 + s)
    chars, offs = _batch(rng, B, 200, k)
    tok = _tok(bsq, "DNA4", flags)
    for dc in "hiqfd" if k <= 6 else "iq":
        assert kmers.kmer_kernel_name(tok, k, B, P, dc, bf, stride=s) == "k_kmer_generic"
        got = kmers.kmer_tokenize_packed(tok, _dev(chars, gpu), _dev(offs, gpu), k, P, dc, bf, stride=s, validate=False)
        torch.cuda.synchronize()
        assert got.cpu().numpy().tobytes() == _expect("DNA4", flags, chars, offs, k, s, P, bf, NP_OF[dc]).tobytes(), dc


CODE = {"b": 0, "h": 1, "i": 2, "q": 3, "f": 4, "d": 5}
S1K, SKK, GENK = "k_kmer_bp<s1>", "k_kmer_bp<sk>", "k_kmer_generic"
# (kernel, key, k, stride, batch_first): the vocabularies at and next to A^k = 2^24, through every kernel
TOP_CASES = ([(S1K, key, k, 1, True) for key, k in (("DNA4", 12), ("SEB8", 8), ("BYTES", 3), ("AMINO20", 5), ("PURPYR", 16))] +
             [(SKK, key, k, k, True) for key, k in (("SEB8", 8), ("BYTES", 3), ("AMINO20", 5))] +
             [(GENK, key, k, 1, False) for key, k in (("DNA4", 12), ("SEB8", 8), ("BYTES", 3), ("AMINO20", 5), ("PURPYR", 16))] +
             [(GENK, key, k, k, False) for key, k in (("SEB8", 8), ("BYTES", 3), ("AMINO20", 5))] + [(GENK, "DNA4", 12, 12, True)])


@pytest.mark.parametrize("kernel, key, k, s, bf", TOP_CASES)
def test_top_of_the_id_range_in_every_element_type(gpu, bsq, kernel, key, k, s, bf):
    """B = 37 rows at P = 40 (row pieces, unstaged stores) and P = 272 (629 pieces: two staged workgroups and a partial one), without
    flags and with all three.  Every element type the rule of include/bsq.h accepts -- 'f' and 'd' included -- holds the twin's values
    when cast back to int64 (the expected side never passes through the element type); every other type is a ValueError, and the raw
    entry point refuses it with BSQ_ERR_DTYPE and writes nothing.  Each batch holds 0, the top id (a whole lane of it), UNK and the
    enabled specials -- asserted, or the case would prove nothing."""
    import torch
    from bioseq_amd import capi, kmers
    L = capi.load()
    lut, A = _lut(key)
    V, B = A ** k, 37
    first, last, _, top = twin.edge_bytes(lut, A, k)
    assert top == V - 1 or key == "BYTES"  # (BYTES maps the bytes below 0x80 only: its top id is 127 * (V - 1) / 255)
    pool = twin.edge_pool(lut)
    for P, flags in ((40, (0, 0, 0)), (40, (1, 1, 1)), (272, (0, 0, 0)), (272, (1, 1, 1))):
        rng = np.random.default_rng(P + k + s + flags[0])
        room = P - flags[0] - flags[1]
        fill = (room - 1) * s + k
        # rows 4 ..: k + 15 copies of the last class (a lane's 16 windows at the top id), of the first class, a row that fills the
        # matrix exactly; the last row is over-long (clamped) and ends at the last byte of chars
        chars, offs = _batch(rng, B, fill + 2 * s + 3, k, pool, pins=((k + 15 * s, last), (k + 15 * s, first), (fill, None)))
        assert offs[-1] == chars.size and offs[-1] - offs[-2] > fill
        dch, dof = _dev(chars, gpu), _dev(offs, gpu)
        tok = _tok(bsq, key, flags)
        sp = twin.specials(A, k, *flags)
        want = twin.rows_fast(lut, A, chars, offs, k, s, P, *flags)
        stored = [0, top, sp["unk"]] + [sp[n] for n, on in zip(("bos", "eos", "pad"), flags) if on]
        assert set(stored) <= set(want.reshape(-1).tolist()), (P, flags)
        assert (want[4, flags[0]:flags[0] + 16] == top).all()
        accepted = []
        for dc in "bhiqfd":
            if not twin.holds(CODE[dc], 0, sp["vocab"] - 1):
                with pytest.raises(ValueError):
                    kmers.kmer_tokenize_packed(tok, dch, dof, k, P, dc, bf, stride=s, validate=False)
                d, km = capi.make_desc(key, eos=flags[1], bos=flags[0], padchar=flags[2]), capi.Kmer(k, s)
                buf = torch.full((B * P + 512,), -77, dtype=capi.torch_dtype(CODE[dc]), device=gpu)
                st = L.bsq_kmer_tokenize_device(ctypes.byref(d), dch.data_ptr(), dof.data_ptr(), B, P, int(bf), ctypes.byref(km), CODE[dc],
                                                buf.data_ptr() + 256 * buf.element_size(), None)
                torch.cuda.synchronize()
                assert st == capi.ERR_DTYPE and bool((buf == -77).all()), (P, flags, dc)
                continue
            assert kmers.kmer_kernel_name(tok, k, B, P, dc, bf, stride=s) == kernel
            got = kmers.kmer_tokenize_packed(tok, dch, dof, k, P, dc, bf, stride=s, validate=False)
            torch.cuda.synchronize()
            vals = got.cpu().numpy().astype(np.int64)
            assert np.array_equal(vals if bf else vals.T, want), (kernel, P, flags, dc)
            accepted.append(dc)
        assert "".join(accepted) == ("iqfd" if V < 2 ** 24 or not any(flags) else "iqd"), (P, flags, accepted)


def test_guard_bytes_offsets_not_at_zero_and_an_empty_batch(gpu, bsq):
    """The raw entry point on a batch inside a larger buffer (offsets[0] > 0), into the middle of a guarded output, on a side stream;
    B == 0 launches nothing."""
    import torch
    from bioseq_amd import capi
    L = capi.load()
    rng = np.random.default_rng(5)
    chars, offs = _batch(rng, 333, 90, 4)
    lead = 7
    big = np.concatenate([np.full(lead, ord("N"), np.uint8), chars])
    offs = offs + lead
    dch, dof = _dev(big, gpu), _dev(offs, gpu)
    d = capi.make_desc("DNA4", eos=True, bos=True, padchar=True)
    side = torch.cuda.Stream(device=gpu)
    for k, s, P in ((4, 1, 80), (4, 4, 32), (4, 1, 37), (4, 3, 20)):
        km = capi.Kmer(k, s)
        n = 333 * P
        buf = torch.full((n + 512,), -77, dtype=torch.int16, device=gpu)
        side.wait_stream(torch.cuda.current_stream())
        capi.check(L.bsq_kmer_tokenize_device(ctypes.byref(d), dch.data_ptr(), dof.data_ptr(), 333, P, 1, ctypes.byref(km), capi.I16,
                                              buf.data_ptr() + 256 * 2, ctypes.c_void_p(side.cuda_stream)))
        side.synchronize()
        raw = buf.cpu().numpy()
        assert (raw[:256] == -77).all() and (raw[256 + n:] == -77).all(), "a guard element of out was overwritten"
        exp = _expect("DNA4", (1, 1, 1), big, offs, k, s, P, True, np.int16)
        assert raw[256:256 + n].tobytes() == exp.tobytes(), (k, s, P)
        capi.check(L.bsq_kmer_tokenize_device(ctypes.byref(d), dch.data_ptr(), dof.data_ptr(), 0, P, 1, ctypes.byref(km), capi.I16,
                                              buf.data_ptr(), ctypes.c_void_p(side.cuda_stream)))
        capi.check(L.bsq_kmer_tokenize_device(ctypes.byref(d), None, None, 0, P, 1, ctypes.byref(km), capi.I16, None, None))
        side.synchronize()
        assert (buf[:256].cpu().numpy() == -77).all()


def test_python_call_validates_and_handles_empty_batches(gpu, bsq):
    import torch
    from bioseq_amd import kmers
    tok = _tok(bsq, "DNA4", (1, 1, 1))
    chars, offs = _batch(np.random.default_rng(1), 50, 40, 3, fixed=True)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    P = kmers.kmer_padlen(tok, 3, 40)
    assert P == 40 and kmers.kmer_max_length(tok, 3, P) == 40
    got = kmers.kmer_tokenize_packed(tok, dch, dof, 3, P)  # validate=True: every row fits
    assert got.dtype == torch.int64 and got.shape == (50, 40)
    assert np.array_equal(got.cpu().numpy(), twin.rows_fast(*_lut("DNA4"), chars, offs, 3, 1, P, 1, 1, 1))
    with pytest.raises(RuntimeError):
        kmers.kmer_tokenize_packed(tok, dch, dof, 3, P - 1)  # 38 windows + BOS + EOS do not fit 39
    assert kmers.kmer_tokenize_packed(tok, dch, dof, 3, P - 1, validate=False).shape == (50, 39)  # (clamped)
    assert kmers.kmer_tokenize_packed(tok, dch, dof, 3, 15, stride=3, validate=True).shape == (50, 15)  # 13 windows: 40 <= 13 * 3 + 2
    with pytest.raises(RuntimeError):
        kmers.kmer_tokenize_packed(tok, dch, dof, 3, 14, stride=2)
    bad = dof.clone()
    bad[3] = bad[2] - 1
    with pytest.raises(RuntimeError):
        kmers.kmer_tokenize_packed(tok, dch, bad, 3, P)  # malformed offsets
    empty = kmers.kmer_tokenize_packed(tok, dch[:0], dof[:1], 3, 8)
    assert empty.shape == (0, 8)
    zeros = torch.zeros(4, dtype=torch.int64, device=gpu)
    allempty = kmers.kmer_tokenize_packed(tok, dch[:0], zeros, 3, 4, "h")
    assert allempty.cpu().tolist() == [[65, 66, 67, 67]] * 3
    with pytest.raises(ValueError):
        kmers.kmer_tokenize_packed(tok, chars, offs, 3, 8)  # host arrays: the device call takes resident batches
    with pytest.raises(ValueError):
        kmers.kmer_tokenize_packed(tok, dch, dof, 13, 8)
    with pytest.raises(ValueError):
        kmers.kmer_tokenize_packed(tok, dch, dof, 4, 8, "b")


def test_reverse_complemented_crops_into_six_mers(gpu, bsq):
    """views.crop_packed(..., revcomp_frac=1) -> kmer_tokenize_packed equals the twin applied to the host-side reverse complement."""
    import torch
    from bioseq_amd import kmers, views
    rng = np.random.default_rng(21)
    chars, offs = _batch(rng, 2000, 3000, 6)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    tok = _tok(bsq, "DNA4", (1, 1, 0))
    for s in (1, 6):
        P = kmers.kmer_padlen(tok, 6, 1000, stride=s)
        vch, vof = views.crop_packed(dch, dof, 1000, revcomp_frac=1.0, seed=77)
        got = kmers.kmer_tokenize_packed(tok, vch, vof, 6, P, "h", stride=s)
        torch.cuda.synchronize()
        e_chars, e_offs, _, strand = views_twin.crop(chars, offs, 1000, revcomp_frac=1.0, seed=77)
        assert strand.all()
        exp = _expect("DNA4", (1, 1, 0), e_chars, e_offs, 6, s, P, True, np.int16)
        assert got.cpu().numpy().tobytes() == exp.tobytes(), s


def test_kmer_dataset_epochs(gpu, bsq, tmp_path):
    import torch
    from bioseq_amd.flatfile import FlatFile, write_flatfile
    from bioseq_amd.loaders import FlatFileDataset
    rng = np.random.default_rng(2)
    lens = rng.integers(0, 900, 1000)
    lens[:3] = (0, 5, 5000)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGTACGTACGTNacgtRY", np.uint8), int(n))) for n in lens]
    ff = FlatFile(write_flatfile(seqs, str(tmp_path / "kmers.ff")))
    tok = _tok(bsq, "DNA4", (1, 1, 1))
    for kw in ({"cnn": True}, {"augment": 1}, {"masked": True}):
        with pytest.raises(ValueError):
            FlatFileDataset(ff, tok, device=gpu, kmer=6, **kw)
    lut, A = _lut("DNA4")
    for crop, frac, stride in ((256, 0.5, 1), (256, 1.0, 6), (None, 0.0, 1)):
        def epoch(**opts):
            ds = FlatFileDataset(ff, tok, device=gpu, kmer=6, kmer_stride=stride, crop=crop, revcomp_frac=frac, token_dtype="i")
            g = torch.Generator(device=gpu).manual_seed(5)
            out = [b.clone() for b in ds.batches(128, generator=g, **opts)]
            torch.cuda.synchronize()
            return ds, out

        ds, base = epoch()
        longest = crop if crop else 5000
        width = (longest - 6) // stride + 1 + 2
        assert ds.max_seq_len == width and all(b.dtype == torch.int32 and b.shape[1] == width for b in base)
        g = torch.Generator(device=gpu).manual_seed(5)
        order = torch.randperm(len(ff), device=gpu, generator=g).cpu().numpy()
        if crop or frac:
            key = (13 * 0xC2B2AE3D27D4EB4F + 1) & (2 ** 64 - 1)  # the dataset's first view key (seed 13)
            starts, lengths, strand = views_twin.plan(ff._offsets, crop or 0, order, mode="random", revcomp_frac=frac, seed=key, first_row=0)
            e_chars, e_offs = views_twin.apply(np.asarray(ff._chars), ff._offsets, order, starts, lengths, strand)
        else:
            e_chars = np.frombuffer(b"".join(seqs[i] for i in order), np.uint8)
            e_offs = np.concatenate([[0], np.cumsum([len(seqs[i]) for i in order])]).astype(np.int64)
        exp = twin.rows_fast(lut, A, e_chars, e_offs, 6, stride, width, 1, 1, 1).astype(np.int32)
        assert torch.cat(base).cpu().numpy().tobytes() == exp.tobytes(), (crop, frac, stride)
        for opts in ({"group": 4}, {"group": 4, "prefetch": 2}):
            _, got = epoch(**opts)
            assert len(got) == len(base) and all(torch.equal(a, b) for a, b in zip(base, got)), opts
        # the other access paths hand out rows of the same width
        assert ds[1].shape == (width,) and ds.get_batch(0, 10).shape == (10, width)


def _fold(a, first):
    """64-bit fold of a chunk of the flattened matrix whose first element has the global index `first`."""
    idx = np.arange(first, first + a.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        w = idx * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
        return int((a.reshape(-1).astype(np.int64).astype(np.uint64) * w).sum(dtype=np.uint64))


@pytest.mark.slow
@pytest.mark.parametrize("s, P", [(1, 512), (6, 96)])
def test_baseline_sized_batch(gpu, bsq, s, P):
    """262 144 DNA4 reads of 512 characters, k = 6, int16: the fold of the result equals the fold of the twin, chunk by chunk."""
    import torch
    from bioseq_amd import kmers
    B, Lmax, step = 262144, 512, 16384
    rng = np.random.default_rng(99)
    lens = rng.integers(400, Lmax + 1, B).astype(np.int64)
    chars = rng.choice(DNA_POOL, int(lens.sum())).astype(np.uint8)
    offs = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    tok = _tok(bsq, "DNA4", (1, 1, 1))
    assert kmers.kmer_kernel_name(tok, 6, B, P, "h", True, stride=s) == ("k_kmer_bp<s1>" if s == 1 else "k_kmer_bp<sk>")
    got = kmers.kmer_tokenize_packed(tok, _dev(chars, gpu), _dev(offs, gpu), 6, P, "h", stride=s)
    torch.cuda.synchronize()
    lut, A = _lut("DNA4")
    f_got = f_exp = 0
    for b0 in range(0, B, step):
        o = offs[b0:b0 + step + 1]
        exp = twin.rows_fast(lut, A, chars[o[0]:o[-1]], o - o[0], 6, s, P, 1, 1, 1).astype(np.int16)
        part = got[b0:b0 + step].cpu().numpy()
        a, b = _fold(part, b0 * P), _fold(exp, b0 * P)
        assert a == b, "rows %d .. %d differ" % (b0, b0 + step)
        f_got, f_exp = (f_got + a) & (2 ** 64 - 1), (f_exp + b) & (2 ** 64 - 1)
    assert f_got == f_exp
