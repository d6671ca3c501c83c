"""GPU: masked-LM batches over sequence-packed rows (bioseq_amd.packing.pack_mlm_tokenize_packed, bsq_pack_mlm_tokenize_device) against
the numpy twin (tests/pack_mlm_twin.py) and the library's CPU twin bit for bit on the launch classes of the packing family, layout
independence against `mlm_tokenize_packed` compared on the device, sharding and resuming, a sequence spanning many rows, the raw entry
points into guarded buffers, and the packed masked FlatFileDataset.  All comparisons are bit-exact."""
import ctypes

import numpy as np
import pytest

import pack_mlm_twin as twin

pytestmark = pytest.mark.gpu

MODES = ("nextfit", "stream")
CODE = {"b": 0, "h": 1, "i": 2, "q": 3, "f": 4, "d": 5}
POOLS = {"DNA4": np.frombuffer(b"ACGTACGTACGTACGTACGTNacgtn*\xff", np.uint8),
         "AMINO20": np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQRSTVWYXBZ*acd", np.uint8),
         "BYTES": np.arange(256, dtype=np.uint8)}
TYPE_PAIRS = ("bq", "qq", "hi", "fd", "ib")  # (inputs, labels): every element size is staged on each side
DRAWS = ((0.15, 0.8, 0.1), (1.0, 0.0, 1.0), (1.0, 0.0, 0.0))  # (frac, mask_prob, random_prob); frac = 1: every mapped character is selected


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _tok(bsq, key, flags):
    bos, eos, pad = flags
    return bsq.Tokenizer(key, bool(eos), bool(bos), bool(pad))


def _lut(key):
    from bioseq_amd import capi
    d = capi.make_desc(key)
    return np.frombuffer(bytes(d.lut), dtype=np.int8), int(d.nchars)


def _batch(rng, key, B, maxlen, lead=0):
    """Packed batch with empty sequences among the first ones; `lead` junk bytes in front (a misaligned base, offsets[0] > 0)."""
    lens = rng.integers(0, maxlen + 1, B).astype(np.int64)
    if B > 4:
        lens[:4] = (0, 1, 0, maxlen)
        lens[-1] = maxlen
    chars = np.concatenate([np.full(lead, ord("N"), np.uint8), rng.choice(POOLS[key], int(lens.sum())).astype(np.uint8)])
    offs = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return chars, offs + lead


def _np(t):
    return t.cpu().numpy()


# (kernel, key, B, P, maxlen, flags, lead): the launch classes of tests/test_packing_gpu.py
CASES = [
    ("k_pack_mlm_flat<perm>", "DNA4", 3000, 1024, 400, (1, 1, 1), 0),    # whole staged blocks
    ("k_pack_mlm_flat<perm>", "AMINO20", 1500, 512, 510, (1, 1, 0), 3),  # misaligned chars base, offsets[0] > 0, no padchar
    ("k_pack_mlm_flat<perm>", "DNA4", 700, 100, 98, (0, 0, 1), 1),       # P % 16 != 0: pieces cross rows
    ("k_pack_mlm_flat<perm>", "DNA4", 900, 17, 15, (1, 0, 0), 7),
    ("k_pack_mlm_flat<perm>", "DNA4", 300, 1, 1, (0, 0, 0), 0),          # one position per row, many empty sequences
    ("k_pack_mlm_flat<lut>", "BYTES", 2000, 256, 200, (1, 1, 1), 5),     # an alphabet that does not fold
    ("k_pack_mlm_flat<lut>", "BYTES", 600, 33, 31, (0, 1, 0), 2),
]


@pytest.mark.parametrize("kernel, key, B, P, maxlen, flags, lead", CASES)
def test_device_entry_equals_the_twins(gpu, bsq, kernel, key, B, P, maxlen, flags, lead):
    import torch
    from bioseq_amd import packing
    rng = np.random.default_rng(B + P)
    chars, offs = _batch(rng, key, B, maxlen, lead)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    tok = _tok(bsq, key, flags)
    lut, nchars = _lut(key)
    for mode in MODES:
        for n, (frac, mp, rp) in enumerate(DRAWS):
            kw = dict(frac=frac, mask_prob=mp, random_prob=rp, seed=17 + n, first_row=1000 * n)
            exp = twin.pack_mlm(key, flags, lut, nchars, chars, offs, P, mode, **kw)
            if frac == 1.0:
                assert (exp[1] != -100).sum() == (lut[chars[offs[0]:offs[-1]]] >= 0).sum()  # every mapped character is selected
            for pair in (TYPE_PAIRS if n == 0 else TYPE_PAIRS[n::2]):
                dc, lc = pair
                assert packing.pack_mlm_kernel_name(tok, B, exp[5], P, dc) == kernel
                got = packing.pack_mlm_tokenize_packed(tok, dch, dof, P, dc, mode=mode, label_dtype=lc, **kw)
                torch.cuda.synchronize()
                assert int(got.n_rows) == exp[5] and got.inputs.shape == got.labels.shape == (exp[5], P)
                assert np.array_equal(_np(got.starts), exp[4]), (mode, pair)
                assert _np(got.inputs).tobytes() == twin.as_dtype(exp[0], CODE[dc]).tobytes(), (mode, pair, kw, "inputs")
                assert _np(got.labels).view(twin.NP_DTYPES[CODE[lc]]).tobytes() == twin.as_dtype(exp[1], CODE[lc]).tobytes(), (mode, pair, kw, "labels")
                assert got.segment_ids.dtype == torch.int32 and np.array_equal(_np(got.segment_ids), exp[2]), (mode, pair)
                assert np.array_equal(_np(got.position_ids), exp[3]), (mode, pair)
            if n == 0:
                host = packing.pack_mlm_tokenize_host(tok, chars, offs, P, "q", mode=mode, **kw)  # the library's CPU twin says the same
                assert np.array_equal(host.inputs.astype(np.int64), exp[0]) and np.array_equal(host.labels.astype(np.int64), exp[1])
                assert np.array_equal(host.segment_ids, exp[2]) and np.array_equal(host.position_ids, exp[3])
                # without seg / pos
                got = packing.pack_mlm_tokenize_packed(tok, dch, dof, P, "h", mode=mode, segment_ids=False, position_ids=False, **kw)
                assert got.segment_ids is None and got.position_ids is None
                assert np.array_equal(_np(got.inputs), exp[0]) and np.array_equal(_np(got.labels), exp[1])


def _raw(gpu, key, flags, dch, dof, B, starts, R, P, m, dt, inputs, ldt, labels, seg, pos, stream=None):
    from bioseq_amd import capi
    L = capi.load()
    bos, eos, pad = flags
    d = capi.make_desc(key, eos=eos, bos=bos, padchar=pad)
    capi.check(L.bsq_pack_mlm_tokenize_device(ctypes.byref(d), dch.data_ptr(), dof.data_ptr(), B, starts.data_ptr(), R, P, ctypes.byref(m), dt,
                                              inputs, ldt, labels, seg, pos, stream))


def test_inputs_only_and_labels_only(gpu, bsq):
    import torch
    from bioseq_amd import capi, packing
    rng = np.random.default_rng(21)
    key, flags, B, P = "AMINO20", (1, 1, 1), 2500, 256
    chars, offs = _batch(rng, key, B, 250, lead=1)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    tok = _tok(bsq, key, flags)
    lut, nchars = _lut(key)
    for mode in MODES:
        exp = twin.pack_mlm(key, flags, lut, nchars, chars, offs, P, mode, frac=0.3, seed=8, first_row=2)
        starts = _dev(exp[4], gpu)
        R = exp[5]
        m = capi.Mlm(0.3, 0.8, 0.1, tok.alphabet_size(), -100, 8, 2)
        ins = torch.full((R, P), -7, dtype=torch.int64, device=gpu)
        labs = torch.full((R, P), -7, dtype=torch.int16, device=gpu)
        seg = torch.full((R, P), -7, dtype=torch.int32, device=gpu)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _raw(gpu, key, flags, dch, dof, B, starts, R, P, m, capi.U64, ins.data_ptr(), capi.I16, None, seg.data_ptr(), None, stream)
        torch.cuda.synchronize()
        assert np.array_equal(_np(ins), exp[0]) and bool((labs == -7).all()) and np.array_equal(_np(seg), exp[2])
        ins.fill_(-7)
        _raw(gpu, key, flags, dch, dof, B, starts, R, P, m, capi.U64, None, capi.I16, labs.data_ptr(), None, None, stream)
        torch.cuda.synchronize()
        assert np.array_equal(_np(labs), exp[1]) and bool((ins == -7).all())


@pytest.mark.parametrize("mode, P", [("nextfit", 1024), ("stream", 1024), ("nextfit", 2048)])
def test_layout_independence_on_the_device(gpu, bsq, mode, P):
    """20 000 sequences: the run of sequence i of the packed masked batch equals the live head of row i of `mlm_tokenize_packed`
    (padlen 1024, the same seed), inputs and labels; positions outside every run hold PAD / ignore_index / 0 / 0."""
    import torch
    from bioseq_amd import masking, packing, synth
    B = 20000
    tok = _tok(bsq, "AMINO20", (1, 1, 1))
    chars, offs = synth.synth_packed(78, B, 0, 1022, "ACDEFGHIKLMNPQRSTVWYX")
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    kw = dict(frac=0.15, seed=123456789, first_row=37)
    got = packing.pack_mlm_tokenize_packed(tok, dch, dof, P, "b", mode=mode, **kw)
    pin, plab = masking.mlm_tokenize_packed(tok, dch, dof, 1024, "b", True, **kw)
    w = (dof[1:] - dof[:-1] + 2)
    j = torch.arange(1024, device=gpu)[None, :]
    live = j < w[:, None]
    at = (got.starts[:-1, None] + j)[live]
    fin, flab = got.inputs.reshape(-1), got.labels.reshape(-1)
    assert torch.equal(fin[at], pin[live]) and torch.equal(flab[at], plab[live])
    assert int((flab != -100).sum()) > 0.1 * int((w - 2).sum())
    covered = torch.zeros(fin.numel(), dtype=torch.bool, device=gpu)
    covered[at] = True
    assert int(covered.sum()) == int(w.sum())
    out = ~covered
    assert bool((fin[out] == tok.pad()).all()) and bool((flab[out] == -100).all())
    assert bool((got.segment_ids.reshape(-1)[out] == 0).all()) and bool((got.position_ids.reshape(-1)[out] == 0).all())
    plain = packing.pack_tokenize_packed(tok, dch, dof, P, "b", mode=mode)
    assert torch.equal(plain.segment_ids, got.segment_ids) and torch.equal(plain.position_ids, got.position_ids)
    assert torch.equal(plain.starts, got.starts)


@pytest.mark.parametrize("mode", MODES)
def test_sharding_and_resuming(gpu, bsq, mode):
    import torch
    from bioseq_amd import packing
    rng = np.random.default_rng(6)
    key, flags, B, P = "AMINO20", (1, 1, 1), 4000, 512
    tok = _tok(bsq, key, flags)
    chars, offs = _batch(rng, key, B, 500)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    kw = dict(frac=0.2, seed=5)
    whole = packing.pack_mlm_tokenize_packed(tok, dch, dof, P, "i", mode=mode, **kw)
    w = np.diff(offs) + 2
    ws, wi, wl = _np(whole.starts), _np(whole.inputs).reshape(-1), _np(whole.labels).reshape(-1)

    def same_runs(part, i0, n):
        ps, pi, pl = _np(part.starts), _np(part.inputs).reshape(-1), _np(part.labels).reshape(-1)
        for k in range(n):
            a, b, wk = int(ws[i0 + k]), int(ps[k]), int(w[i0 + k])
            assert b >= 0 and np.array_equal(wi[a:a + wk], pi[b:b + wk]) and np.array_equal(wl[a:a + wk], pl[b:b + wk]), (i0, k)

    half = B // 2
    same_runs(packing.pack_mlm_tokenize_packed(tok, dch, dof[half:], P, "i", mode=mode, first_row=half, **kw), half, B - half)
    need = int(whole.n_rows)
    head = packing.pack_mlm_tokenize_packed(tok, dch, dof, P, "i", mode=mode, rows=need // 3, validate=False, **kw)
    k = int(head.n_placed)
    assert 0 < k < B and bool((head.starts[k:-1] == -1).all())
    same_runs(head, 0, k)
    same_runs(packing.pack_mlm_tokenize_packed(tok, dch, dof[k:], P, "i", mode=mode, first_row=k, **kw), k, B - k)


def test_a_sequence_spanning_many_rows_and_empty_batches(gpu, bsq):
    import torch
    from bioseq_amd import packing
    rng = np.random.default_rng(8)
    flags = (1, 1, 1)
    tok = _tok(bsq, "DNA4", flags)
    lut, nchars = _lut("DNA4")
    seqs = [5000, 0, 3, 40000, 0, 0, 17]
    chars = rng.choice(POOLS["DNA4"], sum(seqs)).astype(np.uint8)
    offs = np.concatenate([[0], np.cumsum(seqs)]).astype(np.int64)
    for frac in (0.15, 1.0):
        got = packing.pack_mlm_tokenize_packed(tok, _dev(chars, gpu), _dev(offs, gpu), 1024, "h", mode="stream", frac=frac, seed=3, first_row=9)
        exp = twin.pack_mlm("DNA4", flags, lut, nchars, chars, offs, 1024, "stream", frac=frac, seed=3, first_row=9)
        assert int(got.n_rows) == exp[5] == -(-(sum(seqs) + 14) // 1024)
        assert np.array_equal(_np(got.inputs), exp[0]) and np.array_equal(_np(got.labels), exp[1])
        assert np.array_equal(_np(got.segment_ids), exp[2]) and np.array_equal(_np(got.position_ids), exp[3])
    zeros = torch.zeros(8, dtype=torch.int64, device=gpu)
    none = torch.zeros(0, dtype=torch.uint8, device=gpu)
    for mode in MODES:
        for fl in ((1, 1, 1), (0, 0, 0)):
            r = packing.pack_mlm_tokenize_packed(_tok(bsq, "DNA4", fl), none, zeros, 4, "b", mode=mode, frac=1.0)
            e = twin.pack_mlm("DNA4", fl, lut, nchars, np.zeros(0, np.uint8), np.zeros(8, np.int64), 4, mode, frac=1.0)
            assert int(r.n_rows) == e[5] and np.array_equal(_np(r.inputs), e[0]) and np.array_equal(_np(r.labels), e[1])
            assert np.array_equal(_np(r.segment_ids), e[2]) and np.array_equal(_np(r.starts), e[4])
        r = packing.pack_mlm_tokenize_packed(tok, none, zeros[:1], 4, mode=mode)
        assert r.inputs.shape == (0, 4) and r.labels.shape == (0, 4) and int(r.n_rows) == 0 and r.starts.cpu().tolist() == [0]
        r = packing.pack_mlm_tokenize_packed(tok, none, zeros[:1], 4, mode=mode, rows=3)  # B = 0 in a fixed matrix: all PAD
        assert bool((r.inputs == tok.pad()).all()) and bool((r.labels == -100).all()) and bool((r.segment_ids == 0).all())
        assert int(r.n_placed) == 0


def test_guard_elements_a_side_stream_and_a_second_call_on_the_same_buffers(gpu, bsq):
    import torch
    from bioseq_amd import capi
    rng = np.random.default_rng(5)
    key, flags, B = "DNA4", (1, 1, 1), 1234
    chars, offs = _batch(rng, key, B, 90, lead=9)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    lut, nchars = _lut(key)
    side = torch.cuda.Stream(device=gpu)
    m = capi.Mlm(0.25, 0.8, 0.1, 7, -100, 77, 3)
    for mode, P in (("nextfit", 96), ("stream", 96), ("nextfit", 37), ("stream", 1000)):
        exp = twin.pack_mlm(key, flags, lut, nchars, chars, offs, P, mode, frac=0.25, mask_token=7, seed=77, first_row=3)
        R = exp[5]
        n = R * P
        G = 256
        ibuf = torch.full((n + 2 * G,), -77, dtype=torch.int16, device=gpu)
        lbuf = torch.full((n + 2 * G,), -77, dtype=torch.int64, device=gpu)
        sbuf = torch.full((n + 2 * G,), -77, dtype=torch.int32, device=gpu)
        pbuf = torch.full((n + 2 * G,), -77, dtype=torch.int32, device=gpu)
        starts = _dev(exp[4], gpu)
        side.wait_stream(torch.cuda.current_stream())
        stream = ctypes.c_void_p(side.cuda_stream)
        for _ in range(2):
            _raw(gpu, key, flags, dch, dof, B, starts, R, P, m, capi.I16, ibuf.data_ptr() + 2 * G, capi.U64, lbuf.data_ptr() + 8 * G,
                 sbuf.data_ptr() + 4 * G, pbuf.data_ptr() + 4 * G, stream)
            side.synchronize()
            for buf, want in ((ibuf, exp[0]), (lbuf, exp[1]), (sbuf, exp[2]), (pbuf, exp[3])):
                raw = _np(buf)
                assert (raw[:G] == -77).all() and (raw[G + n:] == -77).all(), "a guard element was overwritten"
                assert np.array_equal(raw[G:G + n].reshape(R, P), want), (mode, P)


def test_packed_masked_dataset_epochs(gpu, bsq, tmp_path):
    import torch
    from bioseq_amd.flatfile import FlatFile, write_flatfile
    from bioseq_amd.loaders import FlatFileDataset
    import views_twin
    rng = np.random.default_rng(2)
    lens = rng.integers(0, 300, 1000)
    lens[:3] = (0, 5, 700)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGTACGTACGTNacgtRY", np.uint8), int(n))) for n in lens]
    ff = FlatFile(write_flatfile(seqs, str(tmp_path / "packmlm.ff")))
    flags = (1, 1, 1)
    tok = _tok(bsq, "DNA4", flags)
    lut, nchars = _lut("DNA4")
    for mode, crop in (("nextfit", None), ("stream", None), ("nextfit", 256), ("stream", 256)):
        def epoch(ds=None, **opts):
            ds = ds or FlatFileDataset(ff, tok, device=gpu, pack=mode, pack_mlm=True, crop=crop, token_dtype="i", maskfrac=0.2)
            g = torch.Generator(device=gpu).manual_seed(5)
            out = [tuple(t.clone() for t in b) for b in ds.batches(128, generator=g, **opts)]
            torch.cuda.synchronize()
            return ds, out

        ds, base = epoch()
        width = (crop if crop else 700) + 2
        assert ds.max_seq_len == width and len(base) == 8
        g = torch.Generator(device=gpu).manual_seed(5)
        order = torch.randperm(len(ff), device=gpu, generator=g).cpu().numpy()
        if crop:
            key = (13 * 0xC2B2AE3D27D4EB4F + 1) & (2 ** 64 - 1)  # the dataset's first view key (seed 13)
            starts, lengths, strand = views_twin.plan(ff._offsets, crop, order, mode="random", revcomp_frac=0.0, seed=key, first_row=0)
            e_chars, e_offs = views_twin.apply(np.asarray(ff._chars), ff._offsets, order, starts, lengths, strand)
        else:
            e_chars = np.frombuffer(b"".join(seqs[i] for i in order), np.uint8)
            e_offs = np.concatenate([[0], np.cumsum([len(seqs[i]) for i in order])]).astype(np.int64)
        mask_key = (13 * 0x9E3779B97F4A7C15 + 1) & (2 ** 64 - 1)  # the dataset's first mask key (seed 13)
        for k, batch in enumerate(base):
            assert len(batch) == 4
            inputs, labels, seg, pos = batch
            o = e_offs[k * 128:(k + 1) * 128 + 1]
            exp = twin.pack_mlm("DNA4", flags, lut, nchars, e_chars, o, width, mode, frac=0.2, seed=mask_key, first_row=k * 128)
            assert inputs.dtype == torch.int32 and labels.dtype == torch.int64 and inputs.shape == (exp[5], width)
            assert np.array_equal(_np(inputs), exp[0]) and np.array_equal(_np(labels), exp[1]), (mode, crop, k)
            assert np.array_equal(_np(seg), exp[2]) and np.array_equal(_np(pos), exp[3])
        _, got = epoch(prefetch=2)
        assert len(got) == len(base) and all(torch.equal(x, y) for a, b in zip(base, got) for x, y in zip(a, b)), (mode, crop)
        if not crop:  # a second epoch of the same dataset draws other masks over the same packing
            _, again = epoch(ds)
            assert all(torch.equal(a[2], b[2]) for a, b in zip(base, again))
            assert any(not torch.equal(a[1], b[1]) for a, b in zip(base, again))
        t4 = ds.get_batch(0, 10)
        assert len(t4) == 4 and t4[0].shape == t4[1].shape == t4[2].shape == t4[3].shape and t4[0].shape[1] == width
        assert len(ds.__getitems__([5, 1, 7])) == 4
