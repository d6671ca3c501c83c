"""GPU: sequence packing (bioseq_amd.packing, bsq_pack_plan_device / bsq_pack_tokenize_device) against the numpy twin
(tests/pack_twin.py) and the library's CPU twins bit for bit, on both launch classes of the family, the rows = N form without a
read-back, the unpack identity at a 262 144-sequence batch compared on the device, validation, and the packed FlatFileDataset."""
import ctypes

import numpy as np
import pytest

import pack_twin as twin

pytestmark = pytest.mark.gpu

MODES = ("nextfit", "stream")
NP_OF = {"b": np.int8, "h": np.int16, "i": np.int32, "q": np.int64, "f": np.float32, "d": np.float64}
POOLS = {"DNA4": np.frombuffer(b"ACGTACGTACGTACGTACGTNacgtn*\xff", np.uint8),
         "AMINO20": np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQRSTVWYXBZ*acd", np.uint8),
         "BYTES": np.arange(256, dtype=np.uint8)}


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _tok(bsq, key, flags):
    bos, eos, pad = flags
    return bsq.Tokenizer(key, bool(eos), bool(bos), bool(pad))


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


# (kernel, key, B, P, maxlen, flags, destchars, lead)
CASES = [
    ("k_pack_flat<perm>", "DNA4", 3000, 1024, 400, (1, 1, 1), "bhiqfd", 0),     # whole blocks: staged stores of every element size
    ("k_pack_flat<perm>", "AMINO20", 1500, 512, 510, (1, 1, 0), "bq", 3),       # misaligned chars base, offsets[0] > 0, no padchar
    ("k_pack_flat<perm>", "DNA4", 700, 100, 98, (0, 0, 1), "bhiqfd", 1),        # P % 16 != 0: pieces cross rows
    ("k_pack_flat<perm>", "DNA4", 900, 17, 15, (1, 0, 0), "bq", 7),
    ("k_pack_flat<perm>", "DNA4", 300, 1, 1, (0, 0, 0), "bi", 0),               # one position per row, many empty sequences
    ("k_pack_flat<lut>", "BYTES", 2000, 256, 200, (1, 1, 1), "hiqfd", 5),       # ids up to 130: an alphabet that does not fold
    ("k_pack_flat<lut>", "BYTES", 600, 33, 31, (0, 1, 0), "hq", 2),
]


@pytest.mark.parametrize("kernel, key, B, P, maxlen, flags, destchars, lead", CASES)
def test_device_plan_and_encode_equal_the_twins(gpu, bsq, kernel, key, B, P, maxlen, flags, destchars, lead):
    import torch
    from bioseq_amd import packing
    rng = np.random.default_rng(B + P)
    chars, offs = _batch(rng, key, B, maxlen, lead)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    if lead % 16:
        assert dch.data_ptr() % 16 == 0 and (dch.data_ptr() + int(offs[0])) % 16 != 0
    tok = _tok(bsq, key, flags)
    for mode in MODES:
        exp = twin.pack(key, flags, chars, offs, P, mode)
        for dc in destchars:
            assert packing.pack_kernel_name(tok, B, exp[4], P, dc) == kernel
            for want_seg, want_pos in ((True, True), (False, True), (True, False), (False, False)) if dc == destchars[0] else ((True, True),):
                got = packing.pack_tokenize_packed(tok, dch, dof, P, dc, mode=mode, segment_ids=want_seg, position_ids=want_pos)
                torch.cuda.synchronize()
                assert int(got.n_rows) == exp[4] and got.tokens.shape == (exp[4], P) and got.tokens.is_contiguous()
                assert np.array_equal(got.starts.cpu().numpy(), exp[3]), (mode, dc)
                assert got.tokens.cpu().numpy().tobytes() == exp[0].astype(NP_OF[dc]).tobytes(), (mode, dc)
                assert (got.segment_ids is None) == (not want_seg) and (got.position_ids is None) == (not want_pos)
                if want_seg:
                    assert got.segment_ids.dtype == torch.int32 and np.array_equal(got.segment_ids.cpu().numpy(), exp[1]), (mode, dc)
                if want_pos:
                    assert np.array_equal(got.position_ids.cpu().numpy(), exp[2]), (mode, dc)
            host = packing.pack_tokenize_host(tok, chars, offs, P, dc, mode=mode)  # the library's CPU twin says the same
            assert host.tokens.tobytes() == exp[0].astype(NP_OF[dc]).tobytes() and np.array_equal(host.segment_ids, exp[1])


def test_a_single_sequence_spanning_many_rows_and_all_empty_batches(gpu, bsq):
    import torch
    from bioseq_amd import packing
    rng = np.random.default_rng(8)
    tok = _tok(bsq, "DNA4", (1, 1, 1))
    seqs = [5000, 0, 3, 40000, 0, 0, 17]
    chars = rng.choice(POOLS["DNA4"], sum(seqs)).astype(np.uint8)
    offs = np.concatenate([[0], np.cumsum(seqs)]).astype(np.int64)
    got = packing.pack_tokenize_packed(tok, _dev(chars, gpu), _dev(offs, gpu), 1024, "h", mode="stream")
    exp = twin.pack("DNA4", (1, 1, 1), chars, offs, 1024, "stream", dtype=np.int16)
    torch.cuda.synchronize()
    assert int(got.n_rows) == exp[4] == -(-(sum(seqs) + 14) // 1024)
    assert np.array_equal(got.tokens.cpu().numpy(), exp[0]) and np.array_equal(got.segment_ids.cpu().numpy(), exp[1])
    assert np.array_equal(got.position_ids.cpu().numpy(), exp[2]) and int(got.position_ids.max()) == 40001
    assert np.array_equal(packing.pack_cu_seqlens(got.starts).cpu().numpy(), exp[3].astype(np.int32))
    zeros = torch.zeros(8, dtype=torch.int64, device=gpu)
    for mode in MODES:
        for flags in ((1, 1, 1), (0, 0, 0)):
            r = packing.pack_tokenize_packed(_tok(bsq, "DNA4", flags), torch.zeros(0, dtype=torch.uint8, device=gpu), zeros, 4, "b", mode=mode)
            e = twin.pack("DNA4", flags, np.zeros(0, np.uint8), np.zeros(8, np.int64), 4, mode, dtype=np.int8)
            assert int(r.n_rows) == e[4] and np.array_equal(r.tokens.cpu().numpy(), e[0]) and np.array_equal(r.segment_ids.cpu().numpy(), e[1])
            assert np.array_equal(r.starts.cpu().numpy(), e[3])
        none = packing.pack_tokenize_packed(tok, torch.zeros(0, dtype=torch.uint8, device=gpu), zeros[:1], 4, mode=mode)
        assert none.tokens.shape == (0, 4) and int(none.n_rows) == 0 and none.starts.cpu().tolist() == [0]


def test_guard_bytes_a_side_stream_and_a_second_call_on_the_same_buffers(gpu, bsq):
    """The raw entry points into the middle of guarded buffers on a non-default stream; the same call again over the same buffers."""
    import torch
    from bioseq_amd import capi
    L = capi.load()
    rng = np.random.default_rng(5)
    B = 1234
    chars, offs = _batch(rng, "DNA4", B, 90, lead=9)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    d = capi.make_desc("DNA4", eos=True, bos=True, padchar=True)
    side = torch.cuda.Stream(device=gpu)
    for mode, P in (("nextfit", 96), ("stream", 96), ("nextfit", 37), ("stream", 1000)):
        exp = twin.pack("DNA4", (1, 1, 1), chars, offs, P, mode, dtype=np.int16)
        R = exp[4]
        n = R * P
        G = 256
        tbuf = torch.full((n + 2 * G,), -77, dtype=torch.int16, device=gpu)
        sbuf = torch.full((n + 2 * G,), -77, dtype=torch.int32, device=gpu)
        pbuf = torch.full((n + 2 * G,), -77, dtype=torch.int32, device=gpu)
        plan = torch.full((B + 1 + 2 * G,), -77, dtype=torch.int64, device=gpu)
        counts = torch.full((2 + 2 * G,), -77, dtype=torch.int64, device=gpu)
        side.wait_stream(torch.cuda.current_stream())
        stream = ctypes.c_void_p(side.cuda_stream)
        for _ in range(2):
            capi.check(L.bsq_pack_plan_device(dof.data_ptr(), B, P, 1, 1, capi.PACK_NEXTFIT if mode == "nextfit" else capi.PACK_STREAM, 0,
                                              plan.data_ptr() + 8 * G, counts.data_ptr() + 8 * G, counts.data_ptr() + 8 * G + 8, stream))
            capi.check(L.bsq_pack_tokenize_device(ctypes.byref(d), dch.data_ptr(), dof.data_ptr(), B, plan.data_ptr() + 8 * G, R, P, capi.I16,
                                                  tbuf.data_ptr() + 2 * G, sbuf.data_ptr() + 4 * G, pbuf.data_ptr() + 4 * G, stream))
            side.synchronize()
            for buf, want in ((tbuf, exp[0]), (sbuf, exp[1]), (pbuf, exp[2])):
                raw = buf.cpu().numpy()
                assert (raw[:G] == -77).all() and (raw[G + n:] == -77).all(), "a guard element was overwritten"
                assert np.array_equal(raw[G:G + n].reshape(R, P), want), (mode, P)
            raw = plan.cpu().numpy()
            assert (raw[:G] == -77).all() and (raw[G + B + 1:] == -77).all() and np.array_equal(raw[G:G + B + 1], exp[3])
            raw = counts.cpu().numpy()
            assert (raw[:G] == -77).all() and (raw[G + 2:] == -77).all() and raw[G:G + 2].tolist() == [R, B]


@pytest.mark.parametrize("mode", MODES)
def test_rows_n_without_a_read_back(gpu, bsq, mode):
    import torch
    from bioseq_amd import packing
    rng = np.random.default_rng(4)
    flags = (1, 1, 1)
    tok = _tok(bsq, "AMINO20", flags)
    chars, offs = _batch(rng, "AMINO20", 5000, 500)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    P = 512
    need = twin.plan(offs, P, 1, 1, mode)[1]
    bound = packing.pack_rows_bound(int(offs[-1] - offs[0]), 5000, P, tok, mode)
    assert bound >= need
    for N in (need // 3, need, bound):
        got = packing.pack_tokenize_packed(tok, dch, dof, P, "i", mode=mode, rows=N, validate=False)
        exp = twin.pack("AMINO20", flags, chars, offs, P, mode, rows=N, dtype=np.int32)
        torch.cuda.synchronize()
        assert got.tokens.shape == (N, P) and int(got.n_rows) == need and int(got.n_placed) == exp[5]
        assert np.array_equal(got.starts.cpu().numpy(), exp[3])
        assert np.array_equal(got.tokens.cpu().numpy(), exp[0]) and np.array_equal(got.segment_ids.cpu().numpy(), exp[1])
        assert np.array_equal(got.position_ids.cpu().numpy(), exp[2])
        assert (exp[5] == 5000) == (N >= need)
    # resuming at n_placed packs the rest
    k = twin.plan(offs, P, 1, 1, mode, need // 3)[2]
    rest = packing.pack_tokenize_packed(tok, dch, dof[k:], P, "i", mode=mode)
    exp = twin.pack("AMINO20", flags, chars, offs[k:], P, mode, dtype=np.int32)
    assert np.array_equal(rest.tokens.cpu().numpy(), exp[0])
    plan = packing.pack_plan(tok, dch, dof, P, mode=mode)
    assert int(plan[1]) == need and int(plan[2]) == 5000


@pytest.mark.parametrize("mode, P", [("nextfit", 1024), ("stream", 1024), ("nextfit", 2048)])
def test_unpack_identity_at_a_baseline_sized_batch(gpu, bsq, mode, P):
    """262 144 sequences: every run of the packed matrix equals the head of its row in `tokenize_packed` of the same batch, position
    ids count inside the run and the positions outside every run hold PAD -- compared on the device; the plan equals the CPU loop."""
    import torch
    from bioseq_amd import packing, synth
    B = 262144
    tok = _tok(bsq, "AMINO20", (1, 1, 1))
    chars, offs = synth.synth_packed(77, B, 0, 1022, "ACDEFGHIKLMNPQRSTVWY")
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    got = packing.pack_tokenize_packed(tok, dch, dof, P, "b", mode=mode)
    plan = packing.pack_plan_host(tok, offs, P, mode)
    assert int(got.n_rows) == plan[1] and torch.equal(got.starts, _dev(plan[0], gpu))
    padded = tok.tokenize_packed(dch, dof, 1024, "b", True)
    w = (dof[1:] - dof[:-1] + 2)
    j = torch.arange(1024, device=gpu)[None, :]
    live = j < w[:, None]
    at = (got.starts[:-1, None] + j)[live]
    flat, fpos, fseg = got.tokens.reshape(-1), got.position_ids.reshape(-1), got.segment_ids.reshape(-1)
    assert torch.equal(flat[at], padded[live])
    assert torch.equal(fpos[at], j.expand(B, 1024)[live].to(torch.int32))
    covered = torch.zeros(flat.numel(), dtype=torch.bool, device=gpu)
    covered[at] = True
    assert int(covered.sum()) == int(w.sum())
    pad = bsq.Tokenizer("AMINO20", True, True, True).pad()
    assert bool((flat[~covered] == pad).all()) and bool((fseg[~covered] == 0).all()) and bool((fpos[~covered] == 0).all())
    assert bool((fseg[covered] >= 1).all())
    if mode == "nextfit":
        s = got.starts[:-1]
        assert bool(((s // P) == ((s + w - 1) // P)).all())
        seq_of = torch.repeat_interleave(torch.arange(B, device=gpu), w)
        first = torch.full((int(got.n_rows),), B, dtype=torch.int64, device=gpu).scatter_reduce(0, s // P, torch.arange(B, device=gpu), "amin")
        assert torch.equal(fseg[at].to(torch.int64), 1 + seq_of - first[at // P])


def test_validation_errors_name_the_sequence(gpu, bsq):
    import torch
    from bioseq_amd import packing
    tok = _tok(bsq, "DNA4", (1, 1, 1))
    lens = [10, 20, 63, 5]
    chars = np.full(sum(lens), ord("A"), np.uint8)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    with pytest.raises(RuntimeError, match="sequence 2"):
        packing.pack_tokenize_packed(tok, dch, dof, 64)  # 63 + 2 > 64
    assert packing.pack_tokenize_packed(tok, dch, dof, 65).tokens.shape == (3, 65)  # 12 + 22 | 65 | 7
    assert packing.pack_tokenize_packed(tok, dch, dof, 64, mode="stream").tokens.shape == (2, 64)  # a stream has no width to exceed
    cut = packing.pack_tokenize_packed(tok, dch, dof, 64, "i", validate=False)  # (cut at 64 positions, a row of its own)
    exp = twin.pack("DNA4", (1, 1, 1), chars, offs, 64, "nextfit", dtype=np.int32)
    assert np.array_equal(cut.tokens.cpu().numpy(), exp[0]) and np.array_equal(cut.segment_ids.cpu().numpy(), exp[1])
    bad = dof.clone()
    bad[2] = bad[1] - 1
    for mode in MODES:
        with pytest.raises(RuntimeError, match="malformed offsets"):
            packing.pack_tokenize_packed(tok, dch, bad, 128, mode=mode)
        with pytest.raises(RuntimeError):
            packing.pack_plan(tok, dch, bad, 128, mode=mode)


def test_packed_dataset_epochs(gpu, bsq, tmp_path):
    import torch
    from bioseq_amd.flatfile import FlatFile, write_flatfile
    from bioseq_amd.loaders import FlatFileDataset
    import views_twin
    rng = np.random.default_rng(2)
    lens = rng.integers(0, 300, 1000)
    lens[:3] = (0, 5, 700)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGTACGTACGTNacgtRY", np.uint8), int(n))) for n in lens]
    ff = FlatFile(write_flatfile(seqs, str(tmp_path / "pack.ff")))
    flags = (1, 1, 1)
    tok = _tok(bsq, "DNA4", flags)
    for mode, crop in (("nextfit", None), ("stream", None), ("nextfit", 256), ("stream", 256)):
        def epoch(**opts):
            ds = FlatFileDataset(ff, tok, device=gpu, pack=mode, crop=crop, token_dtype="i")
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
        for k, (tokens, seg, pos) in enumerate(base):
            o = e_offs[k * 128:(k + 1) * 128 + 1]
            exp = twin.pack("DNA4", flags, e_chars, o, width, mode, dtype=np.int32)
            assert tokens.dtype == torch.int32 and tokens.shape == (exp[4], width)
            assert np.array_equal(tokens.cpu().numpy(), exp[0]) and np.array_equal(seg.cpu().numpy(), exp[1]), (mode, crop, k)
            assert np.array_equal(pos.cpu().numpy(), exp[2])
        _, got = epoch(prefetch=2)
        assert len(got) == len(base) and all(torch.equal(x, y) for a, b in zip(base, got) for x, y in zip(a, b)), (mode, crop)
        with pytest.raises(ValueError):
            next(iter(ds.batches(128, group=2)))
        # the other access paths hand out the same triple
        t3 = ds.get_batch(0, 10)
        exp = twin.pack("DNA4", flags, *_first(ff, seqs, 10, crop), width, mode, dtype=np.int32) if not crop else None
        assert len(t3) == 3 and t3[0].shape[1] == width and t3[0].shape == t3[1].shape == t3[2].shape
        if exp is not None:
            assert np.array_equal(t3[0].cpu().numpy(), exp[0])
        assert len(ds.__getitems__([5, 1, 7])) == 3


def _first(ff, seqs, n, crop):
    chars = np.frombuffer(b"".join(seqs[:n]), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs[:n]])]).astype(np.int64)
    return chars, offs
