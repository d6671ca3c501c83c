"""GPU: views of packed stores (bioseq_amd.views, bsq_crop_packed_device / bsq_views_packed_device) against the numpy twin's plan
applied in numpy (tests/views_twin.py), the encodes of cropped batches against the oracle, and the cropping FlatFileDataset."""
import ctypes

import numpy as np
import pytest

import views_twin as twin

pytestmark = pytest.mark.gpu

GUARD = 256
POOL = np.frombuffer(b"ACGTNacgtnRYKMBVDHSWxX*-.\x00\xff\x80@[`{", dtype=np.uint8)


def _store(rng, n, maxlen, empties=True):
    lens = rng.integers(0, maxlen + 1, n).astype(np.int64)
    if empties and n > 3:
        lens[:3] = 0
    chars = rng.choice(POOL, int(lens.sum())).astype(np.uint8)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return chars, offs


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _raw_crop(gpu, chars, offs, index, n, c, capacity, stream=None):
    """bsq_crop_packed_device into guarded buffers; returns (chars, offsets, starts, strand, status) on the host and checks the guards."""
    import torch
    from bioseq_amd import capi
    L = capi.load()
    dch = _dev(chars if chars.size else np.zeros(16, np.uint8), gpu)
    dof = _dev(offs, gpu)
    didx = _dev(index, gpu) if index is not None else None
    buf = torch.full((capacity + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    out_offs = torch.full((n + 1,), -7, dtype=torch.int64, device=gpu)
    starts = torch.full((max(n, 1),), -7, dtype=torch.int64, device=gpu)
    strand = torch.full((max(n, 1),), 9, dtype=torch.uint8, device=gpu)
    status = torch.zeros(1, dtype=torch.int64, device=gpu)
    s = stream.cuda_stream if stream is not None else capi.raw_stream(gpu)
    capi.check(L.bsq_crop_packed_device(dch.data_ptr(), dof.data_ptr(), len(offs) - 1, didx.data_ptr() if didx is not None else None, n,
                                        ctypes.byref(c), buf.data_ptr() + GUARD, capacity, out_offs.data_ptr(), starts.data_ptr(),
                                        strand.data_ptr(), status.data_ptr(), ctypes.c_void_p(s)))
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + capacity:] == 0xA5).all(), "a guard byte of out_chars was overwritten"
    return raw[GUARD:GUARD + capacity], out_offs.cpu().numpy(), starts.cpu().numpy()[:n], strand.cpu().numpy()[:n], int(status.item())


@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 100000])
@pytest.mark.parametrize("window, mode, frac", [(64, "random", 0.5), (1024, "center", 0.0), (17, "head", 1.0), (0, "random", 0.3)])
def test_crop_device_equals_twin(gpu, n, window, mode, frac):
    from bioseq_amd import capi
    rng = np.random.default_rng(n + window)
    chars, offs = _store(rng, 3000, 2500)
    index = rng.integers(0, 3000, n).astype(np.int64)  # repeats included
    seed, first_row = int(rng.integers(0, 2 ** 62)), int(rng.integers(0, 1000))
    c = capi.Crop(window, twin.MODES[mode], frac, seed, first_row)
    e_chars, e_offs, e_starts, e_strand = twin.crop(chars, offs, window, index, mode=mode, revcomp_frac=frac, seed=seed, first_row=first_row)
    cap = int(e_offs[-1])
    got_chars, got_offs, got_starts, got_strand, status = _raw_crop(gpu, chars, offs, index, n, c, cap)
    assert status == -1
    assert np.array_equal(got_offs, e_offs)
    assert got_chars.tobytes() == e_chars.tobytes()
    assert np.array_equal(got_starts, e_starts) and np.array_equal(got_strand, e_strand)


def test_scanned_place_beyond_2_pow_20_rows(gpu):
    """The class beyond 2^20 rows (k_views_lengths2 + k_views_scan + k_views_place<SCANNED>): 2^20 + 65 rows of 0 .. 3 characters, so the
    last workgroup is partial and the last entry of the scanned sums is the sum of one row.  Crops and explicit views of the same rows,
    bit for bit against the library's host plan applied in numpy."""
    from bioseq_amd import views
    n = 2 ** 20 + 65
    rng = np.random.default_rng(20)
    lens = np.arange(n, dtype=np.int64) % 4
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(offs[-1]))
    chars[rng.random(chars.size) < 0.01] = ord("N")
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    opts = dict(mode="head", revcomp_frac=0.5, seed=17)
    starts, vlen, strand = views.crop_plan(offs, 2, **opts)
    assert np.array_equal(vlen, np.minimum(lens, 2)) and not starts.any() and 0.4 < strand.mean() < 0.6
    e_offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(vlen, out=e_offs[1:])
    row = np.repeat(np.arange(n), vlen)
    k = np.arange(int(e_offs[-1])) - e_offs[row]  # position in the row
    rc = strand[row] != 0
    e_chars = chars[offs[row] + starts[row] + np.where(rc, vlen[row] - 1 - k, k)]
    e_chars[rc] = twin.COMP[e_chars[rc]]
    got_c, got_o, got_st, got_sd = views.crop_packed(dch, dof, 2, return_origin=True, **opts)
    assert np.array_equal(got_o.cpu().numpy(), e_offs)
    assert got_c[:int(e_offs[-1])].cpu().numpy().tobytes() == e_chars.tobytes()
    assert np.array_equal(got_st.cpu().numpy(), starts) and np.array_equal(got_sd.cpu().numpy(), strand)
    got_c, got_o = views.gather_views(dch, dof, np.arange(n), starts, vlen, strand)
    assert np.array_equal(got_o.cpu().numpy(), e_offs)
    assert got_c[:int(e_offs[-1])].cpu().numpy().tobytes() == e_chars.tobytes()


@pytest.mark.parametrize("n", [5, 3000])
def test_crop_without_index_bad_indices_and_overflow(gpu, n):
    from bioseq_amd import capi
    rng = np.random.default_rng(n)
    chars, offs = _store(rng, 3000, 600)
    c = capi.Crop(100, 0, 0.5, 77, 0)
    # index NULL: sequences 0 .. n - 1
    e_chars, e_offs, e_starts, e_strand = twin.crop(chars, offs, 100, np.arange(n), revcomp_frac=0.5, seed=77)
    got = _raw_crop(gpu, chars, offs, None, n, c, n * 100)
    assert got[4] == -1 and np.array_equal(got[1], e_offs) and got[0][:e_offs[-1]].tobytes() == e_chars.tobytes()
    assert np.array_equal(got[2], e_starts) and np.array_equal(got[3], e_strand)
    # bad indices: empty rows, the first one reported
    index = rng.integers(0, 3000, n).astype(np.int64)
    index[n // 2] = -1
    index[-1] = 3000
    ok = index.copy()
    ok[(index < 0) | (index >= 3000)] = 0
    _, e_offs, e_starts, e_strand = twin.crop(chars, offs, 100, ok, revcomp_frac=0.5, seed=77)
    lens = np.diff(e_offs)
    lens[[n // 2, n - 1]] = 0
    got = _raw_crop(gpu, chars, offs, index, n, c, n * 100)
    assert got[4] == n // 2
    assert np.array_equal(np.diff(got[1]), lens)
    assert got[2][n // 2] == 0 and got[3][n // 2] == 0
    # overflow: the batch is cut at the capacity, nothing written past it (the guards), the first row that did not fit reported
    index = rng.integers(3, 3000, n).astype(np.int64)
    e_chars, e_offs, _, _ = twin.crop(chars, offs, 100, index, revcomp_frac=0.5, seed=77)
    cap = int(e_offs[-1]) * 2 // 3 + 5
    got = _raw_crop(gpu, chars, offs, index, n, c, cap)
    first_over = int(np.nonzero(e_offs[1:] > cap)[0][0])
    assert got[4] == n + first_over
    assert np.array_equal(got[1], e_offs)
    assert got[0].tobytes() == e_chars[:cap].tobytes()


def test_crop_side_stream_and_shards(gpu):
    import torch
    from bioseq_amd import capi
    rng = np.random.default_rng(3)
    chars, offs = _store(rng, 500, 3000)
    n = 6000
    index = rng.integers(0, 500, n).astype(np.int64)
    c = capi.Crop(256, 0, 0.5, 5, 0)
    whole = _raw_crop(gpu, chars, offs, index, n, c, n * 256)
    side = torch.cuda.Stream(device=gpu)
    alt = _raw_crop(gpu, chars, offs, index, n, c, n * 256, stream=side)
    for a, b in zip(whole[:4], alt[:4]):
        assert np.array_equal(a, b)
    pieces, cut = [], [0, 1000, 4100, n]
    for a, b in zip(cut[:-1], cut[1:]):
        pieces.append(_raw_crop(gpu, chars, offs, index[a:b], b - a, capi.Crop(256, 0, 0.5, 5, a), (b - a) * 256))
    total = int(whole[1][-1])
    assert np.concatenate([p[0][:p[1][-1]] for p in pieces]).tobytes() == whole[0][:total].tobytes()
    assert np.array_equal(np.concatenate([p[2] for p in pieces]), whole[2])
    assert np.array_equal(np.concatenate([p[3] for p in pieces]), whole[3])


@pytest.mark.parametrize("n", [7, 5000])
def test_gather_views_explicit_rows(gpu, n):
    import torch
    from bioseq_amd import capi, views
    rng = np.random.default_rng(n)
    chars, offs = _store(rng, 300, 2000)
    lens = np.diff(offs)
    seq = rng.integers(0, 300, n).astype(np.int64)
    start = (rng.random(n) * (lens[seq] + 1)).astype(np.int64)
    length = (rng.random(n) * (lens[seq] - start + 1)).astype(np.int64)
    strand = rng.integers(0, 2, n).astype(np.uint8)
    e_chars, e_offs = twin.apply(chars, offs, seq, start, length, strand)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    got_c, got_o = views.gather_views(dch, dof, seq, start, length, strand)
    assert np.array_equal(got_o.cpu().numpy(), e_offs) and got_c[:int(e_offs[-1])].cpu().numpy().tobytes() == e_chars.tobytes()
    got_c, got_o = views.gather_views(dch, dof, _dev(seq, gpu), _dev(start, gpu), _dev(length, gpu))  # device tensors, forward
    f_chars, f_offs = twin.apply(chars, offs, seq, start, length, np.zeros(n, np.uint8))
    assert np.array_equal(got_o.cpu().numpy(), f_offs) and got_c[:int(f_offs[-1])].cpu().numpy().tobytes() == f_chars.tobytes()
    # out-of-range views: empty rows, the first reported (raw ABI), IndexError with validate
    bad_start = start.copy()
    bad_start[n // 3] = lens[seq[n // 3]] + 1
    bad_len = length.copy()
    bad_len[-1] = lens[seq[-1]] - start[-1] + 1
    with pytest.raises(IndexError):
        views.gather_views(dch, dof, seq, bad_start, bad_len, strand)
    L = capi.load()
    cap = int(np.maximum(bad_len, 0).sum())
    out = torch.empty(cap + 1, dtype=torch.uint8, device=gpu)
    out_offs = torch.empty(n + 1, dtype=torch.int64, device=gpu)
    status = torch.empty(1, dtype=torch.int64, device=gpu)
    d = [_dev(a, gpu) for a in (seq, bad_start, bad_len, strand)]
    capi.check(L.bsq_views_packed_device(dch.data_ptr(), dof.data_ptr(), 300, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                         d[3].data_ptr(), n, out.data_ptr(), cap, out_offs.data_ptr(), status.data_ptr(),
                                         ctypes.c_void_p(capi.raw_stream(gpu))))
    assert int(status.item()) == n // 3
    got_lens = np.diff(out_offs.cpu().numpy())
    exp_lens = length.copy()
    exp_lens[[n // 3, n - 1]] = 0
    assert np.array_equal(got_lens, exp_lens)


def test_encodes_of_a_cropped_batch_equal_the_oracle(gpu, bsq, oracle):
    from bioseq_amd import masking, views
    rng = np.random.default_rng(11)
    chars, offs = _store(rng, 400, 3000, empties=True)
    index = rng.integers(0, 400, 300).astype(np.int64)
    window = 200
    e_chars, e_offs, _, _ = twin.crop(chars, offs, window, index, mode="random", revcomp_frac=0.5, seed=4)
    seqs = [bytes(e_chars[e_offs[i]:e_offs[i + 1]]) for i in range(len(index))]
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    vc, vo = views.crop_packed(dch, dof, window, index=_dev(index, gpu), revcomp_frac=0.5, seed=4)
    P = window + 2
    tok = bsq.Tokenizer("DNA5", True, True, True)
    ora = oracle.OracleTokenizer("DNA5", True, True, True)
    got = tok.tokenize_packed(vc, vo, P, "q", True)
    assert got.cpu().numpy().tobytes() == ora.batch_tokenize(seqs, padlen=P, destchar="q", batch_first=True).tobytes()
    got = tok.onehot_packed(vc, vo, P, "f")
    assert got.cpu().numpy().tobytes() == ora.batch_onehot_encode(seqs, padlen=P, destchar="f").tobytes()
    # masked-LM of the cropped batch equals masked-LM of the twin's views uploaded as a batch
    inp, lab = masking.mlm_tokenize_packed(tok, vc, vo, P, "q", frac=0.2, seed=8)
    inp2, lab2 = masking.mlm_tokenize_packed(tok, _dev(e_chars, gpu), _dev(e_offs, gpu), P, "q", frac=0.2, seed=8)
    assert (inp == inp2).all() and (lab == lab2).all()
    # return_origin and host index lists
    vc2, vo2, st, sd = views.crop_packed(dch, dof, window, index=list(index), revcomp_frac=0.5, seed=4, return_origin=True)
    _, _, e_st, e_sd = twin.crop(chars, offs, window, index, revcomp_frac=0.5, seed=4)
    assert np.array_equal(st.cpu().numpy(), e_st) and np.array_equal(sd.cpu().numpy(), e_sd)
    assert vc2[:int(e_offs[-1])].cpu().numpy().tobytes() == e_chars.tobytes()
    with pytest.raises(IndexError):
        views.crop_packed(dch, dof, window, index=_dev(np.array([1, 400]), gpu))


def _flatfile(tmp_path, rng, n=700):
    from bioseq_amd.flatfile import FlatFile, write_flatfile
    lens = rng.integers(0, 400, n)
    lens[5] = 5000  # one long outlier
    lens[9] = 0
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGTNacgtRY", np.uint8), L)) for L in lens]
    return FlatFile(write_flatfile(seqs, str(tmp_path / "views.ff"))), seqs


def _expected_rows(ff, order, crop, mode, frac, key, first):
    starts, lengths, strand = twin.plan(ff._offsets, crop or 0, order, mode=mode, revcomp_frac=frac, seed=key, first_row=first)
    e_chars, e_offs = twin.apply(np.asarray(ff._chars), ff._offsets, order, starts, lengths, strand)
    return [bytes(e_chars[e_offs[i]:e_offs[i + 1]]) for i in range(len(order))]


@pytest.mark.parametrize("cnn", [False, True])
@pytest.mark.parametrize("crop, frac", [(128, 0.0), (128, 0.5), (None, 1.0)])
def test_dataset_views_equal_oracle_and_group_prefetch_agree(gpu, bsq, oracle, tmp_path, cnn, crop, frac):
    import torch
    from bioseq_amd.loaders import FlatFileDataset
    rng = np.random.default_rng(2)
    ff, seqs = _flatfile(tmp_path, rng)
    tok = bsq.Tokenizer("DNA", True, True, True)
    ora = oracle.OracleTokenizer("DNA", True, True, True)

    def epoch(**opts):
        ds = FlatFileDataset(ff, tok, device=gpu, cnn=cnn, crop=crop, revcomp_frac=frac, token_dtype="q")
        g = torch.Generator(device=gpu).manual_seed(5)
        out = [b.clone() for b in ds.batches(128, generator=g, **opts)]
        torch.cuda.synchronize()
        return ds, out

    ds, base = epoch()
    width = (crop if crop else 5000) + 2
    assert ds.max_seq_len == width
    assert all(b.dim() == (3 if cnn else 2) and b.shape[-1] == width for b in base)
    g = torch.Generator(device=gpu).manual_seed(5)
    order = torch.randperm(len(ff), device=gpu, generator=g).cpu().numpy()
    key = (13 * 0xC2B2AE3D27D4EB4F + 1) & (2 ** 64 - 1)  # the dataset's first crop key (seed 13)
    rows = _expected_rows(ff, order, crop, "random", frac, key, 0)
    exp = (ora.batch_onehot_encode(rows, padlen=width, destchar="f").transpose(1, 2, 0) if cnn
           else ora.batch_tokenize(rows, padlen=width, destchar="q", batch_first=True))
    assert torch.cat(base).cpu().numpy().tobytes() == np.ascontiguousarray(exp).tobytes()
    for opts in ({"group": 4}, {"group": 4, "prefetch": 2}, {"prefetch": 2}):
        _, got = epoch(**opts)
        assert len(got) == len(base) and all(torch.equal(a, b) for a, b in zip(base, got)), opts


def test_dataset_views_every_path(gpu, bsq, oracle, tmp_path):
    import torch
    from bioseq_amd.loaders import FlatFileDataset
    rng = np.random.default_rng(3)
    ff, seqs = _flatfile(tmp_path, rng, 300)
    tok = bsq.Tokenizer("DNA", True, True, True)
    ora = oracle.OracleTokenizer("DNA", True, True, True)
    crop, width = 64, 66
    key = lambda k: (13 * 0xC2B2AE3D27D4EB4F + k) & (2 ** 64 - 1)  # noqa: E731

    ds = FlatFileDataset(ff, tok, device=gpu, crop=crop, crop_mode="center", revcomp_frac=0.5)
    got = ds.get_batch(0, 40)
    exp = ora.batch_tokenize(_expected_rows(ff, np.arange(40), crop, "center", 0.5, key(1), 0), padlen=width, destchar="q", batch_first=True)
    assert got.shape == (40, width) and got.cpu().numpy().tobytes() == exp.tobytes()
    idx = [5, 9, 5, 200, 17]
    got = ds.__getitems__(idx)
    exp = ora.batch_tokenize(_expected_rows(ff, np.array(idx), crop, "center", 0.5, key(2), 0), padlen=width, destchar="q", batch_first=True)
    assert got.cpu().numpy().tobytes() == exp.tobytes()
    got = ds.__getitems__(torch.tensor(idx, device=gpu))
    exp = ora.batch_tokenize(_expected_rows(ff, np.array(idx), crop, "center", 0.5, key(3), 0), padlen=width, destchar="q", batch_first=True)
    assert got.cpu().numpy().tobytes() == exp.tobytes()
    row = ds[5]
    exp = ora.batch_tokenize(_expected_rows(ff, np.array([5]), crop, "center", 0.5, key(4), 0), padlen=width, destchar="q", batch_first=True)
    assert row.shape == (width,) and row.cpu().numpy().tobytes() == exp[0].tobytes()
    # cnn fetch: single index (with items) and an index list
    dsc = FlatFileDataset(ff, tok, device=gpu, cnn=True, crop=crop, revcomp_frac=1.0)
    t, item = dsc.fetch(5, return_items=True)
    assert bytes(item) == _expected_rows(ff, np.array([5]), crop, "random", 1.0, key(1), 0)[0] and len(item) == crop
    t, items = dsc.fetch([5, 6, 7], return_items=True)
    assert t.shape == (3, tok.alphabet_size(), width) and [bytes(x) for x in items] == _expected_rows(ff, np.array([5, 6, 7]), crop, "random", 1.0, key(2), 0)
    # masked: the masks of a cropped dataset are drawn on the views (the mask counter is not moved by the crop)
    dsm = FlatFileDataset(ff, tok, device=gpu, masked=True, maskfrac=0.2, crop=crop)
    inp, lab = dsm.get_batch(0, 50)
    from bioseq_amd import masking
    rows = _expected_rows(ff, np.arange(50), crop, "random", 0.0, key(1), 0)
    vch = np.frombuffer(b"".join(rows), np.uint8)
    vof = np.zeros(51, np.int64)
    np.cumsum([len(r) for r in rows], out=vof[1:])
    mkey = (13 * 0x9E3779B97F4A7C15 + 1) & (2 ** 64 - 1)
    inp2, lab2 = masking.mlm_tokenize_packed(tok, _dev(vch, gpu), _dev(vof, gpu), width, "q", frac=0.2, seed=mkey)
    assert torch.equal(inp, inp2) and torch.equal(lab, lab2)
    # augmentation runs on the views, never on the store
    dsa = FlatFileDataset(ff, tok, device=gpu, crop=crop, augment=2, augment_frac=1.0)
    store = ff.to_device(gpu)[0].clone()
    assert dsa.get_batch(0, 50).shape == (50, width)
    assert torch.equal(store, ff.to_device(gpu)[0])


def test_default_dataset_is_unchanged(gpu, bsq, tmp_path):
    import torch
    from bioseq_amd.loaders import FlatFileDataset
    ff, _ = _flatfile(tmp_path, np.random.default_rng(4), 400)
    tok = bsq.Tokenizer("DNA", True, True, True)
    for cnn in (False, True):
        a = FlatFileDataset(ff, tok, device=gpu, cnn=cnn)
        b = FlatFileDataset(ff, tok, device=gpu, cnn=cnn, crop=None, revcomp_frac=0.0)
        for ga, gb in ((torch.Generator(device=gpu).manual_seed(1), torch.Generator(device=gpu).manual_seed(1)),):
            for x, y in zip(a.batches(100, generator=ga, group=2), b.batches(100, generator=gb, group=2)):
                assert torch.equal(x, y)
        assert torch.equal(a.get_batch(3, 90), b.get_batch(3, 90))
        assert torch.equal(a.__getitems__([4, 1, 4]), b.__getitems__([4, 1, 4]))


def test_flatfile_windows_device_reassembles_every_sequence(gpu, tmp_path):
    rng = np.random.default_rng(6)
    ff, seqs = _flatfile(tmp_path, rng, 200)
    for window, stride, both in ((100, 60, False), (64, 64, True), (1024, 1000, False)):
        chars, offs, (seq, start, strand) = ff.windows_device(window, stride, start=3, stop=150, device=gpu, both_strands=both)
        hc, ho = chars.cpu().numpy(), offs.cpu().numpy()
        rebuilt = {}
        for r in range(len(seq)):
            piece = hc[ho[r]:ho[r + 1]]
            if strand[r]:
                assert bytes(twin.COMP[piece[::-1]]) == bytes(seqs[seq[r]][start[r]:start[r] + len(piece)])
                continue
            buf = rebuilt.setdefault(int(seq[r]), bytearray(len(seqs[seq[r]])))
            buf[start[r]:start[r] + len(piece)] = piece.tobytes()
        assert sorted(rebuilt) == list(range(3, 150))
        for j, buf in rebuilt.items():
            assert bytes(buf) == seqs[j]
