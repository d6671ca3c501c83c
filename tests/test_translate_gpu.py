"""GPU: codon translation (bioseq_amd.translate, bsq_translate_packed_device) bit for bit against the numpy twin
(tests/translate_twin.py) -- every launch class, the vector edges, the reverse frames against the views, statuses and cuts behind
guard bytes, a side stream --, the encodes of translated batches against the oracle, and the translating FlatFileDataset."""
import ctypes

import numpy as np
import pytest

import translate_twin as twin
import views_twin

pytestmark = pytest.mark.gpu

GUARD = 256
VIEWS_POOL = np.frombuffer(b"ACGTNacgtnRYKMBVDHSWxX*-.\x00\xff\x80@[`{", dtype=np.uint8)  # the byte pool of tests/test_views_gpu.py
POOL = np.concatenate([VIEWS_POOL, np.frombuffer(b"Uu", dtype=np.uint8)])
BASES = np.frombuffer(b"ACGTACGTACGTacgtUu", dtype=np.uint8)


def _store(rng, lens, pool=POOL, bases=BASES):
    """Rows of bases with one character in sixteen drawn from the whole pool: most codons are whole, unknown ones are everywhere."""
    lens = np.asarray(lens, dtype=np.int64)
    total = int(lens.sum())
    chars = rng.choice(bases, total).astype(np.uint8)
    other = rng.random(total) < 1.0 / 16
    chars[other] = rng.choice(pool, int(other.sum()))
    offs = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return chars, offs


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _rule(frame, tab=None, unknown=ord("X")):
    from bioseq_amd import capi
    t = capi.Translate()
    ctypes.memmove(t.code, (twin.table(1) if tab is None else np.asarray(tab, np.uint8)).ctypes.data, 64)
    t.unknown, t.frame = unknown, frame
    return t


def _raw(gpu, store, index, frames, n, frame, capacity, tab=None, unknown=ord("X"), stream=None):
    """bsq_translate_packed_device into a buffer with GUARD bytes on both sides and poisoned offsets; returns (chars, offsets, status)
    on the host and checks the guards.  store: (device chars, device offsets, n_store)."""
    import torch
    from bioseq_amd import capi
    L = capi.load()
    dch, dof, n_store = store
    didx = _dev(index, gpu) if index is not None else None
    dfr = _dev(frames, gpu) if frames is not None else None
    n_out = 6 * n if frame == twin.SIX else n
    buf = torch.full((capacity + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    out_offs = torch.full((n_out + 1,), -7, dtype=torch.int64, device=gpu)
    status = torch.zeros(1, dtype=torch.int64, device=gpu)
    s = stream.cuda_stream if stream is not None else capi.raw_stream(gpu)
    capi.check(L.bsq_translate_packed_device(dch.data_ptr(), dof.data_ptr(), n_store, didx.data_ptr() if didx is not None else None,
                                             dfr.data_ptr() if dfr is not None else None, n, ctypes.byref(_rule(frame, tab, unknown)),
                                             buf.data_ptr() + GUARD, capacity, out_offs.data_ptr(), status.data_ptr(), ctypes.c_void_p(s)))
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + capacity:] == 0xA5).all(), "a guard byte of out_chars was overwritten"
    return raw[GUARD:GUARD + capacity], out_offs.cpu().numpy(), int(status.item())


def _same(got, exp):
    assert got[2] == exp[2]
    assert np.array_equal(got[1], exp[1])
    assert got[0].tobytes() == exp[0].tobytes()


@pytest.fixture(scope="module")
def big(gpu):
    """The store of the launch-class cases: 3000 rows of 0 .. 2500 characters, on the host and the device, and the twin's row cache."""
    rng = np.random.default_rng(16)
    lens = rng.integers(0, 2501, 3000)
    lens[:3] = 0
    chars, offs = _store(rng, lens)
    return {"chars": chars, "offs": offs, "dev": (_dev(chars, gpu), _dev(offs, gpu), 3000), "cache": {}}


@pytest.mark.parametrize("case, n", list(enumerate([0, 1, 4095, 4096, 4097, 100000])))
def test_launch_classes_one_frame(gpu, big, case, n):
    rng = np.random.default_rng(n)
    index = rng.integers(0, 3000, n).astype(np.int64)  # repeats included
    code = case % 6
    exp = twin.translate(big["chars"], big["offs"], index, frame=code, cache=big["cache"])
    _same(_raw(gpu, big["dev"], index, None, n, code, int(exp[1][-1])), exp)


@pytest.mark.parametrize("n", [4096, 4097])
def test_launch_classes_per_row_frames(gpu, big, n):
    rng = np.random.default_rng(n + 1)
    index = rng.integers(0, 3000, n).astype(np.int64)
    frames = rng.integers(0, 6, n).astype(np.uint8)
    exp = twin.translate(big["chars"], big["offs"], index, frames=frames, cache=big["cache"])
    _same(_raw(gpu, big["dev"], index, frames, n, 0, int(exp[1][-1])), exp)


@pytest.mark.parametrize("n", [682, 683, 20000])  # 4092 / 4098 / 120000 output rows
def test_launch_classes_six_frames(gpu, big, n):
    from bioseq_amd import translate
    rng = np.random.default_rng(n)
    index = rng.integers(0, 3000, n).astype(np.int64)
    exp = twin.translate(big["chars"], big["offs"], index, frame=twin.SIX, cache=big["cache"])
    assert exp[1].size == 6 * n + 1
    _same(_raw(gpu, big["dev"], index, None, n, twin.SIX, int(exp[1][-1])), exp)
    assert translate.kernel_name(n, "six") == ("k_translate_small" if n == 682 else "k_translate_lengths+k_translate_place")


def test_scanned_place_beyond_2_pow_20_rows(gpu):
    """The class beyond 2^20 output rows (k_translate_lengths + k_translate_scan + k_translate_place<true>): 2^20 + 65 rows of 0 .. 3
    characters, so the last workgroup is partial and the last entry of the scanned sums is the sum of one row.  Frame 1 (no row of
    these holds a whole codon behind its first character: every offset is 0) and frame 0 (a row in four gives one residue), bit for
    bit against the library's host twin."""
    from bioseq_amd import translate
    n = 2 ** 20 + 65
    rng = np.random.default_rng(20)
    lens = np.arange(n, dtype=np.int64) % 4
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(offs[-1]))
    chars[rng.random(chars.size) < 0.01] = ord("N")
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    for code, total in ((1, 0), (0, n // 4)):
        assert translate.kernel_name(n, code) == "k_translate_lengths+k_translate_scan+k_translate_place"
        e_chars, e_offs = translate.translate_host(chars, offs, frame=code)
        assert e_offs.size == n + 1 and int(e_offs[-1]) == total == e_chars.size
        got_c, got_o = translate.translate_packed(dch, dof, frame=code)
        assert np.array_equal(got_o.cpu().numpy(), e_offs)
        assert got_c[:total].cpu().numpy().tobytes() == e_chars.tobytes()


def test_vector_edges_every_length_every_frame(gpu):
    """Every source length 0 .. 150 (15 / 16 / 17 residues, the 47-, 48- and 49-byte bodies at every phase, sources at every alignment
    modulo 16) and the round boundary of 16 lanes x 16 residues x 4: rows of 3 * 1024 - 2 .. 3 * 1024 + 4 characters."""
    rng = np.random.default_rng(2)
    lens = list(range(151)) + list(range(3 * 1024 - 2, 3 * 1024 + 5))
    chars, offs = _store(rng, lens)
    store = (_dev(chars, gpu), _dev(offs, gpu), len(lens))
    cache = {}
    for tab, unknown in ((twin.table(1), ord("X")), (twin.table(2), ord("?"))):
        cache = {}
        for code in list(range(6)) + [twin.SIX]:
            exp = twin.translate(chars, offs, frame=code, tab=tab, unknown=unknown, cache=cache)
            _same(_raw(gpu, store, None, None, len(lens), code, int(exp[1][-1]), tab, unknown), exp)
    # a table of the caller's own: every entry distinct, so that a wrong codon index shows whatever it is
    own = np.arange(64, dtype=np.uint8) + 48
    for code in (1, 5):
        exp = twin.translate(chars, offs, frame=code, tab=own)
        _same(_raw(gpu, store, None, None, len(lens), code, int(exp[1][-1]), own), exp)


def test_reverse_frames_are_forward_frames_of_the_reverse_complement_view(gpu):
    from bioseq_amd import translate, views
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 700, 400)
    chars, offs = _store(rng, lens, pool=VIEWS_POOL, bases=np.frombuffer(b"ACGTacgt", np.uint8))  # no U / u
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    seq = rng.integers(0, 400, 600).astype(np.int64)
    rc, rco = views.gather_views(dch, dof, seq, np.zeros(600, np.int64), lens[seq], np.ones(600, np.uint8))
    for f in range(3):
        a, ao = translate.translate_packed(dch, dof, index=seq, frame=3 + f)
        b, bo = translate.translate_packed(rc, rco, frame=f)
        total = int(ao[-1].item())
        assert (ao == bo).all() and (a[:total] == b[:total]).all()
        exp = twin.translate(chars, offs, seq, frame=3 + f)
        assert np.array_equal(ao.cpu().numpy(), exp[1]) and a[:total].cpu().numpy().tobytes() == exp[0].tobytes()


@pytest.mark.parametrize("n", [50, 5000])
def test_status_bad_rows_and_cuts(gpu, n):
    rng = np.random.default_rng(n)
    lens = rng.integers(40, 600, 6000)
    chars, offs = _store(rng, lens)
    store = (_dev(chars, gpu), _dev(offs, gpu), 6000)
    cache = {}
    # index NULL with n <= n_store: sequences 0 .. n - 1
    exp = twin.translate(chars, offs, np.arange(n), frame=4, cache=cache)
    _same(_raw(gpu, store, None, None, n, 4, int(exp[1][-1])), exp)
    # bad indices and a frame code above 5: empty rows, the first one reported
    index = rng.integers(0, 6000, n).astype(np.int64)
    index[n // 2], index[-1] = -1, 6000
    frames = rng.integers(0, 6, n).astype(np.uint8)
    exp = twin.translate(chars, offs, index, frames=frames, cache=cache)
    got = _raw(gpu, store, index, frames, n, 0, int(exp[1][-1]))
    _same(got, exp)
    assert got[2] == n // 2 and not np.diff(got[1])[[n // 2, n - 1]].any()
    frames[n // 3] = 6
    exp = twin.translate(chars, offs, index, frames=frames, cache=cache)
    got = _raw(gpu, store, index, frames, n, 0, int(exp[1][-1]))
    _same(got, exp)
    assert got[2] == n // 3 and np.diff(got[1])[n // 3] == 0
    exp = twin.translate(chars, offs, index, frame=twin.SIX, cache=cache)
    got = _raw(gpu, store, index, None, n, twin.SIX, int(exp[1][-1]))
    _same(got, exp)
    assert got[2] == n // 2 and not np.diff(got[1])[6 * (n // 2):6 * (n // 2) + 6].any()
    # a capacity short by one byte and by one whole row: cut there, nothing written past it (the guards), the first row that did not fit
    index = rng.integers(0, 6000, n).astype(np.int64)
    for code in (2, 3, twin.SIX):
        full = twin.translate(chars, offs, index, frame=code, cache=cache)
        last = int(np.diff(full[1])[-1])
        assert last > 0
        for cap in (int(full[1][-1]) - 1, int(full[1][-1]) - last, int(full[1][-1]) * 2 // 3 + 5):
            exp = twin.translate(chars, offs, index, frame=code, cache=cache, capacity=cap)
            got = _raw(gpu, store, index, None, n, code, cap)
            _same(got, exp)
            n_out = full[1].size - 1
            assert got[2] == n_out + int(np.nonzero(full[1][1:] > cap)[0][0]) and np.array_equal(got[1], full[1])


def test_side_stream_and_python_api(gpu):
    import torch
    from bioseq_amd import translate
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 3000, 500)
    chars, offs = _store(rng, lens)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    store = (dch, dof, 500)
    n = 6000
    index = rng.integers(0, 500, n).astype(np.int64)
    cache = {}
    side = torch.cuda.Stream(device=gpu)
    for code in (1, twin.SIX):
        exp = twin.translate(chars, offs, index[:1200], frame=code, cache=cache)
        _same(_raw(gpu, store, index[:1200], None, 1200, code, int(exp[1][-1]), stream=side), exp)
    exp = twin.translate(chars, offs, index, frame=5, cache=cache)
    _same(_raw(gpu, store, index, None, n, 5, int(exp[1][-1]), stream=side), exp)
    # the Python call: host and device index lists, a frame per row, every sequence, the stop letter; errors with validate
    total = int(exp[1][-1])
    for idx in (list(index), _dev(index, gpu)):
        c, o = translate.translate_packed(dch, dof, index=idx, frame=5)
        assert np.array_equal(o.cpu().numpy(), exp[1]) and c[:total].cpu().numpy().tobytes() == exp[0].tobytes()
    frames = rng.integers(0, 6, n).astype(np.uint8)
    e = twin.translate(chars, offs, index, frames=frames, cache=cache)
    for fr in (frames, _dev(frames, gpu)):
        c, o = translate.translate_packed(dch, dof, index=index, frame=fr)
        assert np.array_equal(o.cpu().numpy(), e[1]) and c[:int(e[1][-1])].cpu().numpy().tobytes() == e[0].tobytes()
    tab = twin.table(4)
    tab[tab == ord("*")] = ord("$")
    for frame, code in ((2, 2), ("six", twin.SIX)):
        e = twin.translate(chars, offs, frame=code, tab=tab, unknown=ord("?"))
        c, o = translate.translate_packed(dch, dof, frame=frame, table=4, stop="$", unknown="?")
        assert np.array_equal(o.cpu().numpy(), e[1]) and c[:int(e[1][-1])].cpu().numpy().tobytes() == e[0].tobytes()
    with pytest.raises(IndexError):
        translate.translate_packed(dch, dof, index=_dev(np.array([1, 500]), gpu))
    with pytest.raises(IndexError):
        translate.translate_packed(dch, dof, index=[1, 2], frame=_dev(np.array([1, 6], np.uint8), gpu))
    c, o = translate.translate_packed(dch, dof, index=_dev(np.array([1, 500]), gpu), validate=False)
    assert int(o[2].item()) == int(o[1].item()) == twin.length(lens[1], 0)
    c, o = translate.translate_packed(dch[:0], dof[:1])
    assert o.cpu().tolist() == [0]


def _rows(e_chars, e_offs):
    return [bytes(e_chars[e_offs[i]:e_offs[i + 1]]) for i in range(len(e_offs) - 1)]


@pytest.mark.parametrize("key", ["AMINO20", "SEB8"])
def test_tokens_of_a_translated_batch_equal_the_oracle(gpu, bsq, oracle, key):
    from bioseq_amd import translate
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 900, 400)
    chars, offs = _store(rng, lens)
    index = rng.integers(0, 400, 300).astype(np.int64)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    tok = bsq.Tokenizer(key, True, True, True)
    ora = oracle.OracleTokenizer(key, True, True, True)
    P = 900 // 3 + 2
    for frame, code in ((1, 1), (3, 3), ("six", twin.SIX)):
        e_chars, e_offs, _ = twin.translate(chars, offs, index, frame=code)
        vc, vo = translate.translate_packed(dch, dof, index=_dev(index, gpu), frame=frame)
        got = tok.tokenize_packed(vc, vo, P, "q", True)
        assert got.cpu().numpy().tobytes() == ora.batch_tokenize(_rows(e_chars, e_offs), padlen=P, destchar="q", batch_first=True).tobytes()
    got = tok.onehot_packed(vc, vo, P, "f")
    assert got.cpu().numpy().tobytes() == ora.batch_onehot_encode(_rows(e_chars, e_offs), padlen=P, destchar="f").tobytes()


def _flatfile(tmp_path, rng, n=700):
    from bioseq_amd.flatfile import FlatFile, write_flatfile
    lens = rng.integers(0, 400, n)
    lens[5] = 5000  # one long outlier
    lens[9] = 0
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGTACGTACGTACGTNacgtRYUu", np.uint8), L)) for L in lens]
    return FlatFile(write_flatfile(seqs, str(tmp_path / "translate.ff"))), seqs


CROP_KEY = lambda k: (13 * 0xC2B2AE3D27D4EB4F + k) & (2 ** 64 - 1)  # noqa: E731  the dataset's k-th crop key (seed 13)
MASK_KEY = lambda k: (13 * 0x9E3779B97F4A7C15 + k) & (2 ** 64 - 1)  # noqa: E731  ... and its k-th mask key


def _expected_batch(ff, order, crop, frac, key, first, frame):
    """crop / strand views of the store rows `order` by the views twin, then translated by the translation twin: (chars, offsets)."""
    starts, lengths, strand = views_twin.plan(ff._offsets, crop, order, mode="random", revcomp_frac=frac, seed=key, first_row=first)
    v_chars, v_offs = views_twin.apply(np.asarray(ff._chars), ff._offsets, order, starts, lengths, strand)
    e_chars, e_offs, status = twin.translate(v_chars, v_offs, frame=frame)
    assert status == -1
    return e_chars, e_offs


def test_dataset_translate_plain_shuffle_prefetch(gpu, bsq, oracle, tmp_path):
    import torch
    from bioseq_amd.loaders import FlatFileDataset
    ff, seqs = _flatfile(tmp_path, np.random.default_rng(2))
    tok = bsq.Tokenizer("AMINO20", True, True, True)
    ora = oracle.OracleTokenizer("AMINO20", True, True, True)
    crop, width = 96, 96 // 3 + 2

    def epoch(**opts):
        ds = FlatFileDataset(ff, tok, device=gpu, translate=0, crop=crop, revcomp_frac=0.5, token_dtype="q")
        g = torch.Generator(device=gpu).manual_seed(5)
        out = [b.clone() for b in ds.batches(128, generator=g, **opts)]
        torch.cuda.synchronize()
        return ds, out

    ds, base = epoch()
    assert ds.max_seq_len == width and all(b.shape[-1] == width for b in base)
    g = torch.Generator(device=gpu).manual_seed(5)
    order = torch.randperm(len(ff), device=gpu, generator=g).cpu().numpy()
    e_chars, e_offs = _expected_batch(ff, order, crop, 0.5, CROP_KEY(1), 0, 0)
    exp = ora.batch_tokenize(_rows(e_chars, e_offs), padlen=width, destchar="q", batch_first=True)
    assert torch.cat(base).cpu().numpy().tobytes() == np.ascontiguousarray(exp).tobytes()
    for opts in ({"prefetch": 2}, {"group": 4}, {"group": 4, "prefetch": 2}):
        _, got = epoch(**opts)
        assert len(got) == len(base) and all(torch.equal(a, b) for a, b in zip(base, got)), opts
    # get_batch and index lists; without a crop the width is a third of the longest row, and another frame and table
    got = ds.get_batch(0, 40)
    e_chars, e_offs = _expected_batch(ff, np.arange(40), crop, 0.5, CROP_KEY(2), 0, 0)
    assert got.cpu().numpy().tobytes() == ora.batch_tokenize(_rows(e_chars, e_offs), padlen=width, destchar="q", batch_first=True).tobytes()
    whole = FlatFileDataset(ff, tok, device=gpu, translate=2, codon_table=2)
    assert whole.max_seq_len == 5000 // 3 + 2
    idx = [5, 9, 5, 200, 17]
    got = whole.__getitems__(idx)
    e = twin.translate(np.asarray(ff._chars), ff._offsets, idx, frame=2, tab=twin.table(2))
    assert got.cpu().numpy().tobytes() == ora.batch_tokenize(_rows(e[0], e[1]), padlen=whole.max_seq_len, destchar="q", batch_first=True).tobytes()
    got = whole.get_batch(3, 60)
    e = twin.translate(np.asarray(ff._chars), ff._offsets, np.arange(3, 60), frame=2, tab=twin.table(2))
    assert got.cpu().numpy().tobytes() == ora.batch_tokenize(_rows(e[0], e[1]), padlen=whole.max_seq_len, destchar="q", batch_first=True).tobytes()


def test_dataset_translate_masked_and_packed(gpu, bsq, oracle, tmp_path):
    import torch
    import mlm_twin
    import pack_twin
    from bioseq_amd import capi
    from bioseq_amd.loaders import FlatFileDataset
    ff, seqs = _flatfile(tmp_path, np.random.default_rng(3), 300)
    flags = (1, 1, 1)
    tok = bsq.Tokenizer("AMINO20", *flags)
    ora = oracle.OracleTokenizer("AMINO20", *flags)
    crop, width = 96, 96 // 3 + 2
    # masked: the masks are drawn on the translated rows (the mask twin over the translated batch)
    dsm = FlatFileDataset(ff, tok, device=gpu, translate=0, crop=crop, revcomp_frac=0.5, masked=True, maskfrac=0.2)
    inp, lab = dsm.get_batch(0, 50)
    e_chars, e_offs = _expected_batch(ff, np.arange(50), crop, 0.5, CROP_KEY(1), 0, 0)
    plain = ora.tokenize_packed(e_chars, e_offs, width, "i", True).astype(np.int64)
    lut = np.frombuffer(bytes(capi.make_desc("AMINO20").lut), dtype=np.int8)
    ei, el = mlm_twin.mlm(plain, lut, ora.nchars(), 1, 1, e_chars, e_offs, 0.2, 0.8, 0.1, tok.alphabet_size(), -100, MASK_KEY(1), 0)
    assert np.array_equal(inp.cpu().numpy(), ei) and np.array_equal(lab.cpu().numpy(), el)
    # packed: the packing twin over the translated batch
    dsp = FlatFileDataset(ff, tok, device=gpu, translate=0, crop=crop, revcomp_frac=0.5, pack="nextfit", token_dtype="i")
    tokens, seg, pos = dsp.get_batch(0, 200)
    e_chars, e_offs = _expected_batch(ff, np.arange(200), crop, 0.5, CROP_KEY(1), 0, 0)
    exp = pack_twin.pack("AMINO20", flags, e_chars, e_offs, width, "nextfit", dtype=np.int32)
    assert tokens.dtype == torch.int32 and tokens.shape == (exp[4], width)
    assert np.array_equal(tokens.cpu().numpy(), exp[0]) and np.array_equal(seg.cpu().numpy(), exp[1]) and np.array_equal(pos.cpu().numpy(), exp[2])
    g = torch.Generator(device=gpu).manual_seed(7)
    a = [tuple(t.clone() for t in b) for b in dsp.batches(100, generator=g)]
    dsp2 = FlatFileDataset(ff, tok, device=gpu, translate=0, crop=crop, revcomp_frac=0.5, pack="nextfit", token_dtype="i")
    dsp2.get_batch(0, 200)  # (the same number of view calls in front of the epoch: the same keys)
    g = torch.Generator(device=gpu).manual_seed(7)
    b = [tuple(t.clone() for t in x) for x in dsp2.batches(100, generator=g, prefetch=2)]
    assert len(a) == len(b) == 3 and all(torch.equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))
    # the store is never written
    store = ff.to_device(gpu)[0].clone()
    dsa = FlatFileDataset(ff, tok, device=gpu, translate=1, augment=2, augment_frac=1.0)
    assert dsa.get_batch(0, 50).shape == (50, 5000 // 3 + 2)
    assert torch.equal(store, ff.to_device(gpu)[0])
