"""CPU: the crop / strand draw (include/bsq.h, bsq_crop) -- the library's host twin bsq_crop_plan_host against the numpy twin
(tests/views_twin.py) exactly, the statistics of the draw, the complement table, tile_plan, the argument rules and the dataset's key
check.  No device is needed."""
import ctypes

import numpy as np
import pytest

import views_twin as twin


def _lib():
    from bioseq_amd import capi
    return capi, capi.load()


def _offsets(lens):
    offs = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return offs


def test_new_symbols_are_exported():
    capi, L = _lib()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_crop_packed_device", "bsq_crop_plan_host", "bsq_views_packed_device", "bsq_complement_table"):
        assert n in names and hasattr(L, n)
    assert L.bsq_abi_version() == 7


@pytest.mark.parametrize("window", [0, 1, 15, 16, 17, 1024])
@pytest.mark.parametrize("mode", ["random", "head", "center"])
def test_host_plan_equals_numpy_twin(window, mode):
    from bioseq_amd import views
    rng = np.random.default_rng(window * 7 + len(mode))
    for trial in range(4):
        # lengths below, at and far above the window, empty ones too
        lens = np.concatenate([[0, window, max(window - 1, 0), window + 1, 5 * window + 3, 40000],
                               rng.integers(0, 3 * max(window, 8) + 1, 200)]).astype(np.int64)
        offs = _offsets(lens)
        seed = int(rng.integers(0, 2 ** 63)) * 2 + trial % 2
        first_row = int(rng.integers(0, 2 ** 40)) if trial % 2 else 0
        frac = [0.0, 0.3, 1.0][trial % 3]
        index = None if trial < 2 else rng.integers(0, lens.size, 500)
        got = views.crop_plan(offs, window, index=index, mode=mode, revcomp_frac=frac, seed=seed, first_row=first_row)
        exp = twin.plan(offs, window, index, mode=mode, revcomp_frac=frac, seed=seed, first_row=first_row)
        for g, e in zip(got, exp):
            assert np.array_equal(g, e), (window, mode, trial)
        starts, lengths, strand = got
        Ls = lens if index is None else lens[index]
        assert (starts >= 0).all() and (starts + lengths <= Ls).all()
        assert (lengths == (np.minimum(Ls, window) if window else Ls)).all()
        if frac == 0.0:
            assert not strand.any()
        if frac == 1.0:
            assert strand.all()


def test_plan_is_shard_invariant():
    from bioseq_amd import views
    offs = _offsets(np.random.default_rng(1).integers(0, 3000, 1000))
    whole = views.crop_plan(offs, 100, revcomp_frac=0.5, seed=9)
    idx = np.arange(1000)
    a = views.crop_plan(offs, 100, index=idx[:377], revcomp_frac=0.5, seed=9)
    b = views.crop_plan(offs, 100, index=idx[377:], revcomp_frac=0.5, seed=9, first_row=377)
    for w, x, y in zip(whole, a, b):
        assert np.array_equal(w, np.concatenate([x, y]))


def test_random_starts_are_uniform_and_strand_rate_matches():
    from bioseq_amd import views
    window, L, n = 100, 140, 82000  # starts uniform over [0, 40]: 41 cells of ~2000
    offs = _offsets(np.full(n, L))
    starts, lengths, strand = views.crop_plan(offs, window, revcomp_frac=0.3, seed=12345)
    counts = np.bincount(starts, minlength=L - window + 1)
    assert counts.size == L - window + 1
    expect = n / counts.size
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    assert chi2 < 80.0, chi2  # 40 degrees of freedom: p ~ 1e-4
    p = twin.threshold(0.3) / 65536.0
    rate = strand.mean()
    assert abs(rate - p) < 5 * np.sqrt(p * (1 - p) / n), rate


def test_complement_table_is_the_spec_table_and_an_involution():
    from bioseq_amd import views
    t = views.complement_table()
    assert t.dtype == np.uint8 and t.shape == (256,)
    assert np.array_equal(t, twin.COMP)
    assert np.array_equal(t[t], np.arange(256, dtype=np.uint8))
    assert bytes(t[np.frombuffer(b"ACGTNacgtnRYKMBVDHSW", np.uint8)]) == b"TGCANtgcanYRMKVBHDSW"


@pytest.mark.parametrize("window, stride", [(100, 30), (100, 100), (64, 1), (16, 15)])
@pytest.mark.parametrize("both", [False, True])
def test_tile_plan_covers_every_character(window, stride, both):
    from bioseq_amd import views
    lens = np.array([0, 1, window - 1, window, window + 1, 3 * window + 7, 1000], dtype=np.int64)
    offs = _offsets(lens)
    seq, start, length, strand = views.tile_plan(offs, window, stride, both_strands=both)
    seq2, start2, length2, strand2 = views.tile_plan(lens, window, stride, both_strands=both, lengths=True)
    assert all(np.array_equal(a, b) for a, b in zip((seq, start, length, strand), (seq2, start2, length2, strand2)))
    if both:
        assert np.array_equal(strand, np.tile([0, 1], seq.size // 2))
        assert np.array_equal(seq[0::2], seq[1::2]) and np.array_equal(start[0::2], start[1::2])
        seq, start, length = seq[0::2], start[0::2], length[0::2]
    else:
        assert not strand.any()
    assert np.array_equal(np.unique(seq), np.arange(lens.size))
    for j, L in enumerate(lens):
        mine = seq == j
        s, n = start[mine], length[mine]
        assert (n == min(L, window)).all() and (s >= 0).all() and (s + n <= L).all()
        if L == 0:
            assert mine.sum() == 1
            continue
        covered = np.zeros(L, bool)
        for a, b in zip(s, n):
            covered[a:a + b] = True
        assert covered.all(), (j, L)
        regular = s[:-1]
        assert np.array_equal(regular, np.arange(regular.size) * stride) and (regular + window < L).all()
        assert s[-1] == max(0, L - window)


def _crop(capi, window=16, mode=0, frac=0.0, seed=1, first_row=0):
    return capi.Crop(window, mode, frac, seed, first_row)


def test_argument_errors_before_any_launch():
    capi, L = _lib()
    offs = _offsets([5, 7, 9])
    chars = np.zeros(21, np.uint8)
    out = np.zeros(64, np.uint8)
    out_offs = np.zeros(8, np.int64)
    idx = np.array([0, 2], np.int64)
    st = np.zeros(1, np.int64)

    def dev(c, n=2, index=idx.ctypes.data, offsets=offs.ctypes.data, out_offsets=out_offs.ctypes.data, ch=chars.ctypes.data):
        # host pointers are never touched: every one of these calls is refused before any HIP call
        return L.bsq_crop_packed_device(ch, offsets, 3, index, n, ctypes.byref(c) if c is not None else None, out.ctypes.data, 64,
                                        out_offsets, None, None, st.ctypes.data, None)

    bad = [_crop(capi, window=-1), _crop(capi, mode=3), _crop(capi, mode=-1), _crop(capi, frac=1.5), _crop(capi, frac=-0.1),
           _crop(capi, frac=float("nan")), _crop(capi, first_row=-1)]
    for c in bad:
        assert dev(c) == capi.ERR_INVALID_ARG
        s = np.zeros(2, np.int64)
        assert L.bsq_crop_plan_host(offs.ctypes.data, 3, idx.ctypes.data, 2, ctypes.byref(c), s.ctypes.data, s.ctypes.data,
                                    out.ctypes.data) == capi.ERR_INVALID_ARG
    good = _crop(capi)
    assert dev(None) == capi.ERR_INVALID_ARG
    assert dev(good, offsets=None) == capi.ERR_INVALID_ARG
    assert dev(good, out_offsets=None) == capi.ERR_INVALID_ARG
    assert dev(good, ch=None) == capi.ERR_INVALID_ARG
    assert dev(good, n=-1) == capi.ERR_INVALID_ARG
    assert dev(good, index=None, n=4) == capi.ERR_INVALID_ARG  # no index list, n > n_store
    assert L.bsq_views_packed_device(chars.ctypes.data, offs.ctypes.data, 3, None, idx.ctypes.data, idx.ctypes.data, None, 2,
                                     out.ctypes.data, 64, out_offs.ctypes.data, st.ctypes.data, None) == capi.ERR_INVALID_ARG
    assert L.bsq_views_packed_device(chars.ctypes.data, None, 3, idx.ctypes.data, idx.ctypes.data, idx.ctypes.data, None, 2,
                                     out.ctypes.data, 64, out_offs.ctypes.data, st.ctypes.data, None) == capi.ERR_INVALID_ARG
    assert L.bsq_complement_table(None) == capi.ERR_INVALID_ARG
    # the host twin: a bad index and a missing output are argument errors too
    s = np.zeros(2, np.int64)
    assert L.bsq_crop_plan_host(offs.ctypes.data, 3, np.array([0, 3], np.int64).ctypes.data, 2, ctypes.byref(good), s.ctypes.data,
                                s.ctypes.data, out.ctypes.data) == capi.ERR_INVALID_ARG
    assert L.bsq_crop_plan_host(offs.ctypes.data, 3, None, 4, ctypes.byref(good), s.ctypes.data, s.ctypes.data,
                                out.ctypes.data) == capi.ERR_INVALID_ARG
    assert L.bsq_crop_plan_host(offs.ctypes.data, 3, None, 2, ctypes.byref(good), None, s.ctypes.data,
                                out.ctypes.data) == capi.ERR_INVALID_ARG


def test_python_argument_errors():
    from bioseq_amd import views
    offs = _offsets([5, 7])
    for kw in ({"mode": "tail"}, {"revcomp_frac": 2.0}, {"revcomp_frac": float("nan")}, {"first_row": -3}):
        with pytest.raises(ValueError):
            views.crop_plan(offs, 4, **kw)
    with pytest.raises(ValueError):
        views.crop_plan(offs, -1)
    with pytest.raises(IndexError):
        views.crop_plan(offs, 4, index=[0, 2])
    with pytest.raises(ValueError):
        views.tile_plan(offs, 0)
    with pytest.raises(ValueError):
        views.tile_plan(offs, 4, stride=0)


def test_dataset_rejects_revcomp_for_proteins_and_bad_crop(tmp_path):
    import bioseq_amd
    from bioseq_amd.flatfile import FlatFile, write_flatfile
    from bioseq_amd.loaders import FlatFileDataset
    ff = FlatFile(write_flatfile([b"ACGT", b"MKV"], str(tmp_path / "v.ff")))
    with pytest.raises(ValueError):
        FlatFileDataset(ff, bioseq_amd.Tokenizer("AMINO20", 1, 1, 1), device="cpu", revcomp_frac=0.5)
    with pytest.raises(ValueError):
        FlatFileDataset(ff, bioseq_amd.Tokenizer("DNA", 1, 1, 1), device="cpu", crop=0)
    with pytest.raises(ValueError):
        FlatFileDataset(ff, bioseq_amd.Tokenizer("DNA", 1, 1, 1), device="cpu", crop=8, crop_mode="tail")
    with pytest.raises(ValueError):
        FlatFileDataset(ff, bioseq_amd.Tokenizer("DNA", 1, 1, 1), device="cpu", revcomp_frac=1.5)
    # construction alone touches no device: a nucleotide key and a crop set the width
    for key in ("DNA", "DNA4", "DNA5"):
        ds = FlatFileDataset(ff, bioseq_amd.Tokenizer(key, 1, 1, 1), device="cpu", crop=32, revcomp_frac=0.5)
        assert ds.max_seq_len == ds.maxseqlen == 34
    ds = FlatFileDataset(ff, bioseq_amd.Tokenizer("AMINO20", 1, 1, 1), device="cpu", crop=2)
    assert ds.max_seq_len == 4
    assert FlatFileDataset(ff, bioseq_amd.Tokenizer("AMINO20", 1, 1, 1), device="cpu").max_seq_len == 6
