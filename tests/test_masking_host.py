"""CPU: the masked-LM draw (include/bsq.h, bsq_mlm) -- the library's host twin bsq_random_mask_host against the numpy twin
(tests/mlm_twin.py) byte for byte, the statistics of the draw, the argument rules and the exports.  No device is needed."""
import ctypes

import numpy as np
import pytest

import mlm_twin as twin


def _lib():
    from bioseq_amd import capi
    return capi, capi.load()


def _batch(rng, nseq, maxlen, unmapped=True):
    lens = rng.integers(0, maxlen + 1, nseq)
    lens[: min(3, nseq)] = 0  # empty sequences up front
    alphabet = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYacgtnBJOUXZ*-.\x00\xff\x80", dtype=np.uint8)
    pool = alphabet if unmapped else alphabet[:20]
    chars = rng.choice(pool, int(lens.sum())).astype(np.uint8)
    offsets = np.zeros(nseq + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    return chars, offsets


def _host_mask(key, chars, offsets, frac, seed, first_row):
    capi, L = _lib()
    d = capi.make_desc(key)
    m = capi.Mlm(frac, 0.8, 0.1, 0, -100, seed, first_row)
    out = np.full(len(chars), 7, dtype=np.uint8)
    st = L.bsq_random_mask_host(ctypes.byref(d), chars.ctypes.data, offsets.ctypes.data, len(offsets) - 1, ctypes.byref(m), out.ctypes.data)
    assert st == capi.OK, L.bsq_last_error()
    return out, np.frombuffer(bytes(d.lut), dtype=np.int8)


def test_new_symbols_are_exported():
    capi, L = _lib()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_mlm_tokenize_device", "bsq_random_mask_device", "bsq_random_mask_host"):
        assert n in names and hasattr(L, n)


@pytest.mark.parametrize("key", ["DNA", "AMINO20", "SEB8", "DAYHOFF", "BYTES"])
def test_host_mask_equals_numpy_twin(key):
    rng = np.random.default_rng(sum(key.encode()))
    for trial in range(6):
        chars, offsets = _batch(rng, int(rng.integers(1, 300)), int(rng.choice([5, 64, 700, 5000])))
        if key == "BYTES":
            chars = rng.integers(0, 256, len(chars)).astype(np.uint8)
        seed = int(rng.integers(0, 2 ** 63)) * 2 + trial % 2
        first_row = int(rng.integers(0, 2 ** 40)) if trial % 3 else 0
        frac = float(rng.choice([0.0, 0.15, 0.5, 1.0, rng.random()]))
        got, lut = _host_mask(key, chars, offsets, frac, seed, first_row)
        exp = twin.mask(lut, chars, offsets, frac, seed, first_row)
        assert np.array_equal(got, exp), (key, trial, frac)
        unmapped = lut[chars] < 0
        assert (got[unmapped] == 1).all()  # unmapped characters are never selected
        if frac == 1.0:
            assert (got[~unmapped] == 0).all()


def test_host_mask_with_offsets_not_at_zero_and_bytes_between():
    """A batch that starts inside its buffer: only [offsets[0], offsets[B]) is written."""
    rng = np.random.default_rng(5)
    chars, offsets = _batch(rng, 40, 60)
    chars = np.concatenate([np.full(9, ord("A"), np.uint8), chars, np.full(5, ord("A"), np.uint8)])
    offsets = offsets + 9
    got, lut = _host_mask("AMINO20", chars, offsets, 0.3, 99, 4)
    assert (got[:9] == 7).all() and (got[-5:] == 7).all()
    exp = twin.mask(lut, chars, offsets, 0.3, 99, 4)
    assert np.array_equal(got[9:-5], exp[9:-5])


def test_shard_invariance_on_the_host():
    rng = np.random.default_rng(11)
    chars, offsets = _batch(rng, 200, 300)
    whole, _ = _host_mask("AMINO20", chars, offsets, 0.15, 1234, 0)
    split = 77
    lo_c, lo_o = chars[: offsets[split]], offsets[: split + 1]
    hi_c, hi_o = chars[offsets[split]:], offsets[split:] - offsets[split]
    a, _ = _host_mask("AMINO20", lo_c.copy(), lo_o.copy(), 0.15, 1234, 0)
    b, _ = _host_mask("AMINO20", hi_c.copy(), hi_o.copy(), 0.15, 1234, split)
    assert np.array_equal(np.concatenate([a, b]), whole)


def _big_draw(frac=0.15, seed=2024):
    rng = np.random.default_rng(3)
    chars, offsets = _batch(rng, 4000, 600, unmapped=False)  # ~1.2 million mapped characters
    lut = np.frombuffer(bytes(_lib()[0].make_desc("AMINO20").lut), dtype=np.int8)
    return twin.draw(lut, chars, offsets, frac, seed), len(chars)


def test_selected_share_within_4_sigma():
    for frac in (0.15, 0.5, 0.03):
        (row, j, selected, cat, rnd, sel16), n = _big_draw(frac)
        assert n >= 10 ** 6
        p = twin.threshold(frac) / 65536.0
        sigma = np.sqrt(n * p * (1 - p))
        assert abs(int(selected.sum()) - n * p) < 4 * sigma, (frac, int(selected.sum()), n * p)


def test_split_and_random_ids_are_uniform():
    (row, j, selected, cat, rnd, sel16), n = _big_draw(0.5)
    cat, rnd = cat[selected], rnd[selected]
    m = len(cat)
    tm, tr = twin.threshold(0.8), twin.threshold(0.8) + twin.threshold(0.1)
    counts = np.array([(cat < tm).sum(), ((cat >= tm) & (cat < tr)).sum(), (cat >= tr).sum()])
    expected = m * np.array([tm, tr - tm, 65536 - tr]) / 65536.0
    chi2 = (((counts - expected) ** 2) / expected).sum()
    assert chi2 < 20, (counts, expected)  # 2 degrees of freedom: p ~ 5e-5
    ids = (rnd[(cat >= tm) & (cat < tr)] * 20) >> 16
    hist = np.bincount(ids, minlength=20)
    assert hist.shape == (20,)
    e = len(ids) / 20.0
    chi2 = (((hist - e) ** 2) / e).sum()
    assert chi2 < 60, hist  # 19 degrees of freedom: p ~ 5e-6


def test_four_lanes_of_a_selection_word_are_uncorrelated():
    (row, j, selected, cat, rnd, sel16), n = _big_draw(0.15)
    # whole quads only: the 4 lanes of one word side by side
    quad0 = np.nonzero((j % 4 == 0))[0]
    quad0 = quad0[quad0 + 3 < len(j)]
    quad0 = quad0[(row[quad0 + 3] == row[quad0])]
    lanes = np.stack([sel16[quad0 + k].astype(np.float64) for k in range(4)])
    r = np.corrcoef(lanes)
    bound = 5.0 / np.sqrt(len(quad0))
    off = r[~np.eye(4, dtype=bool)]
    assert np.abs(off).max() < bound, (r, bound)
    # and each lane is uniform over 16 bits (mean, loose)
    assert np.abs(lanes.mean(axis=1) - 32767.5).max() < 5 * 18918.6 / np.sqrt(len(quad0))


@pytest.mark.parametrize("kw, what", [({"frac": 1.5}, "frac"), ({"frac": -0.1}, "frac"), ({"mask_prob": 1.2}, "mask_prob"),
                                      ({"random_prob": -1}, "random_prob"), ({"mask_prob": 0.8, "random_prob": 0.3}, "exceed"),
                                      ({"first_row": -1}, "first_row"), ({"frac": float("nan")}, "frac")])
def test_argument_errors_raise_in_python_before_any_device(kw, what):
    from bioseq_amd import masking, Tokenizer
    tok = Tokenizer("AMINO20")
    with pytest.raises(ValueError, match=what):
        masking.mlm_tokenize_packed(tok, None, None, 16, **kw)
    if "mask_prob" not in kw and "random_prob" not in kw:
        args = {"frac": 0.15, "seed": 0}
        args.update({k: v for k, v in kw.items() if k in ("frac", "first_row")})
        with pytest.raises(ValueError, match=what):
            masking.random_mask_packed(tok, None, None, **args)
        with pytest.raises(ValueError, match=what):
            masking.onehot_masked_packed(tok, None, None, 16, **args)


def test_argument_errors_of_the_c_abi():
    """BSQ_ERR_INVALID_ARG before any launch (so also on a machine without a device)."""
    capi, L = _lib()
    d = capi.make_desc("DNA")
    chars = np.frombuffer(b"ACGTACGT", dtype=np.uint8).copy()
    offs = np.array([0, 4, 8], dtype=np.int64)
    out = np.zeros(16, dtype=np.int8)
    good = dict(frac=0.15, mask_prob=0.8, random_prob=0.1, mask_token=4, ignore_index=-100, seed=1, first_row=0)
    for bad in ({"frac": 2.0}, {"mask_prob": -0.5}, {"random_prob": 1.01}, {"mask_prob": 0.7, "random_prob": 0.4}, {"first_row": -3}):
        m = capi.Mlm(**dict(good, **bad))
        assert L.bsq_random_mask_host(ctypes.byref(d), chars.ctypes.data, offs.ctypes.data, 2, ctypes.byref(m), out.ctypes.data) == capi.ERR_INVALID_ARG
        assert L.bsq_mlm_tokenize_device(ctypes.byref(d), chars.ctypes.data, offs.ctypes.data, 2, 8, 1, ctypes.byref(m), capi.I8,
                                         out.ctypes.data, capi.U64, None, None) == capi.ERR_INVALID_ARG
    m = capi.Mlm(**good)
    assert L.bsq_mlm_tokenize_device(ctypes.byref(d), chars.ctypes.data, offs.ctypes.data, 2, 8, 1, ctypes.byref(m), capi.I8, None,
                                     capi.U64, None, None) == capi.ERR_INVALID_ARG
    assert b"both outputs" in L.bsq_last_error()
    assert L.bsq_mlm_tokenize_device(ctypes.byref(d), chars.ctypes.data, offs.ctypes.data, 2, 8, 1, None, capi.I8, out.ctypes.data,
                                     capi.U64, None, None) == capi.ERR_INVALID_ARG
    assert L.bsq_random_mask_device(ctypes.byref(d), chars.ctypes.data, offs.ctypes.data, 2, ctypes.byref(capi.Mlm(**dict(good, frac=3.0))),
                                    out.ctypes.data, None) == capi.ERR_INVALID_ARG
    # an empty batch is fine and touches nothing
    assert L.bsq_mlm_tokenize_device(ctypes.byref(d), None, offs.ctypes.data, 0, 8, 1, ctypes.byref(m), capi.I8, out.ctypes.data,
                                     capi.U64, None, None) == capi.OK
