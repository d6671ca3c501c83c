"""GPU: masked-LM batches over BPE ids (bioseq_amd.bpe.bpe_mlm_tokenize_packed, bsq_bpe_mlm_tokenize_device) against the library's CPU
twin, byte for byte -- inputs, labels and lengths: row lengths at every lane, 64-position and form edge, the block form's bounds and
the too-long code, one to five rows, poly-A rows, N barriers, cut rows and P = 1, all 36 pairs of element types in both layouts, each
output left out, a side stream, frac 0 against the plain device encode and frac 1, shards, a mask token and an ignore_index of the
caller's, the outputs of refused calls, a store that ends at the last byte of its allocation, and the dataset's bpe= / bpe_mlm=
options.  tests/test_bpe_mlm_host.py holds the twin to an independent statement of the draw."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import bpe_twin as twin

pytestmark = pytest.mark.gpu

EDGES = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024)  # (tests/test_bpe_gpu.py's)
PARITY_MERGES = [("A", "A"), ("AA", "AA"), ("AA", "A")]
ALL_FLAGS = [(False, False, False), (True, True, True), (True, False, False), (False, True, False)]


def _tok(key="DNA4", eos=False, bos=False, padchar=False):
    import bioseq_amd
    return bioseq_amd.Tokenizer(key, eos, bos, padchar)


@functools.lru_cache(maxsize=None)
def _trained(flags=(False, False, False), key="DNA4", letters="ACGT", n_merges=200):
    from bioseq_amd import bpe
    rng = np.random.default_rng(n_merges)
    rows = [twin.random_row(rng, 300, letters) for _ in range(40)] + [twin.low_complexity_row(rng, 300, letters) for _ in range(20)]
    return bpe.bpe_train_host(_tok(key, *flags), *twin.pack(rows), n_merges)


def _dev(a, gpu):
    import torch
    return torch.from_numpy(a).to(gpu)


def _check(gpu, v, rows, P, destchar="i", batch_first=True, **kw):
    """bpe_mlm_tokenize_packed on uploaded copies against bpe_mlm_tokenize_host; returns the twin's (inputs, labels, lengths)."""
    import torch
    from bioseq_amd import bpe, capi
    chars, offs = twin.pack(rows)
    kw.setdefault("frac", 0.3)
    kw.setdefault("seed", 17)
    host_kw = dict(kw)
    if host_kw.get("max_chars") is None:
        host_kw["max_chars"] = 8192 if max(len(r) for r in rows) > 1024 or kw.get("form") == 2 else 1024
    exp = bpe.bpe_mlm_tokenize_host(v, chars, offs, P, destchar, batch_first, **host_kw)
    got = bpe.bpe_mlm_tokenize_packed(v, _dev(chars, gpu), _dev(offs, gpu), P, destchar, batch_first, **kw)
    for g, e, ch in zip(got[:2], exp[:2], (destchar, kw.get("label_destchar", "q"))):
        assert g.device == gpu and g.is_contiguous() and g.dtype == capi.dtype_of(ch)[1] and tuple(g.shape) == e.shape
    assert got[2].dtype == torch.int32 and tuple(got[2].shape) == (len(rows),)
    assert got[2].cpu().numpy().tobytes() == exp[2].tobytes(), (got[2].cpu().numpy().tolist(), exp[2].tolist())
    assert got[0].cpu().numpy().tobytes() == exp[0].tobytes(), "inputs"
    assert got[1].cpu().numpy().tobytes() == exp[1].tobytes(), "labels"
    return exp


@functools.lru_cache(maxsize=None)
def _edge_rows():
    rng = np.random.default_rng(42)
    rows = []
    for n in EDGES:
        rows += [twin.random_row(rng, n, "ACGT"), twin.random_row(rng, n, "ACGT", 0.02), twin.low_complexity_row(rng, n, "ACGT")]
    return rows


@pytest.mark.parametrize("form", [None, 1, 2])
def test_row_lengths_at_every_edge_in_both_forms(gpu, bsq, form):
    from bioseq_amd import bpe
    v = _trained()
    exp = _check(gpu, v, _edge_rows(), 1030, form=form)
    assert bpe.bpe_mlm_kernel_name(v, max_chars=1024, form=form) == ("k_bpe_mlm_block" if form == 2 else "k_bpe_mlm_wave")
    lab = exp[1].view(np.int64)
    assert (lab != -100).sum() > 500 and (lab[:3] == -100).all(), "tokens are selected; the empty rows hold none"


def test_block_form_lengths_and_the_too_long_code(gpu, bsq):
    """1025 and 8192 characters take the block form; 8193 gets -1, the inputs of an empty row and no label; under max_chars 1024 four do."""
    rng = np.random.default_rng(7)
    v = _trained((True, True, True))
    rows = [twin.random_row(rng, n, "ACGT", 0.01) for n in (1025, 8192, 8193, 100, 0, 4097)]
    for kw in (dict(), dict(max_chars=8192)):
        ins, lab, lens = _check(gpu, v, rows, 3000, "h", **kw)
        assert lens[2] == -1 and ins[2, :3].tolist() == [v.M + 5, v.M + 6, v.M + 7] and (lab[2].view(np.int64) == -100).all()
        assert (lens[[0, 1, 3, 5]] > 0).all() and (lab[1].view(np.int64) != -100).sum() > 100
    ins, lab, lens = _check(gpu, v, rows, 16, "h", max_chars=1024)
    assert lens.tolist()[:3] == [-1, -1, -1] and lens[3] > 0 and lens[5] == -1 and (lab[[0, 1, 2, 5]].view(np.int64) == -100).all()


@pytest.mark.parametrize("B", [1, 3, 4, 5])
def test_one_to_five_rows(gpu, bsq, B):
    """Four rows share a workgroup of the wave form: a last workgroup with one, three and four of its waves at work."""
    rng = np.random.default_rng(B)
    rows = [twin.random_row(rng, int(n), "ACGT", 0.02) for n in rng.integers(100, 700, B)]
    for form in (1, 2):
        _check(gpu, _trained(), rows, 400, form=form)


def test_poly_a_rows_of_every_length(gpu, bsq):
    from bioseq_amd import bpe
    v = bpe.BPEVocab.from_merges(_tok(), PARITY_MERGES)
    rows = [np.full(n, ord("A"), np.uint8) for n in range(1, 201)]
    for form in (1, 2):
        ins, lab, lens = _check(gpu, v, rows, 64, "b", label_destchar="b", form=form)
    assert lens[:8].tolist() == [1, 1, 1, 1, 2, 2, 2, 2] and (lab != -100).sum() > 300


def test_unmapped_bytes_are_barriers_at_the_boundaries(gpu, bsq):
    """N at positions 15, 16, 63, 64 and at a row's first and last character: an UNK is never selected, whatever frac is."""
    from bioseq_amd import bpe
    rng = np.random.default_rng(5)
    rows = []
    for at in ([15], [16], [63], [64], [0], [-1], [0, -1], [15, 16], [63, 64], [62, 64], [0, 15, 16, 63, 64, -1]):
        for base in (np.full(130, ord("A"), np.uint8), twin.low_complexity_row(rng, 130, "ACGT")):
            row = base.copy()
            row[at] = ord("N")
            rows.append(row)
    rows += [np.full(n, ord("N"), np.uint8) for n in (1, 2, 64, 65)]
    for v in (bpe.BPEVocab.from_merges(_tok(), PARITY_MERGES), _trained()):
        for form in (1, 2):
            ins, lab, lens = _check(gpu, v, rows, 140, label_destchar="i", frac=1.0, form=form)
        unk = ins == v.M + 4
        assert unk.sum() > 150 and (lab[unk] == -100).all() and (lab[-1] == -100).all() and (ins[-1, :65] == v.M + 4).all()


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_cut_rows_keep_their_count_in_lengths(gpu, bsq, flags):
    """P = 1, 2 and n + bos + eos - 1 .. + 1: lengths holds n before the cut, and a token that is not shown is not drawn."""
    v = _trained(flags)
    rng = np.random.default_rng(3)
    rows = [twin.random_row(rng, 300, "ACGT"), twin.random_row(rng, 40, "ACGT", 0.05), np.zeros(0, np.uint8)]
    eos, bos, _ = flags
    n = int(_check(gpu, v, rows, 400)[2][0])
    for P in (1, 2, n + bos + eos - 1, n + bos + eos, n + bos + eos + 1):
        for form in (1, 2):
            exp = _check(gpu, v, rows, P, form=form)
            assert exp[2][0] == n and exp[2][2] == 0


@functools.lru_cache(maxsize=None)
def _type_rows():
    rng = np.random.default_rng(8)
    return [twin.random_row(rng, int(n), "ACGT", 0.02) for n in rng.integers(0, 500, 37)]


@pytest.mark.parametrize("destchar,label_destchar", list(itertools.product("bhiqfd", repeat=2)))
def test_every_pair_of_element_types_in_both_layouts(gpu, bsq, destchar, label_destchar):
    v = _trained((True, True, True), n_merges=100)  # vocab 108, mask token 108: int8 holds them
    for batch_first, form in ((True, 1), (False, 2)):
        _check(gpu, v, _type_rows(), 131, destchar, batch_first, label_destchar=label_destchar, form=form)
    _check(gpu, v, _type_rows(), 131, destchar, False, label_destchar=label_destchar, form=1)
    _check(gpu, v, _type_rows(), 131, destchar, True, label_destchar=label_destchar, form=2)


def test_each_output_left_out_and_a_side_stream(gpu, bsq):
    import torch
    from bioseq_amd import bpe, capi
    L = capi.load()
    v = _trained((True, True, True), n_merges=100)
    chars, offs = twin.pack(_type_rows())
    B, P = len(offs) - 1, 131
    kw = dict(frac=0.3, seed=17)
    exp = bpe.bpe_mlm_tokenize_host(v, chars, offs, P, "h", label_destchar="i", max_chars=1024, **kw)
    dch, dof, table = _dev(chars, gpu), _dev(offs, gpu), v.device_table(gpu)
    m = capi.BpeMlm(0.3, 0.8, 0.1, bpe.bpe_vocab_size(v), -100, 17, 0)
    for form, no_in, no_lab in ((1, True, False), (2, False, True)):
        ins = torch.full((B, P), 0x5A5A, dtype=torch.int16, device=gpu)
        lab = torch.full((B, P), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
        lens = torch.empty(B, dtype=torch.int32, device=gpu)
        capi.check(L.bsq_bpe_mlm_tokenize_device(ctypes.byref(v.desc), dch.data_ptr(), dof.data_ptr(), B, P, 1, table.data_ptr(), v.M,
                                                 ctypes.byref(capi.Bpe(1024, form, 0)), ctypes.byref(m), capi.I16, None if no_in else ins.data_ptr(),
                                                 capi.I32, None if no_lab else lab.data_ptr(), lens.data_ptr(), None))
        torch.cuda.synchronize()
        assert lens.cpu().numpy().tobytes() == exp[2].tobytes()
        assert bool((ins == 0x5A5A).all()) if no_in else ins.cpu().numpy().tobytes() == exp[0].tobytes()
        assert bool((lab == 0x5A5A5A5A).all()) if no_lab else lab.cpu().numpy().tobytes() == exp[1].tobytes()
    side = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = bpe.bpe_mlm_tokenize_packed(v, dch, dof, P, "h", label_destchar="i", max_chars=1024, **kw)
    side.synchronize()
    assert all(g.cpu().numpy().tobytes() == e.tobytes() for g, e in zip(got, exp))


def test_frac_zero_is_the_plain_device_encode_and_frac_one_selects_every_token(gpu, bsq):
    import torch
    from bioseq_amd import bpe
    v = _trained()
    rows = _edge_rows()
    chars, offs = twin.pack(rows)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    for form, batch_first in ((1, True), (2, False)):
        plain_t, plain_l = bpe.bpe_tokenize_packed(v, dch, dof, 300, "h", batch_first, max_chars=1024, form=form)
        ins, lab, lens = bpe.bpe_mlm_tokenize_packed(v, dch, dof, 300, "h", batch_first, frac=0.0, seed=9, max_chars=1024, form=form)
        assert torch.equal(ins, plain_t) and torch.equal(lens, plain_l) and bool((lab == -100).all())
        exp = _check(gpu, v, rows, 300, "h", batch_first, frac=1.0, form=form)
        t = plain_t.cpu().numpy().astype(np.int64)
        t, lab1 = (t, exp[1].view(np.int64)) if batch_first else (t.T, exp[1].view(np.int64).T)
        token = (np.arange(300)[None, :] < np.minimum(plain_l.cpu().numpy(), 300)[:, None]) & (t != v.M + 4)
        assert token.sum() > 1000 and (~token).sum() > 1000 and (lab1[token] == t[token]).all() and (lab1[~token] == -100).all()


def test_the_whole_batch_against_two_shards(gpu, bsq):
    import torch
    from bioseq_amd import bpe
    v = _trained()
    rows = _type_rows()
    kw = dict(frac=0.25, seed=31, max_chars=1024)
    whole = bpe.bpe_mlm_tokenize_packed(v, *(_dev(a, gpu) for a in twin.pack(rows)), 200, "i", first_row=40, **kw)
    a = bpe.bpe_mlm_tokenize_packed(v, *(_dev(x, gpu) for x in twin.pack(rows[:13])), 200, "i", first_row=40, **kw)
    b = bpe.bpe_mlm_tokenize_packed(v, *(_dev(x, gpu) for x in twin.pack(rows[13:])), 200, "i", first_row=53, form=2, **kw)
    for w, x, y in zip(whole, a, b):
        assert torch.equal(w, torch.cat([x, y]))
    _check(gpu, v, rows, 200, first_row=40, **kw)


def test_a_mask_token_and_an_ignore_index_of_the_callers(gpu, bsq):
    v = _trained()
    for form in (1, 2):
        ins, lab, _ = _check(gpu, v, _type_rows(), 150, "q", label_destchar="h", mask_token=2 ** 40 + 3, ignore_index=-7, frac=0.5, form=form)
        assert (ins.view(np.int64) == 2 ** 40 + 3).sum() > 200 and (lab == -7).sum() > 200
    _check(gpu, v, _type_rows(), 150, "i", label_destchar="q", mask_token=0, ignore_index=2 ** 62, mask_prob=0.3, random_prob=0.7)


def test_refused_calls_leave_the_outputs_untouched(gpu, bsq):
    import torch
    from bioseq_amd import bpe, capi
    L = capi.load()
    v = _trained()  # vocab 205
    chars, offs = twin.pack(_edge_rows()[:12])
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    B, P = len(offs) - 1, 16
    table = v.device_table(gpu)
    nan = float("nan")

    def call(in_dt=capi.I16, lab_dt=capi.I16, max_chars=1024, form=0, reserved=0, M=v.M, tab=table.data_ptr(), padlen=P, rows=B, m="default",
             frac=0.15, mask_prob=0.8, random_prob=0.1, mask_token=205, ignore=-100, first_row=0, no_in=False, no_lab=False, no_len=False):
        ins = torch.full((B * P * 8,), 0x5A, dtype=torch.uint8, device=gpu)
        lab = torch.full((B * P * 8,), 0x5A, dtype=torch.uint8, device=gpu)
        lens = torch.full((B * 4,), 0x5A, dtype=torch.uint8, device=gpu)
        mm = capi.BpeMlm(frac, mask_prob, random_prob, mask_token, ignore, 1, first_row)
        st = L.bsq_bpe_mlm_tokenize_device(ctypes.byref(v.desc), dch.data_ptr(), dof.data_ptr(), rows, padlen, 1, tab, M,
                                           ctypes.byref(capi.Bpe(max_chars, form, reserved)), ctypes.byref(mm) if m == "default" else None, in_dt,
                                           None if no_in else ins.data_ptr(), lab_dt, None if no_lab else lab.data_ptr(),
                                           None if no_len else lens.data_ptr(), None)
        torch.cuda.synchronize()
        return st, bool((ins == 0x5A).all()), bool((lab == 0x5A).all()), bool((lens == 0x5A).all())

    assert call() == (capi.OK, False, False, False)
    for kw in (dict(max_chars=0), dict(max_chars=8193), dict(max_chars=1025, form=1), dict(form=3), dict(reserved=1), dict(M=70000), dict(tab=None),
               dict(padlen=0), dict(rows=-1), dict(no_len=True),
               dict(m=None), dict(frac=-0.1), dict(frac=1.5), dict(frac=nan), dict(mask_prob=nan), dict(random_prob=1.01),
               dict(mask_prob=0.7, random_prob=0.4), dict(first_row=-1), dict(mask_token=-1), dict(no_in=True, no_lab=True)):
        assert call(**kw) == (capi.ERR_INVALID_ARG, True, True, True), kw
        assert L.bsq_last_error()
    for kw in (dict(in_dt=capi.I8), dict(mask_token=40000), dict(in_dt=capi.F32, mask_token=2 ** 24 + 1), dict(lab_dt=capi.I8),
               dict(ignore=-40000), dict(lab_dt=9)):
        assert call(**kw) == (capi.ERR_DTYPE, True, True, True), kw
    assert call(rows=0) == (capi.OK, True, True, True)  # B == 0: nothing launched
    got = bpe.bpe_mlm_tokenize_packed(v, dch[:0], dof[:1], 5)
    assert tuple(got[0].shape) == tuple(got[1].shape) == (0, 5) and tuple(got[2].shape) == (0,)
    for kw in (dict(destchar="b"), dict(label_destchar="b"), dict(max_chars=1025, form=1), dict(frac=2.0), dict(first_row=-1)):
        with pytest.raises(ValueError):
            bpe.bpe_mlm_tokenize_packed(v, dch, dof, P, kw.pop("destchar", "h"), **kw)
    with pytest.raises(ValueError):
        bpe.bpe_mlm_tokenize_packed(v, chars, offs, P)  # host arrays


def test_a_store_that_ends_with_its_allocation(gpu, bsq):
    """The last row ends exactly at offsets[B] and the character tensor holds not one byte more: no read goes past it."""
    import torch
    from bioseq_amd import bpe
    v = _trained()
    rng = np.random.default_rng(21)
    for last in (1, 15, 16, 17, 1024):
        rows = [twin.random_row(rng, 33, "ACGT"), twin.random_row(rng, last, "ACGT")]
        chars, offs = twin.pack(rows)
        dch = torch.empty(int(offs[-1]), dtype=torch.uint8, device=gpu)
        dch.copy_(torch.from_numpy(chars))
        assert dch.numel() == offs[-1]
        got = bpe.bpe_mlm_tokenize_packed(v, dch, _dev(offs, gpu), 600, "i", frac=0.3, seed=5, max_chars=1024)
        exp = bpe.bpe_mlm_tokenize_host(v, chars, offs, 600, "i", frac=0.3, seed=5)
        assert all(g.cpu().numpy().tobytes() == e.tobytes() for g, e in zip(got, exp))


def test_the_dataset_options(gpu, bsq, tmp_path):
    import torch
    from bioseq_amd import bpe
    from bioseq_amd.flatfile import FlatFile, write_flatfile
    from bioseq_amd.loaders import FlatFileDataset
    rng = np.random.default_rng(2)
    lens = rng.integers(0, 300, 150)
    lens[:3] = (0, 5, 700)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGTACGTACGTACGTNacgt", np.uint8), int(n))) for n in lens]
    ff = FlatFile(write_flatfile(seqs, str(tmp_path / "bpe.ff")))
    flags = (True, True, True)
    v = _trained(flags)
    tok = _tok("DNA4", *flags)
    chars, offs = twin.pack(seqs)
    mask_key = (13 * 0x9E3779B97F4A7C15 + 1) & (2 ** 64 - 1)  # the dataset's first mask key (seed 13)

    # bpe_mlm=False: bpe_tokenize_packed's tokens, from every access path
    ds = FlatFileDataset(ff, tok, device=gpu, bpe=v, token_dtype="i")
    assert ds.max_seq_len == 702
    want = bpe.bpe_tokenize_host(v, chars, offs, 702, "i", max_chars=700)[0]
    assert np.array_equal(ds.get_batch(0, 150).cpu().numpy(), want) and np.array_equal(ds[2].cpu().numpy(), want[2])
    assert np.array_equal(ds.__getitems__([5, 3, 9]).cpu().numpy(), want[[5, 3, 9]])
    got = torch.cat(list(ds.batches(64, shuffle=False, group=2)))
    assert np.array_equal(got.cpu().numpy(), want)
    ds = FlatFileDataset(ff, tok, device=gpu, bpe=v, bpe_padlen=50, token_dtype="h")
    assert ds.max_seq_len == 50 and np.array_equal(ds.get_batch(0, 150).cpu().numpy(), bpe.bpe_tokenize_host(v, chars, offs, 50, "h")[0])

    # bpe_mlm=True: get_batch is the direct call with the dataset's key
    ds = FlatFileDataset(ff, tok, device=gpu, bpe=v, bpe_mlm=True, token_dtype="i", maskfrac=0.2)
    gi, gl = ds.get_batch(10, 90)
    di, dl, _ = bpe.bpe_mlm_tokenize_packed(v, _dev(chars[offs[10]:offs[90]], gpu), _dev(offs[10:91] - offs[10], gpu), 702, "i", frac=0.2,
                                            seed=mask_key, max_chars=700)
    assert gi.dtype == torch.int32 and gl.dtype == torch.int64 and torch.equal(gi, di) and torch.equal(gl, dl) and bool((gl != -100).any())
    a, b = ds[1]
    assert a.shape == b.shape == (702,)
    x3, y3 = ds.__getitems__([5, 3, 9])
    assert x3.shape == y3.shape == (3, 702)

    def epoch(**opts):
        d = FlatFileDataset(ff, tok, device=gpu, bpe=v, bpe_mlm=True, token_dtype="i", maskfrac=0.2, crop=opts.pop("crop", None),
                            revcomp_frac=opts.pop("revcomp_frac", 0.0))
        g = torch.Generator(device=gpu).manual_seed(5)
        out = [(p.clone(), q.clone()) for p, q in d.batches(32, generator=g, **opts)]
        torch.cuda.synchronize()
        return out

    base = epoch(shuffle=False)
    ei, el, _ = bpe.bpe_mlm_tokenize_host(v, chars, offs, 702, "i", frac=0.2, seed=mask_key, max_chars=700)
    assert len(base) == 5 and np.array_equal(torch.cat([p for p, _ in base]).cpu().numpy(), ei)
    assert np.array_equal(torch.cat([q for _, q in base]).cpu().numpy(), el.view(np.int64))
    for kw in (dict(shuffle=False), dict(shuffle=True), dict(shuffle=True, crop=128, revcomp_frac=0.5)):
        one = epoch(**kw)
        for opts in (dict(group=2), dict(prefetch=2), dict(group=2, prefetch=2)):
            got = epoch(**kw, **opts)
            assert len(got) == len(one) and all(torch.equal(p, r) and torch.equal(q, s) for (p, q), (r, s) in zip(one, got)), (kw, opts)
    assert one[0][0].shape == (32, 130)

    # the refused combinations
    for kw in (dict(cnn=True), dict(augment=1), dict(masked=True), dict(kmer=3), dict(pack="stream"), dict(spectrum=3)):
        with pytest.raises(ValueError):
            FlatFileDataset(ff, tok, device=gpu, bpe=v, **kw)
    with pytest.raises(ValueError):
        FlatFileDataset(ff, tok, device=gpu, bpe_mlm=True)
    with pytest.raises(ValueError):
        FlatFileDataset(ff, _tok("DNA4"), device=gpu, bpe=v)  # the vocabulary is over another tokenizer (flags)
    with pytest.raises(ValueError):
        FlatFileDataset(ff, tok, device=gpu, bpe=v, token_dtype="b")
    with pytest.raises(ValueError):
        FlatFileDataset(ff, tok, device=gpu, bpe=v, bpe_padlen=0)
    long_ff = FlatFile(write_flatfile([b"A" * 9000, b"ACGT"], str(tmp_path / "long.ff")))
    with pytest.raises(ValueError, match="crop="):
        FlatFileDataset(long_ff, tok, device=gpu, bpe=v)
    assert FlatFileDataset(long_ff, tok, device=gpu, bpe=v, crop=512).max_seq_len == 514
    short = FlatFile(str(tmp_path / "long.ff"), maxseqlen=100)  # lengths not trusted: the too-long row raises
    ds = FlatFileDataset(short, tok, device=gpu, bpe=v, bpe_mlm=True)
    with pytest.raises(RuntimeError):
        ds.get_batch(0, 2)
    assert ds.get_batch(1, 2)[0].shape == (1, 102)
