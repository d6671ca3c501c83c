"""GPU: masked-LM batches on the device (bioseq_amd.masking, bsq_mlm_tokenize_device / bsq_random_mask_device) against the oracle's
plain tokens / one-hot with the numpy twin's draw applied (tests/mlm_twin.py), and the masked FlatFileDataset."""
import ctypes

import numpy as np
import pytest

import mlm_twin as twin
from bioseq_amd import synth

pytestmark = pytest.mark.gpu

DTYPES = {"b": (np.int8, 0), "h": (np.int16, 1), "i": (np.int32, 2), "q": (np.int64, 3), "f": (np.float32, 4), "d": (np.float64, 5)}
GUARD = 64  # elements of sentinel in front of and behind every output


def _packed(rng, B, room, unmapped=True):
    lens = rng.integers(0, room + 1, B) if room > 0 else np.zeros(B, np.int64)
    if B:
        lens[0] = min(room, max(room, 0))  # one full-length sequence
    pool = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYXBZ*acgt" if unmapped else b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    chars = rng.choice(pool, int(lens.sum())).astype(np.uint8)
    offsets = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    return chars, offsets


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _lut(key):
    from bioseq_amd import capi
    return np.frombuffer(bytes(capi.make_desc(key).lut), dtype=np.int8)


def _guarded_call(tok, dch, doffs, B, P, batch_first, m, in_code, lab_code, in_np, lab_np, stream=None):
    """bsq_mlm_tokenize_device into buffers with GUARD sentinel elements on both sides; returns the two outputs, checks the guards."""
    import torch
    from bioseq_amd import capi
    L = capi.load()
    n = B * P
    bufs = []
    for np_t in (in_np, lab_np):
        t = torch.from_numpy(np.zeros(0, np_t)).dtype
        buf = torch.empty(n + 2 * GUARD, dtype=t, device=dch.device)
        buf.view(torch.uint8).fill_(0xA5)
        bufs.append(buf)
    desc = capi.make_desc(tok.key, tok.includes_eos(), tok.includes_bos(), tok.is_padded())
    chars_ptr = dch.data_ptr() if dch.numel() else bufs[0].data_ptr()
    st = L.bsq_mlm_tokenize_device(ctypes.byref(desc), chars_ptr, doffs.data_ptr(), B, P, int(batch_first), ctypes.byref(m), in_code,
                                   bufs[0].data_ptr() + GUARD * bufs[0].element_size(), lab_code,
                                   bufs[1].data_ptr() + GUARD * bufs[1].element_size(), stream if stream is not None else capi.raw_stream(dch.device))
    capi.check(st)
    torch.cuda.synchronize()
    outs = []
    for buf in bufs:
        raw = buf.view(torch.uint8).cpu().numpy()
        es = buf.element_size()
        assert (raw[: GUARD * es] == 0xA5).all() and (raw[(GUARD + n) * es:] == 0xA5).all(), "an output guard was overwritten"
        outs.append(buf[GUARD: GUARD + n].cpu().numpy())
    return outs


@pytest.mark.parametrize("key, flags", [("AMINO20", (0, 0, 0)), ("AMINO20", (1, 1, 1)), ("DNA", (1, 0, 1)), ("SEB8", (0, 1, 0))])
@pytest.mark.parametrize("P", [1, 15, 16, 17, 511, 512, 1000])
def test_mlm_tokenize_every_dtype_pair_and_layout(gpu, bsq, oracle, key, flags, P):
    from bioseq_amd import capi
    eos, bos, pad = flags
    tok = bsq.Tokenizer(key, eos, bos, pad)
    ora = oracle.OracleTokenizer(key, eos, bos, pad)
    room = P - bos - eos
    rng = np.random.default_rng(P * 31 + sum(flags))
    lut = _lut(key)
    for B in (0, 1, 255, 4097):
        if room < 0:
            continue
        chars, offs = _packed(rng, B, room)
        plain = ora.tokenize_packed(chars, offs, P, "i", True).astype(np.int64) if B else np.zeros((0, P), np.int64)
        seed, first_row = int(rng.integers(0, 2 ** 62)), int(rng.integers(0, 1000))
        frac, mp, rp = 0.3, 0.6, 0.25
        mtok = tok.alphabet_size()
        m = capi.Mlm(frac, mp, rp, mtok, -100, seed, first_row)
        exp_in, exp_lab = twin.mlm(plain, lut, ora.nchars(), bos, eos, chars, offs, frac, mp, rp, mtok, -100, seed, first_row)
        dch, doffs = _dev(chars, gpu), _dev(offs, gpu)
        pairs = [(a, b) for a in DTYPES for b in DTYPES] if B * P <= 300000 else [("b", "b"), ("b", "q"), ("q", "q"), ("f", "d"), ("h", "i")]
        for in_ch, lab_ch in pairs:
            (in_np, in_code), (lab_np, lab_code) = DTYPES[in_ch], DTYPES[lab_ch]
            for bf in (True, False):
                got_in, got_lab = _guarded_call(tok, dch, doffs, B, P, bf, m, in_code, lab_code, in_np, lab_np)
                want_in, want_lab = exp_in.astype(in_np), exp_lab.astype(lab_np)
                if not bf:
                    want_in, want_lab = want_in.T, want_lab.T
                assert np.array_equal(got_in, want_in.ravel()), (B, in_ch, lab_ch, bf)
                assert np.array_equal(got_lab, want_lab.ravel()), (B, in_ch, lab_ch, bf)


def test_python_api_equals_twin_and_bytes_alphabet(gpu, bsq, oracle):
    from bioseq_amd import masking
    rng = np.random.default_rng(8)
    for key, flags in (("BYTES", (1, 1, 1)), ("AMINO20", (0, 0, 0))):
        tok, ora = bsq.Tokenizer(key, *flags), oracle.OracleTokenizer(key, *flags)
        P = 300
        chars, offs = _packed(rng, 700, P - 2 * flags[0])
        if key == "BYTES":
            chars = rng.integers(0, 256, len(chars)).astype(np.uint8)
        inputs, labels = masking.mlm_tokenize_packed(tok, _dev(chars, gpu), _dev(offs, gpu), P, "i", True, frac=0.2, seed=5, first_row=3)
        plain = ora.tokenize_packed(chars, offs, P, "i", True).astype(np.int64)
        ei, el = twin.mlm(plain, _lut(key), ora.nchars(), flags[1], flags[0], chars, offs, 0.2, 0.8, 0.1, tok.alphabet_size(), -100, 5, 3)
        assert np.array_equal(inputs.cpu().numpy(), ei.astype(np.int32)) and np.array_equal(labels.cpu().numpy(), el)


def test_random_mask_equals_twin(gpu, bsq):
    from bioseq_amd import masking
    rng = np.random.default_rng(2)
    for key in ("AMINO20", "DNA", "BYTES"):
        tok = bsq.Tokenizer(key)
        for B, room in ((1, 1), (3, 0), (500, 40), (3000, 600)):
            chars, offs = _packed(rng, B, room)
            seed, first_row, frac = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 5000)), float(rng.random())
            got = masking.random_mask_packed(tok, _dev(chars, gpu), _dev(offs, gpu), frac=frac, seed=seed, first_row=first_row)
            assert np.array_equal(got.cpu().numpy(), twin.mask(_lut(key), chars, offs, frac, seed, first_row)), (key, B, room)


def test_frac_zero_and_frac_one(gpu, bsq):
    import torch
    from bioseq_amd import masking
    rng = np.random.default_rng(4)
    tok = bsq.Tokenizer("AMINO20", 1, 1, 1)
    P = 257
    chars, offs = _packed(rng, 999, P - 2)
    dch, doffs = _dev(chars, gpu), _dev(offs, gpu)
    for dt in ("b", "q", "f"):
        plain = tok.tokenize_packed(dch, doffs, P, dt, True)
        inp, lab = masking.mlm_tokenize_packed(tok, dch, doffs, P, dt, True, frac=0.0, seed=1)
        assert torch.equal(inp, plain) and bool((lab == -100).all())
        inp, lab = masking.mlm_tokenize_packed(tok, dch, doffs, P, dt, True, frac=1.0, mask_prob=1.0, random_prob=0.0, seed=1)
        mapped = torch.from_numpy(_lut("AMINO20")[chars] >= 0)
        mapped_pos = np.zeros((999, P), bool)
        lens = np.diff(offs)
        for i in range(999):
            mapped_pos[i, 1:1 + lens[i]] = mapped[offs[i]:offs[i + 1]].numpy()
        mp = torch.from_numpy(mapped_pos).to(gpu)
        assert bool((inp[mp] == tok.alphabet_size()).all()) and torch.equal(inp[~mp], plain[~mp])
        assert torch.equal(lab[mp].to(torch.int64), plain[mp].to(torch.int64)) and bool((lab[~mp] == -100).all())


@pytest.mark.parametrize("layout", ["tbc", "bcl"])
def test_onehot_masked_equals_oracle_with_twin_mask(gpu, bsq, oracle, layout):
    from bioseq_amd import masking
    rng = np.random.default_rng(6)
    tok, ora = bsq.Tokenizer("AMINO20", 0, 1, 1), oracle.OracleTokenizer("AMINO20", 0, 1, 1)
    P = 200
    chars, offs = _packed(rng, 333, P - 1)
    onehot, labels = masking.onehot_masked_packed(tok, _dev(chars, gpu), _dev(offs, gpu), P, "f", layout, frac=0.25, seed=77, first_row=10)
    mask = twin.mask(_lut("AMINO20"), chars, offs, 0.25, 77, 10)
    exp = ora.onehot_packed(chars, offs, P, "f", mask=mask)  # (P, B, C)
    got = onehot.cpu().numpy()
    if layout == "bcl":
        got = got.transpose(2, 0, 1)  # (B, C, P) -> (P, B, C)
    assert np.array_equal(got, exp)
    plain = ora.tokenize_packed(chars, offs, P, "i", True).astype(np.int64)
    _, el = twin.mlm(plain, _lut("AMINO20"), ora.nchars(), 1, 0, chars, offs, 0.25, 0.8, 0.1, 0, -100, 77, 10)
    assert np.array_equal(labels.cpu().numpy(), el)
    # the zeroed one-hot rows are exactly the labelled positions
    zero_rows = exp.sum(axis=2).T == 0
    assert zero_rows[el != -100].all()


def test_shard_invariance_and_non_default_stream(gpu, bsq):
    import torch
    from bioseq_amd import masking
    rng = np.random.default_rng(9)
    tok = bsq.Tokenizer("AMINO20")
    P = 128
    chars, offs = _packed(rng, 2000, P)
    dch, doffs = _dev(chars, gpu), _dev(offs, gpu)
    whole = masking.mlm_tokenize_packed(tok, dch, doffs, P, "b", True, seed=3)
    wmask = masking.random_mask_packed(tok, dch, doffs, frac=0.15, seed=3)
    split = 613
    lo_c, lo_o = dch[: int(offs[split])].contiguous(), doffs[: split + 1].contiguous()
    hi_c, hi_o = dch[int(offs[split]):].contiguous(), (doffs[split:] - int(offs[split])).contiguous()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        a = masking.mlm_tokenize_packed(tok, lo_c, lo_o, P, "b", True, seed=3)
        b = masking.mlm_tokenize_packed(tok, hi_c, hi_o, P, "b", True, seed=3, first_row=split)
        ma = masking.random_mask_packed(tok, lo_c, lo_o, frac=0.15, seed=3)
        mb = masking.random_mask_packed(tok, hi_c, hi_o, frac=0.15, seed=3, first_row=split)
    s.synchronize()
    assert torch.equal(torch.cat([a[0], b[0]]), whole[0]) and torch.equal(torch.cat([a[1], b[1]]), whole[1])
    assert torch.equal(torch.cat([ma, mb]), wmask)
    # and the layout does not change a character's fate
    sf = masking.mlm_tokenize_packed(tok, dch, doffs, P, "q", False, label_dtype="b", seed=3)
    assert torch.equal(sf[0].t().to(torch.int8), whole[0]) and torch.equal(sf[1].t().to(torch.int64), whole[1])


def _store(tmp_path, n=2100):
    from bioseq_amd.flatfile import FlatFile, write_flatfile
    chars, offs = synth.synth_packed(31, n, 0, 150, synth.AA)
    return FlatFile(write_flatfile(synth.unpack(chars, offs), str(tmp_path / "mlm.ff")))


def test_masked_loader_group_prefetch_and_agreement(gpu, bsq, tmp_path):
    import torch
    from bioseq_amd.loaders import FlatFileDataset
    ff = _store(tmp_path)
    tok = bsq.Tokenizer("AMINO20", 1, 1, 1)

    def epoch(masked, **opts):
        ds = FlatFileDataset(ff, tok, device=gpu, masked=masked, maskfrac=0.2, token_dtype="q")
        g = torch.Generator(device=gpu).manual_seed(5)
        out = [tuple(t.clone() for t in b) if masked else b.clone() for b in ds.batches(256, generator=g, **opts)]
        torch.cuda.synchronize()
        return out

    base = epoch(True)
    plain = epoch(False)
    assert len(base) == len(plain) == 9
    for opts in ({"group": 4}, {"group": 4, "prefetch": 2}, {"prefetch": 1}):
        got = epoch(True, **opts)
        assert len(got) == len(base)
        for (a, b), (c, d) in zip(base, got):
            assert torch.equal(a, c) and torch.equal(b, d), opts
    selected = 0
    for (inp, lab), p in zip(base, plain):
        keep = lab == -100
        assert torch.equal(inp[keep], p[keep])  # unselected positions: the unmasked loader's tokens
        assert torch.equal(lab[~keep], p[~keep])  # selected: the label is the plain token
        selected += int((~keep).sum())
    assert selected > 0
    # a rebuilt dataset repeats its masks; the next epoch of the same dataset draws new ones
    ds = FlatFileDataset(ff, tok, device=gpu, masked=True, maskfrac=0.2)
    e1 = [b[1].clone() for b in ds.batches(256, shuffle=False)]
    e2 = [b[1].clone() for b in ds.batches(256, shuffle=False)]
    assert not all(torch.equal(x, y) for x, y in zip(e1, e2))
    ds2 = FlatFileDataset(ff, tok, device=gpu, masked=True, maskfrac=0.2)
    assert all(torch.equal(x, y[1]) for x, y in zip(e1, ds2.batches(256, shuffle=False)))
    # get_batch / __getitems__ / indexing return the pair
    inp, lab = ds.get_batch(0, 10)
    assert inp.shape == lab.shape == (10, ds.max_seq_len)
    inp, lab = ds.__getitems__([5, 3, 9])
    assert inp.shape == (3, ds.max_seq_len) and lab.dtype == torch.int64
    inp, lab = ds[4]
    assert inp.shape == (ds.max_seq_len,)


def test_masked_loader_cnn_returns_onehot_and_labels(gpu, bsq, tmp_path):
    import torch
    from bioseq_amd.loaders import FlatFileDataset
    ff = _store(tmp_path, n=700)
    tok = bsq.Tokenizer("AMINO20", 0, 0, 1)
    ds = FlatFileDataset(ff, tok, device=gpu, masked=True, cnn=True, maskfrac=0.3)
    plain_ds = FlatFileDataset(ff, tok, device=gpu, cnn=True)
    plain_tok = FlatFileDataset(ff, tok, device=gpu)
    g = torch.Generator(device=gpu).manual_seed(1)
    batches = list(ds.batches(100, generator=g, group=2))
    g = torch.Generator(device=gpu).manual_seed(1)
    plain = list(plain_ds.batches(100, generator=g))
    g = torch.Generator(device=gpu).manual_seed(1)
    toks = list(plain_tok.batches(100, generator=g))
    assert len(batches) == 7
    for (oh, lab), p, t in zip(batches, plain, toks):
        assert oh.shape == p.shape and oh.dtype == torch.float32 and lab.shape == t.shape
        sel = lab != -100
        rows_zero = oh.sum(dim=1) == 0
        assert bool(rows_zero[sel].all()) and torch.equal(lab[sel], t[sel])
        assert torch.equal(oh.permute(0, 2, 1)[~sel], p.permute(0, 2, 1)[~sel])


def test_masked_loader_with_augmentation(gpu, bsq, tmp_path):
    import torch
    from bioseq_amd.loaders import FlatFileDataset
    ff = _store(tmp_path, n=600)
    tok = bsq.Tokenizer("AMINO20")
    ds = FlatFileDataset(ff, tok, device=gpu, masked=True, augment=2, augment_frac=1.0, token_dtype="b")
    inp, lab = ds.get_batch(0, 600)
    assert inp.dtype == torch.int8 and lab.dtype == torch.int64 and inp.shape == (600, ds.max_seq_len)
    # the resident store is untouched by the augmentation
    chars, offs = ff.packed_device(0, 600, gpu)
    before = chars.clone()
    ds.get_batch(0, 600)
    torch.cuda.synchronize()
    assert torch.equal(chars, before)
