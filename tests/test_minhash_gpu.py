"""GPU: MinHash sketches of packed batches (bioseq_amd.sketch.minhash_packed, bsq_minhash_device) and the all-pairs comparison
(sketch_compare, bsq_sketch_compare_device) against the numpy twin (tests/minhash_twin.py) and the library's host twins, byte for byte,
on shapes that reach both kernel forms, every rolling mode and their boundaries; the two forms against each other; the layout guards; the
Python surface."""
import ctypes

import numpy as np
import pytest

import minhash_twin as twin

pytestmark = pytest.mark.gpu

I32, U64 = 2, 3
CODE = {"i": I32, "q": U64}
WAVE, BLOCK = "k_minhash_wave", "k_minhash_block<%d>"
# (about 4 % unmapped bytes -- N, lower case, * and \xff: at k = 32 a quarter of the windows is still whole)
POOLS = {
    "DNA4": b"ACGT" * 25 + b"Na*\xff",
    "DNA5": b"ACGTN" * 20 + b"ag*\xff",
    "AMINO20": b"ACDEFGHIKLMNPQRSTVWY" * 5 + b"XBZ*a",
    "PURPYR": b"ACGTRY" * 12 + b"*N\xc1",
}
DNA_KS = [1, 3, 16, 17, 21, 31, 32]


def _lut(key):
    from bioseq_amd import capi
    lut = (ctypes.c_int8 * 256)()
    n = ctypes.c_int32(0)
    assert capi.load().bsq_lut_get(key.encode(), lut, ctypes.byref(n)) == capi.OK
    return np.array(lut, dtype=np.int8), n.value


def _batch(rng, key, lens):
    """Packed batch of rows of the given lengths; the LAST row ends at the last byte of chars (the guarded tail loads)."""
    lens = np.asarray(lens, dtype=np.int64)
    chars = rng.choice(np.frombuffer(POOLS[key], np.uint8), int(lens.sum())).astype(np.uint8)
    offs = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    assert offs[-1] == chars.size
    return chars, offs


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _tok(bsq, key):
    return bsq.Tokenizer(key, False, False, False)


def _check(bsq, gpu, key, chars, offs, k, widths, dcs=("i", "q"), canonical=False, seed=0, forms=(None,), kernel=None, dev=None):
    """minhash_packed == the numpy twin == the library's host twin, byte for byte, for every width, element type and form; the filled
    buckets of the batch (a check of nothing but EMPTY would be vacuous: callers assert on it)."""
    import torch
    from bioseq_amd import sketch
    tok = _tok(bsq, key)
    lut, A = _lut(key)
    dch, dof = dev if dev is not None else (_dev(chars, gpu), _dev(offs, gpu))
    B = len(offs) - 1
    hashes = twin.batch_hashes(lut, A, chars, offs, k, canonical, seed)
    filled = 0
    for S in widths:
        for dc in dcs:
            exp = twin.sketch(lut, A, chars, offs, k, S, CODE[dc], canonical, seed, hashes=hashes)
            host = sketch.minhash_host(tok, chars, offs, k, S, dc, canonical=canonical, seed=seed)
            assert host.tobytes() == exp.tobytes(), (key, k, S, dc, canonical)
            filled += int((exp.view(np.int32 if dc == "i" else np.int64) != -1).sum())
            for form in forms:
                if kernel is not None:
                    assert sketch.minhash_kernel_name(tok, k, B, S, dc, canonical=canonical, form=form, total_chars=chars.size) == kernel
                got = sketch.minhash_packed(tok, dch, dof, k, S, dc, canonical=canonical, seed=seed, form=form, validate=False)
                torch.cuda.synchronize()
                assert got.shape == (B, S) and got.is_contiguous() and got.dtype == (torch.int32 if dc == "i" else torch.int64)
                assert got.cpu().numpy().tobytes() == exp.tobytes(), (key, k, S, dc, canonical, form)
    return filled


@pytest.mark.parametrize("k", DNA_KS)
@pytest.mark.parametrize("B", [1, 3, 5, 257])
def test_wave_form_equals_the_twins(gpu, bsq, k, B):
    """DNA4 at S = 1, 3, 64, 1000, 1024 (3 and 1000 with 'i': rows that are not 16-byte aligned, the element stores).  Random lengths
    0 .. 700 with rows pinned on the lane-run (16 windows), 64-window and wave-sweep (64 x 16 windows) boundaries; B = 1, 3, 5: rows that
    do not fill four waves, B = 257: a partial last workgroup."""
    rng = np.random.default_rng(k * 1000 + B)
    lens = rng.integers(0, 701, B)
    pins = {1: [16 * 64 + k - 1], 3: [0, 63 + k, 64 + k], 5: [0, k - 1, k, 63 + k, 16 * 64 + k - 1],
            257: [0, k - 1, k, 15 + k, 16 + k, 63 + k, 64 + k, 16 * 64 + k - 1, 16 * 64 + k]}[B]
    lens[:len(pins)] = pins
    if B == 257:
        lens[-1] = 700
    chars, offs = _batch(rng, "DNA4", lens)
    assert _check(bsq, gpu, "DNA4", chars, offs, k, (1, 3, 64, 1000, 1024), kernel=WAVE) > 10


@pytest.mark.parametrize("k", [3, 21, 32])
@pytest.mark.parametrize("S, form, bins", [(1025, None, 4096), (4096, None, 4096), (16384, None, 16384), (64, 2, 1024)])
@pytest.mark.parametrize("B", [1, 3])
def test_block_form_equals_the_twins(gpu, bsq, k, S, form, bins, B):
    """Rows of one piece (256 x 16 windows) less one window, exactly, plus one; and a row of several pieces."""
    rng = np.random.default_rng(S + B + k)
    lens = [20011] if B == 1 else [4096 + k - 2, 4096 + k - 1, 4096 + k]
    chars, offs = _batch(rng, "DNA4", lens)
    assert _check(bsq, gpu, "DNA4", chars, offs, k, (S,), forms=(form,), kernel=BLOCK % bins) > 10


@pytest.mark.parametrize("key, k", [("DNA5", 27), ("AMINO20", 1), ("AMINO20", 7), ("AMINO20", 14), ("PURPYR", 32)])
def test_other_alphabets(gpu, bsq, key, k):
    """The rolling word by multiplication (any alphabet but the four-class ones), up to the largest k of each alphabet."""
    rng = np.random.default_rng(k)
    chars, offs = _batch(rng, key, [0, k, 700, 16 * 64 + k, 333])
    assert _check(bsq, gpu, key, chars, offs, k, (64, 1000), forms=(1, 2)) > 100


@pytest.mark.parametrize("k", [1, 4, 21, 31, 32])
def test_canonical_and_strand_invariance(gpu, bsq, k):
    """k = 4 meets words that are their own reverse complement.  A batch and its reverse complement have equal canonical sketches."""
    import torch
    from bioseq_amd import sketch
    rng = np.random.default_rng(40 + k)
    lens = rng.integers(0, 701, 37)
    lens[:5] = (0, k - 1, k, 16 * 64 + k, 4096 + k)
    chars, offs = _batch(rng, "DNA4", lens)
    dev = _dev(chars, gpu), _dev(offs, gpu)
    assert _check(bsq, gpu, "DNA4", chars, offs, k, (64, 1000), canonical=True, seed=3, forms=(1, 2), dev=dev) > 100
    rc = np.concatenate([twin.revcomp(chars[offs[i]:offs[i + 1]]) for i in range(37)])
    tok = _tok(bsq, "DNA4")
    for form in (1, 2):
        fwd = sketch.minhash_packed(tok, *dev, k, 256, canonical=True, form=form)
        rev = sketch.minhash_packed(tok, _dev(rc, gpu), dev[1], k, 256, canonical=True, form=form)
        assert torch.equal(fwd, rev), (k, form)
        if k > 1:
            assert not torch.equal(sketch.minhash_packed(tok, *dev, k, 256, form=form), sketch.minhash_packed(tok, _dev(rc, gpu), dev[1], k, 256, form=form))


def test_both_forms_agree(gpu, bsq):
    import torch
    from bioseq_amd import sketch
    rng = np.random.default_rng(11)
    for key, k, canonical in (("DNA4", 21, True), ("DNA4", 32, False), ("AMINO20", 7, False)):
        tok = _tok(bsq, key)
        lens = rng.integers(0, 3000, 41)
        lens[:3] = (0, k, 5000)
        chars, offs = _batch(rng, key, lens)
        dch, dof = _dev(chars, gpu), _dev(offs, gpu)
        for S in (1, 100, 1024):
            for dc in ("i", "q"):
                a = sketch.minhash_packed(tok, dch, dof, k, S, dc, canonical=canonical, form=1)
                b = sketch.minhash_packed(tok, dch, dof, k, S, dc, canonical=canonical, form=2)
                c = sketch.minhash_packed(tok, dch, dof, k, S, dc, canonical=canonical)
                torch.cuda.synchronize()
                assert torch.equal(a, b) and torch.equal(a, c), (key, k, S, dc)


def test_one_bucket_and_empty_rows(gpu, bsq):
    """5 000 A: every window of every lane falls on one bucket; a row of nothing but unmapped bytes and an empty row are all EMPTY."""
    from bioseq_amd import sketch
    chars = np.frombuffer(b"A" * 5000 + b"N" * 3000 + b"n*\xff" * 100 + b"AC" * 2500, dtype=np.uint8).copy()
    offs = np.array([0, 5000, 8000, 8300, 8300, 13300], dtype=np.int64)
    dev = _dev(chars, gpu), _dev(offs, gpu)
    tok = _tok(bsq, "DNA4")
    for k in (4, 21):
        for canonical in (False, True):
            _check(bsq, gpu, "DNA4", chars, offs, k, (64, 1024, 4096), canonical=canonical, forms=(None, 2), dev=dev)
            for form, S in ((1, 64), (2, 64), (2, 4096)):
                got = sketch.minhash_packed(tok, *dev, k, S, "q", canonical=canonical, form=form).cpu().numpy()
                assert (got[0] != -1).sum() == 1 and (got[1:4] == -1).all() and (got[4] != -1).sum() in (1, 2)


def test_write_once_guards_and_a_sub_batch(gpu, bsq):
    """The raw entry point on a batch inside a larger buffer (offsets[0] > 0), into the middle of a 0x5A-filled output, on a side stream:
    every byte of the (B, S) block is written -- EMPTY included --, the guards stay; B == 0 launches nothing; a refusal writes nothing."""
    import torch
    from bioseq_amd import capi
    L = capi.load()
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 90, 133)
    lens[:3] = (0, 21, 4200)
    chars, offs = _batch(rng, "DNA4", lens)
    lead = 7
    big = np.concatenate([np.full(lead, ord("A"), np.uint8), chars])
    offs = offs + lead
    dch, dof = _dev(big, gpu), _dev(offs, gpu)
    d = capi.make_desc("DNA4", eos=True, bos=True, padchar=True)  # (BOS, EOS and PAD play no part)
    lut, A = _lut("DNA4")
    side = torch.cuda.Stream(device=gpu)
    B, guard = 133, 256
    for k, S, form, dt, canonical, skew in ((21, 64, 1, I32, 1, 0), (21, 3, 1, I32, 0, 4), (5, 1000, 2, U64, 0, 8), (32, 4096, 0, I32, 1, 0), (3, 1, 0, U64, 0, 8)):
        m = capi.MinHash(k, S, canonical, form, 77, big.size, 0)
        size = 4 if dt == I32 else 8
        n = B * S * size
        buf = torch.full((n + 2 * guard + skew,), 0x5A, dtype=torch.uint8, device=gpu)
        side.wait_stream(torch.cuda.current_stream())
        capi.check(L.bsq_minhash_device(ctypes.byref(d), dch.data_ptr(), dof.data_ptr(), B, ctypes.byref(m), dt, buf.data_ptr() + guard + skew,
                                        ctypes.c_void_p(side.cuda_stream)))
        side.synchronize()
        raw = buf.cpu().numpy()
        assert (raw[:guard + skew] == 0x5A).all() and (raw[guard + skew + n:] == 0x5A).all(), "a guard byte of out was overwritten"
        exp = twin.sketch(lut, A, big, offs, k, S, dt, bool(canonical), 77)
        assert raw[guard + skew:guard + skew + n].tobytes() == exp.tobytes(), (k, S, form, dt)
        capi.check(L.bsq_minhash_device(ctypes.byref(d), dch.data_ptr(), dof.data_ptr(), 0, ctypes.byref(m), dt, buf.data_ptr(), ctypes.c_void_p(side.cuda_stream)))
        capi.check(L.bsq_minhash_device(ctypes.byref(d), None, None, 0, ctypes.byref(m), dt, None, None))
        side.synchronize()
        assert (buf[:guard].cpu().numpy() == 0x5A).all()
    buf = torch.full((B * 1024 * 8,), 0x5A, dtype=torch.uint8, device=gpu)
    for dt, m in ((I32, capi.MinHash(33, 64, 0, 0, 0, 0, 0)), (I32, capi.MinHash(21, 2048, 0, 1, 0, 0, 0)), (4, capi.MinHash(21, 64, 0, 0, 0, 0, 0)),
                  (I32, capi.MinHash(21, 64, 0, 0, 0, 0, 1)), (I32, capi.MinHash(21, 0, 0, 0, 0, 0, 0))):
        st = L.bsq_minhash_device(ctypes.byref(d), dch.data_ptr(), dof.data_ptr(), B, ctypes.byref(m), dt, buf.data_ptr(), None)
        torch.cuda.synchronize()
        assert st in (capi.ERR_INVALID_ARG, capi.ERR_DTYPE) and bool((buf == 0x5A).all())


@pytest.mark.parametrize("S, form, kernel", [(5, 1, WAVE), (5, 2, BLOCK % 1024), (4095, 0, BLOCK % 4096), (16383, 0, BLOCK % 16384)])
def test_row_store_paths_on_an_output_one_element_off(gpu, bsq, S, form, kernel):
    """The shared row store (csrc/bsq_row_table.h, write_row) in every form: S no multiple of 16 / sizeof(T), into a (5, S) block that
    starts one element behind a 16-byte boundary inside a guard-filled buffer, so that rows start on and off such a boundary (16-byte
    stores and the tail of S % (16 / sizeof(T)) elements; element stores) -- five rows: a wave workgroup's four and one in a second,
    partly filled one; lengths on the first window, a lane's run of 16 windows, a wave's sweep step and a workgroup's.  Bit-exact
    against the library's CPU twin."""
    import torch
    from bioseq_amd import capi, sketch
    L, tok, k = capi.load(), _tok(bsq, "DNA4"), 21
    d = capi.desc_of(tok)
    rng = np.random.default_rng(50 + S)
    guard = 256
    for lens in ([0, k - 1, k, k + 15, k + 16], [64 * 16 + k, 256 * 16 + k, 0, k + 15, k]):
        chars, offs = _batch(rng, "DNA4", lens)
        dch, dof = _dev(chars, gpu), _dev(offs, gpu)
        for dc, dt in (("i", I32), ("q", U64)):
            assert sketch.minhash_kernel_name(tok, k, 5, S, dc, canonical=True, form=form or None, total_chars=chars.size) == kernel
            exp = sketch.minhash_host(tok, chars, offs, k, S, dc, canonical=True, seed=9)
            skew, n = exp.itemsize, exp.nbytes
            buf = torch.full((n + 2 * guard + skew,), 0x5A, dtype=torch.uint8, device=gpu)
            assert (buf.data_ptr() + guard) % 16 == 0
            m = capi.MinHash(k, S, 1, form, 9, chars.size, 0)
            capi.check(L.bsq_minhash_device(ctypes.byref(d), dch.data_ptr(), dof.data_ptr(), 5, ctypes.byref(m), dt, buf.data_ptr() + guard + skew,
                                            ctypes.c_void_p(capi.raw_stream(gpu))))
            raw = buf.cpu().numpy()
            assert (raw[:guard + skew] == 0x5A).all() and (raw[guard + skew + n:] == 0x5A).all(), "a guard byte of out was overwritten"
            assert raw[guard + skew:guard + skew + n].tobytes() == exp.tobytes(), (S, form, dc, lens)


def test_python_surface_and_refusals(gpu, bsq):
    import torch
    from bioseq_amd import sketch
    tok, amino = _tok(bsq, "DNA4"), _tok(bsq, "AMINO20")
    chars, offs = _batch(np.random.default_rng(1), "DNA4", [60] * 50)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    got = sketch.minhash_packed(tok, dch, dof, 21)  # validate=True: well-formed offsets
    assert got.dtype == torch.int32 and got.shape == (50, 1024)
    bad = dof.clone()
    bad[3] = bad[2] - 1
    with pytest.raises(RuntimeError):
        sketch.minhash_packed(tok, dch, bad, 21)  # malformed offsets
    empty = sketch.minhash_packed(tok, dch[:0], dof[:1], 21, 16, "q")
    assert empty.shape == (0, 16) and empty.dtype == torch.int64
    zeros = torch.zeros(4, dtype=torch.int64, device=gpu)
    assert bool((sketch.minhash_packed(tok, dch[:0], zeros, 21, 16) == sketch.EMPTY).all())  # three empty rows
    for call in (lambda: sketch.minhash_packed(tok, chars, offs, 21),  # host arrays
                 lambda: sketch.minhash_packed(tok, dch, dof, 0), lambda: sketch.minhash_packed(tok, dch, dof, 33),
                 lambda: sketch.minhash_packed(_tok(bsq, "DNA5"), dch, dof, 28), lambda: sketch.minhash_packed(amino, dch, dof, 15),
                 lambda: sketch.minhash_packed(tok, dch, dof, 21, 0), lambda: sketch.minhash_packed(tok, dch, dof, 21, 2 ** 14 + 1),
                 lambda: sketch.minhash_packed(amino, dch, dof, 7, canonical=True),
                 lambda: sketch.minhash_packed(tok, dch, dof, 21, 64, "f"), lambda: sketch.minhash_packed(tok, dch, dof, 21, 64, "h"),
                 lambda: sketch.minhash_packed(tok, dch, dof, 21, 64, "?"), lambda: sketch.minhash_packed(tok, dch, dof, 21, 2048, form=1),
                 lambda: sketch.sketch_compare(got, got[:, :5].contiguous()), lambda: sketch.sketch_compare(got, got.to(torch.int64)),
                 lambda: sketch.sketch_compare(got.to(torch.float32)), lambda: sketch.sketch_compare(got.cpu()), lambda: sketch.sketch_compare(got[0])):
        with pytest.raises(ValueError):
            call()


VALUES = np.array([0xFFFFFFFF, 0, 1, 2, 3, 4, 5, 2 ** 31, 2 ** 32 - 2], dtype=np.uint64)


def _sketch_like(rng, B, S, dtype):
    """values drawn from {EMPTY, 0 .. 5, 2^31, 2^32 - 2} as the element type stores them"""
    v = VALUES[rng.integers(0, VALUES.size, (B, S))]
    if dtype == np.int32:
        return v.astype(np.uint32).view(np.int32)
    v[v == 0xFFFFFFFF] = np.uint64(2 ** 64 - 1)
    return v.view(np.int64)


@pytest.mark.parametrize("Ba, Bb, S", [(1, 1, 1), (3, 5, 7), (65, 130, 100), (64, 64, 1024), (33, 257, 16384)])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_compare_equals_the_twins(gpu, bsq, Ba, Bb, S, dtype):
    import torch
    from bioseq_amd import capi, sketch
    rng = np.random.default_rng(Ba * 1000 + S)
    a, b = _sketch_like(rng, Ba, S, dtype), _sketch_like(rng, Bb, S, dtype)
    exp_m, exp_e = twin.compare(a, b)
    host_m, host_e = sketch.sketch_compare_host(a, b)
    assert np.array_equal(host_m, exp_m) and np.array_equal(host_e, exp_e) and (exp_m.sum() > 0 or S == 1)
    da, db = _dev(a, gpu), _dev(b, gpu)
    got_m, got_e = sketch.sketch_compare(da, db)
    assert got_m.dtype == torch.int32 and got_m.shape == (Ba, Bb) and got_m.is_contiguous()
    assert np.array_equal(got_m.cpu().numpy(), exp_m) and np.array_equal(got_e.cpu().numpy(), exp_e)
    only_m, none = sketch.sketch_compare(da, db, either=False)
    assert none is None and np.array_equal(only_m.cpu().numpy(), exp_m)
    self_m, self_e = sketch.sketch_compare(da)  # a is b
    exp_sm, exp_se = twin.compare(a, a)
    assert np.array_equal(self_m.cpu().numpy(), exp_sm) and np.array_equal(self_e.cpu().numpy(), exp_se)
    # the raw entry point into 0x5A-filled outputs with guards around them
    L, guard, n = capi.load(), 64, Ba * Bb
    bufs = [torch.full((n + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device=gpu) for _ in range(2)]
    capi.check(L.bsq_sketch_compare_device(da.data_ptr(), Ba, db.data_ptr(), Bb, S, I32 if dtype == np.int32 else U64,
                                           bufs[0].data_ptr() + 4 * guard, bufs[1].data_ptr() + 4 * guard, ctypes.c_void_p(capi.raw_stream(gpu))))
    torch.cuda.synchronize()
    for buf, exp in zip(bufs, (exp_m, exp_e)):
        raw = buf.cpu().numpy()
        assert (raw[:guard] == 0x5A5A5A5A).all() and (raw[guard + n:] == 0x5A5A5A5A).all() and np.array_equal(raw[guard:guard + n].reshape(Ba, Bb), exp)
    empty_m, empty_e = sketch.sketch_compare(da[:0], db)
    assert empty_m.shape == (0, Bb) and empty_e.shape == (0, Bb)


def test_jaccard_of_real_sketches(gpu, bsq):
    """sketch_jaccard of a batch with itself: ones on the diagonal for non-empty rows, zeros for empty ones; a copy of a row with a few
    substitutions scores high, unrelated rows near 0; the device result equals the host twin's."""
    import torch
    from bioseq_amd import sketch
    rng = np.random.default_rng(23)
    lens = rng.integers(200, 3000, 70)
    lens[:3] = (0, 20, 2000)
    chars, offs = _batch(rng, "DNA4", lens)
    src = chars[offs[2]:offs[3]].copy()
    edited = src.copy()
    edited[rng.choice(2000, 10, replace=False)] = ord("A")
    chars = np.concatenate([chars, edited])
    offs = np.concatenate([offs, [offs[-1] + 2000]])
    tok = _tok(bsq, "DNA4")
    for dc in ("i", "q"):
        sk = sketch.minhash_packed(tok, _dev(chars, gpu), _dev(offs, gpu), 21, 512, dc, canonical=True)
        jac = sketch.sketch_jaccard(sk)
        assert jac.dtype == torch.float32 and jac.shape == (71, 71)
        diag = torch.diagonal(jac).cpu().numpy()
        assert (diag[:2] == 0).all() and (diag[2:] == 1).all()
        host = sketch.sketch_jaccard(sk.cpu().numpy())
        assert np.array_equal(jac.cpu().numpy(), host)
        assert 0.5 < host[2, 70] < 1.0 and host[2, 3:70].max() < 0.1
        assert torch.equal(jac, sketch.sketch_jaccard(sk, sk.clone()))
