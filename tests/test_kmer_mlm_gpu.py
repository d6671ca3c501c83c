"""GPU: span-masked k-mer masked-LM batches (bioseq_amd.kmers.kmer_mlm_tokenize_packed, bsq_kmer_mlm_tokenize_device) against the numpy
twin (tests/kmer_mlm_twin.py) bit for bit.  A lane owns 16 positions and a workgroup 256 lanes, so the shapes are small: padlens around
the piece, batches of 37 rows (two whole staged workgroups and a partial one at P = 272, rows that start in the middle of a workgroup),
one row longer than a workgroup; spans that reach back across a piece, across a workgroup and before the start of the row."""
import ctypes
import itertools

import numpy as np
import pytest

import kmer_mlm_twin as twin
import kmer_twin
import views_twin

pytestmark = pytest.mark.gpu

DNA_POOL = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTNacgtn*\xff", dtype=np.uint8)  # mostly mapped, some N / lower case / junk
NP_OF = {"b": np.int8, "h": np.int16, "i": np.int32, "q": np.int64, "f": np.float32, "d": np.float64}
S1, SK, GEN = "k_kmer_mlm_bp<s1>", "k_kmer_mlm_bp<sk>", "k_kmer_mlm_generic"


def _lut(key):
    from bioseq_amd import capi
    lut = (ctypes.c_int8 * 256)()
    n = ctypes.c_int32(0)
    assert capi.load().bsq_lut_get(key.encode(), lut, ctypes.byref(n)) == capi.OK
    return np.array(lut, dtype=np.int8), n.value


def _batch(rng, B, k, s, room, pool=DNA_POOL, unmapped=ord("N"), pins=()):
    """Packed batch: rows with no window (lengths 0 and k - 1), one window, exactly `room` windows, more (clamped), random ones; a run of N
    (`unmapped`) in the middle of some rows; the LAST row is full and ends at the last byte of chars (the guarded loads).
    pins: (length, byte) for rows 7, 8, ...: rows of that length filled with that byte."""
    fill = (max(room, 1) - 1) * s + k
    lens = rng.integers(0, fill + 1, B).astype(np.int64)
    lens[:6] = (0, max(k - 1, 0), k, fill, fill + 2 * s + 3, 0)
    lens[-1] = fill
    for r, (n, _) in enumerate(pins):
        lens[7 + r] = n
    chars = rng.choice(pool, int(lens.sum())).astype(np.uint8)
    offs = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    for b in range(6, B, 3):  # N runs of 1 .. 3 characters (inside a span, and where a span would end)
        if lens[b] > 8:
            a = int(offs[b] + rng.integers(0, lens[b] - 3))
            chars[a:a + int(rng.integers(1, 4))] = unmapped
    for r, (_, byte) in enumerate(pins):
        chars[offs[7 + r]:offs[8 + r]] = byte
    chars[offs[-1] - 1] = ord("A")
    return chars, offs


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _tok(bsq, key, flags):
    bos, eos, pad = flags
    return bsq.Tokenizer(key, bool(eos), bool(bos), bool(pad))


# (kernel, k, stride, batch_first): every form of the launch
FORMS = [(S1, 1, 1, True), (S1, 3, 1, True), (S1, 6, 1, True), (S1, 12, 1, True), (SK, 2, 2, True), (SK, 6, 6, True), (SK, 8, 8, True),
         (GEN, 6, 3, True), (GEN, 9, 9, True), (GEN, 6, 1, False)]


@pytest.mark.parametrize("P", [8, 16, 40, 272])
def test_device_equals_the_twin_on_every_form(gpu, bsq, P):
    import torch
    from bioseq_amd import kmers
    B = 37
    last_anchor = unk_in_span = rows_n0 = clamped = 0
    for kernel, k, s, bf in FORMS:
        # (span, flags): before the row start without BOS (j0 = 0) and with it (j0 = -1); span 16 reaches the previous piece
        for span, flags in ((1, (0, 0, 0)), (min(k, 16), (1, 1, 1)), (16, (0, 1, 0)), (16, (1, 0, 1))):
            rng = np.random.default_rng(1000 * P + 10 * k + s + span)
            room = max(P - flags[0] - flags[1], 0)
            chars, offs = _batch(rng, B, k, s, room)
            assert offs[-1] == chars.size
            tok = _tok(bsq, "DNA4", flags)
            dc = "q" if k > 6 else "h"
            assert kmers.kmer_mlm_kernel_name(tok, k, B, P, dc, bf, stride=s) == kernel
            kw = dict(stride=s, span=span, anchor_prob=0.2, mask_prob=0.6, random_prob=0.3, seed=77 + span, first_row=3)
            gi, gl = kmers.kmer_mlm_tokenize_packed(tok, _dev(chars, gpu), _dev(offs, gpu), k, P, dc, bf, validate=False, **kw)
            torch.cuda.synchronize()
            det = []
            kw.pop("stride")
            ti, tl = twin.mlm(*_lut("DNA4"), chars, offs, k, s, P, *flags, details=det, fast=True, **kw)
            gi, gl = gi.cpu().numpy(), gl.cpu().numpy()
            assert gi.dtype == NP_OF[dc] and gl.dtype == np.int64 and gi.shape == ((B, P) if bf else (P, B))
            assert np.array_equal(gi if bf else gi.T, ti.astype(NP_OF[dc])), (kernel, k, s, span, flags)
            assert np.array_equal(gl if bf else gl.T, tl), (kernel, k, s, span, flags)
            V = 4 ** k
            plain = kmer_twin.rows_fast(*_lut("DNA4"), chars, offs, k, s, P, *flags)
            for i, (n, anch, cov, sel) in enumerate(det):
                last_anchor += int(n > 0 and anch[n - 1])
                unk_in_span += int((cov & ~sel).any())
                rows_n0 += int(n == 0)
                clamped += int(n == room and kmer_twin.count(int(offs[i + 1] - offs[i]), k, s) > room)
            assert (tl != -100).any() or room == 0
            assert ((plain == V) & (tl != -100)).sum() == 0
    # the batch reached what it is meant to reach
    assert last_anchor > 0 and unk_in_span > 0 and rows_n0 > 0 and clamped > 0


CODE = {"b": 0, "h": 1, "i": 2, "q": 3, "f": 4, "d": 5}
# (kernel, key, k, stride, batch_first): the rolling-id code and the uniform replacement (rnd32 * V) >> 32 beyond DNA4 -- an alphabet
# that is no power of two, and V = 2^24 through each of its three alphabets
WIDE_FORMS = [(S1, "AMINO20", 5, 1, True), (SK, "AMINO20", 5, 5, True), (GEN, "AMINO20", 5, 2, True), (S1, "SEB8", 8, 1, True),
              (SK, "SEB8", 8, 8, True), (S1, "BYTES", 3, 1, True), (SK, "BYTES", 3, 3, True), (S1, "DNA4", 12, 1, True),
              (GEN, "AMINO20", 5, 1, False), (GEN, "DNA4", 12, 12, True)]


@pytest.mark.parametrize("kernel, key, k, s, bf", WIDE_FORMS)
def test_device_equals_the_twin_beyond_dna4(gpu, bsq, kernel, key, k, s, bf):
    """The loop of test_device_equals_the_twin_on_every_form over the other alphabets, with float and int32 element types: inputs and
    labels cast back to int64 equal the twin's int64 (never the twin through the element type).  f32 inputs run where the rule of
    include/bsq.h accepts them -- at V = 2^24 without flags and with mask_token = 2^24 -- and f64 inputs with every flag.  Every random
    replacement is a plain id, and over an alphabet that is no power of two the batch holds replacements from the upper half of [0, V)."""
    import torch
    from bioseq_amd import kmers
    lut, A = _lut(key)
    V, B = A ** k, 37
    first, last, unmapped, top = kmer_twin.edge_bytes(lut, A, k)
    pool = kmer_twin.edge_pool(lut)
    # (flags, input type, label type): 'f' inputs only where the type holds the ids; mask_token None = the vocabulary size
    plans = [((0, 0, 0), "f", "i"), ((1, 1, 1), "d", "f"), ((1, 0, 1), "i", "d")]
    lab_seen, upper, n_rand, changed = set(), 0, 0, 0
    for P, (flags, dc, ldc), span in itertools.product((40, 272), plans, (1, 16)):
        rng = np.random.default_rng(1000 * P + 10 * k + s + span)
        room = P - flags[0] - flags[1]
        chars, offs = _batch(rng, B, k, s, room, pool, unmapped, pins=((k + 15 * s, last), (k + 15 * s, first)))
        assert offs[-1] == chars.size
        tok = _tok(bsq, key, flags)
        sp = kmer_twin.specials(A, k, *flags)
        mask_token = V if dc == "f" and V == 2 ** 24 else sp["vocab"]
        assert kmer_twin.holds(CODE[dc], 0, max(sp["vocab"] - 1, mask_token)) and kmer_twin.holds(CODE[ldc], -100, V - 1)
        kw = dict(span=span, anchor_prob=0.2, mask_prob=0.5, random_prob=0.3, mask_token=mask_token, seed=77 + span, first_row=3)
        assert kmers.kmer_mlm_kernel_name(tok, k, B, P, dc, bf, stride=s, label_destchar=ldc, mask_token=mask_token) == kernel
        gi, gl = kmers.kmer_mlm_tokenize_packed(tok, _dev(chars, gpu), _dev(offs, gpu), k, P, dc, bf, stride=s, label_destchar=ldc,
                                                validate=False, **kw)
        torch.cuda.synchronize()
        det = []
        ti, tl = twin.mlm(lut, A, chars, offs, k, s, P, *flags, details=det, fast=True, **kw)
        gi, gl = gi.cpu().numpy(), gl.cpu().numpy()
        assert gi.dtype == NP_OF[dc] and gl.dtype == NP_OF[ldc] and gi.shape == ((B, P) if bf else (P, B))
        gi, gl = (x.astype(np.int64) if bf else x.astype(np.int64).T for x in (gi, gl))
        assert np.array_equal(gi, ti), (kernel, P, flags, dc, span)
        assert np.array_equal(gl, tl), (kernel, P, flags, ldc, span)
        # the random branch, recovered from the twin's selection: plain ids only, on the device and in the twin
        for i, (n, anch, cov, sel) in enumerate(det):
            at = flags[0] + np.flatnonzero(twin.fates(kw["seed"], 3 + i, sel, 0.5, 0.3) == 2)
            assert (gi[i, at] >= 0).all() and (gi[i, at] < V).all() and (tl[i, at] != -100).all()
            upper += int((ti[i, at] >= V // 2).sum())
            n_rand += at.size
            changed += int((gi[i, at] != tl[i, at]).sum())
        plain = kmer_twin.rows_fast(lut, A, chars, offs, k, s, P, *flags)
        assert ((plain == V) & (tl != -100)).sum() == 0
        lab_seen |= {0, top} & set(tl.reshape(-1).tolist())
        stored = [0, top, sp["unk"], mask_token] + [sp[n] for n, on in zip(("bos", "eos", "pad"), flags) if on]
        assert set(stored) <= set(ti.reshape(-1).tolist()), (P, flags, span)
    assert lab_seen == {0, top} and n_rand > 200  # both ends of the plain ids were labels; the random branch is well populated
    # a uniform draw meets the window's own id with probability 1 / V <= 20 ** -5: positions that kept their id are not in `at`
    assert changed >= 0.99 * n_rand
    assert upper > 20  # (replacements from the upper half of the plain ids: a product (rnd32 * V) cut to 32 bits would not get there)
    if V == 2 ** 24:  # what the rule refuses for f32 inputs is a ValueError before any launch
        chars, offs = _batch(np.random.default_rng(1), B, k, s, 38, pool, unmapped)
        dch, dof = _dev(chars, gpu), _dev(offs, gpu)
        for flags, mt in (((0, 0, 0), None), ((1, 1, 1), V), ((0, 0, 1), V)):
            with pytest.raises(ValueError):
                kmers.kmer_mlm_tokenize_packed(_tok(bsq, key, flags), dch, dof, k, 40, "f", bf, stride=s, mask_token=mt, validate=False)


@pytest.mark.parametrize("P", [4128, 4124])
def test_a_row_longer_than_a_workgroup(gpu, bsq, P):
    """B = 3 rows of 258 pieces: a row crosses a workgroup boundary and a span reaches back across it; P = 4124 takes the row-piece
    form with unstaged stores."""
    import torch
    from bioseq_amd import kmers
    for (kernel, k, s), span, flags in itertools.product(((S1, 6, 1), (SK, 6, 6)), (6, 16), ((1, 1, 1), (0, 0, 0))):
        rng = np.random.default_rng(P + k + s + span)
        fill = (P - flags[0] - flags[1] - 1) * s + k
        lens = [fill, 0, fill + 5]  # a full row, an empty one, a clamped one that ends at the last byte of chars
        chars = rng.choice(DNA_POOL, sum(lens)).astype(np.uint8)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        tok = _tok(bsq, "DNA4", flags)
        assert kmers.kmer_mlm_kernel_name(tok, k, 3, P, "h", stride=s, label_destchar="h") == kernel
        kw = dict(span=span, anchor_prob=0.05, seed=5)
        gi, gl = kmers.kmer_mlm_tokenize_packed(tok, _dev(chars, gpu), _dev(offs, gpu), k, P, "h", stride=s, label_destchar="h", validate=False, **kw)
        torch.cuda.synchronize()
        ti, tl = twin.mlm(*_lut("DNA4"), chars, offs, k, s, P, *flags, fast=True, **kw)
        assert np.array_equal(gi.cpu().numpy(), ti.astype(np.int16)) and np.array_equal(gl.cpu().numpy(), tl.astype(np.int16)), (kernel, span, flags)
        assert (tl[0, 4000:] != -100).any() and (tl[2, :200] != -100).any()  # (windows either side of the workgroup boundaries)


def test_all_type_pairs_either_output_and_a_side_stream(gpu, bsq):
    import torch
    from bioseq_amd import capi, kmers
    L = capi.load()
    B, P, k, flags = 37, 272, 3, (1, 1, 1)  # 629 pieces: two whole staged workgroups and a partial one
    rng = np.random.default_rng(9)
    chars, offs = _batch(rng, B, k, 1, P - 2)
    lead = 5  # the batch inside a larger buffer: offsets[0] > 0
    big = np.concatenate([np.full(lead, ord("N"), np.uint8), chars])
    offs = offs + lead
    dch, dof = _dev(big, gpu), _dev(offs, gpu)
    d = capi.make_desc("DNA4", eos=True, bos=True, padchar=True)
    side = torch.cuda.Stream(device=gpu)
    tdt = {capi.I8: torch.int8, capi.I16: torch.int16, capi.I32: torch.int32, capi.U64: torch.int64, capi.F32: torch.float32, capi.F64: torch.float64}
    n, guard = B * P, 256
    for (kernel, s), bf in itertools.product(((S1, 1), (SK, 3), (GEN, 2)), (True,)):
        km = capi.Kmer(k, s)
        m = capi.KmerMlm(0.25, 0.8, 0.1, 3, 68, -100, 11, 2)
        ti, tl = twin.mlm(*_lut("DNA4"), big, offs, k, s, P, *flags, anchor_prob=0.25, span=3, mask_token=68, seed=11, first_row=2, fast=True)
        assert (tl != -100).any()
        for it, lt in itertools.product(range(6), repeat=2):
            assert L.bsq_kmer_mlm_kernel_name(ctypes.byref(d), ctypes.byref(km), ctypes.byref(m), B, P, 1, it, lt) == kernel.encode()
            bi = torch.full((n + 2 * guard,), -77, dtype=tdt[it], device=gpu)
            bl = torch.full((n + 2 * guard,), -77, dtype=tdt[lt], device=gpu)
            side.wait_stream(torch.cuda.current_stream())
            capi.check(L.bsq_kmer_mlm_tokenize_device(ctypes.byref(d), dch.data_ptr(), dof.data_ptr(), B, P, 1, ctypes.byref(km), ctypes.byref(m),
                                                      it, bi.data_ptr() + guard * bi.element_size(), lt, bl.data_ptr() + guard * bl.element_size(),
                                                      ctypes.c_void_p(side.cuda_stream)))
            side.synchronize()
            for buf, want in ((bi, ti), (bl, tl)):
                raw = buf.cpu().numpy()
                assert (raw[:guard] == -77).all() and (raw[guard + n:] == -77).all(), "a guard element was overwritten"
                assert np.array_equal(raw[guard:guard + n].reshape(B, P), want.astype(raw.dtype)), (kernel, it, lt)
        # either output alone: the other buffer is not touched, the one given holds the same values
        for want_in in (True, False):
            bi = torch.full((n,), -77, dtype=torch.int16, device=gpu)
            bl = torch.full((n,), -77, dtype=torch.int64, device=gpu)
            capi.check(L.bsq_kmer_mlm_tokenize_device(ctypes.byref(d), dch.data_ptr(), dof.data_ptr(), B, P, 1, ctypes.byref(km), ctypes.byref(m),
                                                      capi.I16, bi.data_ptr() if want_in else None, capi.U64, None if want_in else bl.data_ptr(), None))
            torch.cuda.synchronize()
            if want_in:
                assert np.array_equal(bi.cpu().numpy().reshape(B, P), ti.astype(np.int16)) and (bl == -77).all()
            else:
                assert np.array_equal(bl.cpu().numpy().reshape(B, P), tl) and (bi == -77).all()
    # refusals on the device, nothing written: both outputs NULL, the element types
    bi = torch.full((n,), -77, dtype=torch.int64, device=gpu)
    km, m = capi.Kmer(4, 1), capi.KmerMlm(0.25, 0.8, 0.1, 4, 260, -100, 11, 0)  # vocab 260, V - 1 = 255
    call = lambda it, i, lt, l_: L.bsq_kmer_mlm_tokenize_device(ctypes.byref(d), dch.data_ptr(), dof.data_ptr(), B, P, 1, ctypes.byref(km),
                                                               ctypes.byref(m), it, i, lt, l_, None)
    assert call(capi.U64, None, capi.U64, None) == capi.ERR_INVALID_ARG
    assert call(capi.I8, bi.data_ptr(), capi.U64, None) == capi.ERR_DTYPE      # the inputs: vocab - 1 and mask_token > 127
    assert call(capi.I16, bi.data_ptr(), capi.I8, bi.data_ptr()) == capi.ERR_DTYPE  # the labels: V - 1 > 127
    assert call(capi.I16, bi.data_ptr(), capi.I16, None) == capi.OK
    m.mask_token = 32768
    assert call(capi.I16, bi.data_ptr(), capi.U64, None) == capi.ERR_DTYPE
    # mask_token and ignore_index against the rule of the element types: each refusal, then its neighbour at the boundary.  The int8
    # labels run with k = 3 (V - 1 = 63, vocab 68), where the type holds every plain id and ignore_index alone decides
    bl = torch.full((n,), -77, dtype=torch.int64, device=gpu)
    for kk, it, lt, mt, ign, want in ((4, capi.I32, capi.U64, 2 ** 31, -100, capi.ERR_DTYPE), (4, capi.I32, capi.U64, 2 ** 31 - 1, -100, capi.OK),
                                      (4, capi.F32, capi.U64, 2 ** 24 + 1, -100, capi.ERR_DTYPE), (4, capi.F32, capi.U64, 2 ** 24, -100, capi.OK),
                                      (4, capi.F64, capi.U64, 2 ** 53 + 1, -100, capi.ERR_DTYPE),
                                      (3, capi.U64, capi.I8, 68, -129, capi.ERR_DTYPE), (3, capi.U64, capi.I8, 68, -128, capi.OK),
                                      (3, capi.U64, capi.I8, 68, -1000, capi.ERR_DTYPE),  # (would read as the plain id 24)
                                      (4, capi.U64, capi.I16, 260, -32769, capi.ERR_DTYPE), (4, capi.U64, capi.I16, 260, -32768, capi.OK),
                                      (4, capi.U64, capi.F32, 260, -2 ** 24 - 1, capi.ERR_DTYPE), (4, capi.U64, capi.F32, 260, -2 ** 24, capi.OK)):
        km.k, m.mask_token, m.ignore_index = kk, mt, ign
        assert kmer_twin.holds(lt, 0, 4 ** kk - 1) and kmer_twin.holds(it, 0, 4 ** kk + 3)  # (so mask_token or ignore_index decides)
        bi.fill_(-77), bl.fill_(-77)
        assert call(it, bi.data_ptr(), lt, bl.data_ptr()) == want, (kk, it, lt, mt, ign)
        torch.cuda.synchronize()
        if want != capi.OK:
            assert bool((bi == -77).all()) and bool((bl == -77).all()), (kk, it, lt, mt, ign)
        else:  # (the buffers are int64 elements wide: a narrower type fills their first bytes)
            ti, tl = twin.mlm(*_lut("DNA4"), big, offs, kk, 1, P, *flags, anchor_prob=0.25, span=4, mask_token=mt, ignore_index=ign, seed=11, fast=True)
            assert (tl != ign).any() and (tl == ign).any()
            for buf, t, exp in ((bi, it, ti), (bl, lt, tl)):
                got = buf.cpu().numpy().view(kmer_twin.NP_DTYPES[t])[:n]
                assert np.array_equal(kmer_twin.back(got).reshape(B, P), exp), (kk, it, lt, mt, ign)
    km.k = 4
    m.mask_token, m.ignore_index = 260, -100
    torch.cuda.synchronize()
    tok = _tok(bsq, "DNA4", flags)
    with pytest.raises(ValueError):
        kmers.kmer_mlm_tokenize_packed(tok, dch, dof, 4, P, "b")
    with pytest.raises(ValueError):
        kmers.kmer_mlm_tokenize_packed(tok, dch, dof, 4, P, "h", label_destchar="b")
    with pytest.raises(ValueError):
        kmers.kmer_mlm_tokenize_packed(tok, big, offs, 3, P)  # host arrays
    with pytest.raises(RuntimeError):
        kmers.kmer_mlm_tokenize_packed(tok, dch, dof, 3, P)  # validate=True: a row is over-long
    empty = kmers.kmer_mlm_tokenize_packed(tok, dch[:0], dof[:1], 3, 8)
    assert empty[0].shape == (0, 8) and empty[1].shape == (0, 8)


def test_no_anchor_is_the_plain_encode_and_the_draw_ignores_shards_and_padlen(gpu, bsq):
    import torch
    from bioseq_amd import kmers
    rng = np.random.default_rng(31)
    B = 37
    for (k, s), flags in itertools.product(((6, 1), (6, 6), (6, 3)), ((1, 1, 1), (0, 0, 0))):
        P1, P2 = 40, 272
        chars, offs = _batch(rng, B, k, s, P2 - flags[0] - flags[1])
        dch, dof = _dev(chars, gpu), _dev(offs, gpu)
        tok = _tok(bsq, "DNA4", flags)
        for bf in (True, False):
            plain = kmers.kmer_tokenize_packed(tok, dch, dof, k, P2, "h", bf, stride=s, validate=False)
            gi, gl = kmers.kmer_mlm_tokenize_packed(tok, dch, dof, k, P2, "h", bf, stride=s, anchor_prob=0.0, validate=False)
            assert torch.equal(gi, plain) and bool((gl == -100).all())
        kw = dict(stride=s, frac=0.3, seed=4, validate=False)
        wi, wl = kmers.kmer_mlm_tokenize_packed(tok, dch, dof, k, P2, "i", **kw)
        assert bool((wl != -100).any())
        # a shard with first_row = r equals rows r .. of the whole (the shard's offsets start inside the buffer)
        for b0, b1 in ((0, 5), (5, 37), (20, 21)):
            pi, pl = kmers.kmer_mlm_tokenize_packed(tok, dch, dof[b0:b1 + 1].contiguous(), k, P2, "i", first_row=b0, **kw)
            assert torch.equal(pi, wi[b0:b1]) and torch.equal(pl, wl[b0:b1]), (k, s, b0)
        # the windows a row holds at the short padlen carry the values they have at the long one
        si, sl = kmers.kmer_mlm_tokenize_packed(tok, dch, dof, k, P1, "i", **kw)
        torch.cuda.synchronize()
        si, sl, wi_, wl_ = (x.cpu().numpy() for x in (si, sl, wi, wl))
        for b in range(B):
            n1 = min(kmer_twin.count(int(offs[b + 1] - offs[b]), k, s), P1 - flags[0] - flags[1])
            w = slice(flags[0], flags[0] + n1)
            assert np.array_equal(si[b, w], wi_[b, w]) and np.array_equal(sl[b, w], wl_[b, w]), (k, s, b)


def test_kmer_mlm_dataset(gpu, bsq, tmp_path):
    import torch
    from bioseq_amd import kmers
    from bioseq_amd.flatfile import FlatFile, write_flatfile
    from bioseq_amd.loaders import FlatFileDataset
    rng = np.random.default_rng(2)
    lens = rng.integers(0, 300, 300)
    lens[:3] = (0, 5, 700)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGTACGTACGTACGTNacgtRY", np.uint8), int(n))) for n in lens]
    ff = FlatFile(write_flatfile(seqs, str(tmp_path / "kmlm.ff")))
    tok = _tok(bsq, "DNA4", (1, 1, 1))
    lut, A = _lut("DNA4")
    mask_key = (13 * 0x9E3779B97F4A7C15 + 1) & (2 ** 64 - 1)  # the dataset's first mask key (seed 13)
    for crop, rc, stride, span in ((None, 0.0, 1, None), (128, 0.5, 1, 3), (128, 1.0, 6, None)):
        def epoch(**opts):
            ds = FlatFileDataset(ff, tok, device=gpu, kmer=6, kmer_stride=stride, kmer_mlm=True, kmer_span=span, crop=crop, revcomp_frac=rc,
                                 token_dtype="i", maskfrac=0.2)
            g = torch.Generator(device=gpu).manual_seed(5)
            out = [(a.clone(), b.clone()) for a, b in ds.batches(64, generator=g, **opts)]
            torch.cuda.synchronize()
            return ds, out

        ds, base = epoch()
        longest = crop if crop else 700
        width = (longest - 6) // stride + 1 + 2
        assert ds.max_seq_len == width and len(base) == 5
        assert all(a.dtype == torch.int32 and b.dtype == torch.int64 and a.shape == b.shape and a.shape[1] == width for a, b in base)
        g = torch.Generator(device=gpu).manual_seed(5)
        order = torch.randperm(len(ff), device=gpu, generator=g).cpu().numpy()
        if crop or rc:
            key = (13 * 0xC2B2AE3D27D4EB4F + 1) & (2 ** 64 - 1)  # the dataset's first view key
            starts, lengths, strand = views_twin.plan(ff._offsets, crop or 0, order, mode="random", revcomp_frac=rc, seed=key, first_row=0)
            e_chars, e_offs = views_twin.apply(np.asarray(ff._chars), ff._offsets, order, starts, lengths, strand)
        else:
            e_chars = np.frombuffer(b"".join(seqs[i] for i in order), np.uint8)
            e_offs = np.concatenate([[0], np.cumsum([len(seqs[i]) for i in order])]).astype(np.int64)
        # the direct call with the loader's key, rows keyed by their index in the epoch's order
        di, dl = kmers.kmer_mlm_tokenize_packed(tok, _dev(e_chars, gpu), _dev(e_offs, gpu), 6, width, "i", stride=stride, frac=0.2, span=span,
                                                seed=mask_key, validate=False)
        gi, gl = torch.cat([a for a, _ in base]), torch.cat([b for _, b in base])
        assert torch.equal(gi, di) and torch.equal(gl, dl), (crop, rc, stride)
        eff_span = span if span is not None else -(-6 // stride)
        ti, tl = twin.mlm(lut, A, e_chars, e_offs, 6, stride, width, 1, 1, 1, anchor_prob=twin.span_anchor_prob(0.2, eff_span), span=eff_span,
                          seed=mask_key, fast=True)
        assert np.array_equal(gi.cpu().numpy(), ti.astype(np.int32)) and np.array_equal(gl.cpu().numpy(), tl)
        # labels are set only where the plain batch holds a plain window, and hold its id
        plain = kmer_twin.rows_fast(lut, A, e_chars, e_offs, 6, stride, width, 1, 1, 1)
        lab = gl.cpu().numpy()
        on = lab != -100
        assert on.any() and (plain[on] < 4 ** 6).all() and np.array_equal(lab[on], plain[on])
        assert np.array_equal(gi.cpu().numpy()[~on], plain[~on])
        for opts in ({"group": 4}, {"prefetch": 2}, {"group": 4, "prefetch": 2}):
            _, got = epoch(**opts)
            assert len(got) == len(base) and all(torch.equal(a, c) and torch.equal(b, e) for (a, b), (c, e) in zip(base, got)), opts
        # the other access paths hand out pairs; every call draws with the next key
        a, b = ds[1]
        assert a.shape == b.shape == (width,)
        x1, y1 = ds.get_batch(0, 50)
        x2, y2 = ds.get_batch(0, 50)
        assert x1.shape == y1.shape == (50, width) and y1.dtype == torch.int64 and not torch.equal(y1, y2)
        x3, y3 = ds.__getitems__([5, 3, 9])
        assert x3.shape == y3.shape == (3, width)
    for kw in ({"masked": True}, {"cnn": True}, {"pack": "stream"}):
        with pytest.raises(ValueError):
            FlatFileDataset(ff, tok, device=gpu, kmer=6, kmer_mlm=True, **kw)
    with pytest.raises(ValueError):
        FlatFileDataset(ff, tok, device=gpu, kmer_mlm=True)
