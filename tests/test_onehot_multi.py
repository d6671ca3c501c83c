"""bsq_onehot_device_multi / bioseq_amd.multi.onehot_packed_multi on the device: n packed batches of one tokenizer, padlen, layout and
element type -- the chunk-owner batches in ONE k_onehot_chunks_multi launch, the one-piece two-pass batches in ONE raw-id launch and ONE
expansion launch, the plain (B,C,P) chunk-stream batches in ONE k_tokenize_chunks_multi launch, everything else as its single call -- byte for byte against the single calls (bsq_onehot_device / bsq_onehot_bcl_device)
and the oracle, with sentinel bytes around every output."""
import ctypes
import itertools

import numpy as np
import pytest

from bioseq_amd import synth

pytestmark = pytest.mark.gpu

DTYPES = {"b": ("I8", "int8"), "h": ("I16", "int16"), "i": ("I32", "int32"), "l": ("U64", "int64"), "f": ("F32", "float32"),
          "d": ("F64", "float64")}
SENT = 0x5A


def _batch(seed, n, lo, hi, alphabet=synth.AA):
    lens = synth.synth_lengths(seed, n, lo, hi)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    rng = np.random.default_rng(seed)
    letters = np.frombuffer((alphabet + alphabet.lower()).encode(), dtype=np.uint8)
    chars = letters[rng.integers(0, letters.size, size=int(offs[-1]))].copy()
    k = rng.random(chars.size) < 0.03
    chars[k] = rng.integers(0, 256, size=int(k.sum()), dtype=np.uint8)
    return chars, offs


class _Run:
    """the batches on the device; outputs as views into one sentinel-filled byte buffer (`pad` bytes before and after each)"""

    def __init__(self, gpu, batches, masks=None, pad=4096, shift=0):
        import torch
        self.torch, self.gpu = torch, gpu
        self.dev = []
        for i, (c, o) in enumerate(batches):
            dc = torch.from_numpy(np.concatenate([c, np.zeros(16, np.uint8)])).to(gpu)
            do = torch.from_numpy(o).to(gpu)
            m = None
            if masks is not None and masks[i] is not None:
                m = torch.from_numpy(np.concatenate([masks[i], np.ones(16, np.uint8)])).to(gpu)
            self.dev.append((dc, do, m, len(o) - 1))
        self.pad, self.shift = pad, shift

    def launch(self, lib, capi, desc, P, layout, code, multi=True, stream=None, table_hook=None, host=True):
        """host=False: no device-wide synchronisation; the (device) buffer comes back, ordered only by the caller's stream"""
        torch = self.torch
        C = lib.bsq_alphabet_size(ctypes.byref(desc))
        sz = int(lib.bsq_dtype_size(getattr(capi, code)))
        sizes = [B * C * P * sz for (_, _, _, B) in self.dev]
        at, offs = 0, []
        for n in sizes:
            at += self.pad + self.shift
            offs.append(at)
            at += (n + 4095) // 4096 * 4096
        buf = torch.full((at + self.pad,), SENT, dtype=torch.uint8, device=self.gpu)
        arr = (capi.OnehotBatch * max(len(self.dev), 1))()
        for i, (dc, do, m, B) in enumerate(self.dev):
            arr[i].chars, arr[i].offsets, arr[i].B = dc.data_ptr(), do.data_ptr(), B
            arr[i].mask = m.data_ptr() if m is not None else None
            arr[i].out = buf.data_ptr() + offs[i]
        if table_hook:
            table_hook(arr)
        s = ctypes.c_void_p(stream) if stream else None
        st = capi.OK
        if multi:
            st = lib.bsq_onehot_device_multi(ctypes.byref(desc), len(self.dev), arr, P, layout, getattr(capi, code), s)
        else:
            fn = lib.bsq_onehot_device if layout == 0 else lib.bsq_onehot_bcl_device
            for i in range(len(self.dev)):
                a = arr[i]
                st = fn(ctypes.byref(desc), a.chars, a.offsets, a.mask, a.B, P, getattr(capi, code), a.out, s)
                if st != capi.OK:
                    break
        if not host:
            return st, buf, offs, sizes
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        return st, h, offs, sizes


def _check_sentinels(h, offs, sizes):
    prev = 0
    for o, n in zip(offs, sizes):
        assert (h[prev:o] == SENT).all(), "bytes before an output changed"
        prev = o + n
    assert (h[prev:] == SENT).all(), "bytes after the last output changed"


def _same(lib, capi, gpu, batches, key, flags, P, layout, dc, masks=None, shift=0, oracle=None):
    desc = capi.make_desc(key, *flags)
    code, npn = DTYPES[dc]
    run = _Run(gpu, batches, masks, shift=shift)
    st, got, offs, sizes = run.launch(lib, capi, desc, P, layout, code, multi=True)
    capi.check(st)
    _check_sentinels(got, offs, sizes)
    st, want, _, _ = run.launch(lib, capi, desc, P, layout, code, multi=False)
    capi.check(st)
    for i, (o, n) in enumerate(zip(offs, sizes)):
        assert np.array_equal(got[o:o + n], want[o:o + n]), (key, flags, P, layout, dc, i)
    if oracle is not None:
        ora = oracle.OracleTokenizer(key, *flags)
        C = lib.bsq_alphabet_size(ctypes.byref(desc))
        for i, ((c, of), o, n) in enumerate(zip(batches, offs, sizes)):
            B = len(of) - 1
            if B == 0:
                continue
            m = masks[i] if masks is not None else None
            w = ora.onehot_packed(c, of, P, dc, mask=m) if m is not None else ora.onehot_packed(c, of, P, dc)
            w = np.ascontiguousarray(w if layout == 0 else np.transpose(w, (1, 2, 0)))
            g = got[o:o + n].view(np.dtype(npn)).reshape(w.shape)
            assert np.array_equal(g, w), ("oracle", key, flags, dc, i)
    return desc


def _plan(lib, capi, desc, batches, P, layout, code, shift=0):  # (fabricated 4-KiB aligned addresses + shift: the plan reads pointer values only)
    arr = (capi.OnehotBatch * max(len(batches), 1))()
    fam = (ctypes.c_int32 * max(len(batches), 1))()
    for i, (_, o) in enumerate(batches):
        arr[i].chars = arr[i].offsets = 1 << 40
        arr[i].B = len(o) - 1
        arr[i].out = (1 << 40) + (i << 34) + shift
    r = lib.bsq_onehot_multi_plan(ctypes.byref(desc), len(batches), arr, P, layout, getattr(capi, code), fam)
    return r, list(fam)[:len(batches)]


def test_chunk_owner_family_all_flags_dtypes(gpu, oracle):
    """family 1 (k_onehot_chunks_multi) for 1 ... 8 batches of different B, every flag combination on DNA4 / DNA5 / AMINO20, every dtype"""
    from bioseq_amd import capi
    lib = capi.load()
    P = 256
    sizes = [300, 1024, 77, 2048, 1, 640, 999, 128]
    for key, alpha in (("DNA4", "ACGT"), ("DNA5", "ACGTN"), ("AMINO20", synth.AA)):
        batches = [_batch(10 + i, b, 0, P - 2, alpha) for i, b in enumerate(sizes)]
        for flags in itertools.product([False, True], repeat=3):
            desc = capi.make_desc(key, *flags)
            _, fam = _plan(lib, capi, desc, batches, P, 0, "F32")
            assert fam == [1] * 8, (key, flags, fam)
            for n in (1, 2, 5, 8):
                _same(lib, capi, gpu, batches[:n], key, flags, P, 0, "f", oracle=oracle if n == 5 else None)
        for dc in "bhild":
            _same(lib, capi, gpu, batches[:4], key, (True, True, True), P, 0, dc, oracle=oracle)


def test_two_pass_family_bytes_and_nibbles(gpu, oracle):
    """family 2: one raw-id launch + one expansion launch -- k_expand_chunks<nibbles> (DNA4 f32), k_expand_rows1<nibbles> (int8), byte ids
    with the gate (AMINO20 bf16-sized rows: int16) -- against the single calls and the oracle"""
    from bioseq_amd import capi
    lib = capi.load()
    for key, alpha, flags, P, dc, sizes in (("DNA4", "ACGT", (True, True, True), 160, "f", [131072, 65536 + 333, 100000]),
                                             ("DNA4", "ACGT", (True, True, True), 160, "b", [262144, 262144 - 5]),
                                             ("DNA5", "ACGTN", (False, True, False), 100, "b", [600000, 300001]),
                                             ("AMINO20", synth.AA, (True, False, True), 512, "h", [16384, 16384 + 64])):
        batches = [_batch(50 + i, b, 0, P - 2, alpha) for i, b in enumerate(sizes)]
        desc = capi.make_desc(key, *flags)
        _, fam = _plan(lib, capi, desc, batches, P, 0, DTYPES[dc][0])
        assert fam == [2] * len(sizes), (key, dc, fam)
        _same(lib, capi, gpu, batches, key, flags, P, 0, dc, oracle=oracle if dc == "b" else None)


def test_channels_first_family_all_flags_dtypes(gpu, oracle):
    """family 3 (k_tokenize_chunks_multi): (B,C,P) batches of 1 ... 8 of different B, every flag combination on DNA4 / DNA5 / AMINO20, every
    dtype, masks on some; element-aligned outputs and a padlen that is no multiple of 16 / sizeof(T) take the ragged single calls"""
    from bioseq_amd import capi
    lib = capi.load()
    P = 256
    sizes = [300, 1024, 77, 2048, 1, 640, 999, 128]
    rng = np.random.default_rng(11)
    for key, alpha in (("DNA4", "ACGT"), ("DNA5", "ACGTN"), ("AMINO20", synth.AA)):
        batches = [_batch(210 + i, b, 0, P - 2, alpha) for i, b in enumerate(sizes)]
        for flags in itertools.product([False, True], repeat=3):
            desc = capi.make_desc(key, *flags)
            assert _plan(lib, capi, desc, batches, P, 1, "F32")[1] == [3] * 8, (key, flags)
            for n in (1, 2, 5, 8):
                _same(lib, capi, gpu, batches[:n], key, flags, P, 1, "f", oracle=oracle if n == 5 else None)
        masks = [(rng.random(c.size) > 0.25).astype(np.uint8) if i % 3 == 0 else None for i, (c, _) in enumerate(batches)]
        for dc in "bhild":
            _same(lib, capi, gpu, batches[:4], key, (True, True, True), P, 1, dc, masks=masks[:4], oracle=oracle)
            code = DTYPES[dc][0]
            sz = int(lib.bsq_dtype_size(getattr(capi, code)))
            desc = capi.make_desc(key, True, True, True)
            if sz < 16:  # element-aligned, not 16-byte aligned: the ragged form, single calls
                assert _plan(lib, capi, desc, batches[:4], P, 1, code, shift=sz)[1] == [0] * 4
                _same(lib, capi, gpu, batches[:4], key, (True, True, True), P, 1, dc, shift=sz)
        odd = [_batch(230 + i, b, 0, 199, alpha) for i, b in enumerate([500, 64, 1000])]
        assert _plan(lib, capi, capi.make_desc(key), odd, 201, 1, "I32")[1] == [0] * 3
        _same(lib, capi, gpu, odd, key, (False, False, False), 201, 1, "i")


def test_two_pass_8_byte_elements_and_mixed_keys(gpu):
    """family 2 with 8-byte elements (k_expand_chunks_multi<uint64_t>: int64, f64), and a group whose two-pass batches have different keys
    (byte ids beside one batch with more than 128 MB of ids, which takes nibbles and runs as its single call) -- against the single calls,
    compared on the device"""
    import torch
    from bioseq_amd import capi
    lib = capi.load()
    for dc in "ld":
        batches = [_batch(240 + i, b, 0, 158, "ACGT") for i, b in enumerate([100000, 100077])]
        desc = capi.make_desc("DNA4", True, True, True)
        assert _plan(lib, capi, desc, batches, 160, 0, DTYPES[dc][0])[1] == [2, 2]
        _same(lib, capi, gpu, batches, "DNA4", (True, True, True), 160, 0, dc)
    batches = [_batch(250 + i, b, 0, 62, "ACGTN") for i, b in enumerate([200000, 2100000, 200005])]
    desc = capi.make_desc("DNA5")
    assert _plan(lib, capi, desc, batches, 64, 0, "F32")[1] == [2, 0, 2]
    run = _Run(gpu, batches)
    st, got, offs, sizes = run.launch(lib, capi, desc, 64, 0, "F32", multi=True, host=False)
    capi.check(st)
    torch.cuda.synchronize()
    prev = 0
    for o, n in zip(offs, sizes):
        assert bool((got[prev:o] == SENT).all())
        prev = o + n
    assert bool((got[prev:] == SENT).all())
    st, want, _, _ = run.launch(lib, capi, desc, 64, 0, "F32", multi=False, host=False)
    capi.check(st)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_full_size_cases(gpu):
    """4 x the cfg4f shard (131072 x 160 DNA4 + BOS/EOS/PAD f32, family 2), 4 x (8192 x 1024 AMINO20 f32, family 1) and 4 x the cnn loader's
    (B,C,P) batch (4096 x 512 SEB8 f32, family 3) against the single calls"""
    from bioseq_amd import capi
    lib = capi.load()
    for key, alpha, flags, P, B, want in (("DNA4", "ACGT", (True, True, True), 160, 131072, 2), ("AMINO20", synth.AA, (False, False, False), 1024, 8192, 1)):
        batches = [_batch(70 + i, B, P // 2, P - 2, alpha) for i in range(4)]
        desc = capi.make_desc(key, *flags)
        assert _plan(lib, capi, desc, batches, P, 0, "F32")[1] == [want] * 4
        _same(lib, capi, gpu, batches, key, flags, P, 0, "f")
    seb = [_batch(80 + i, 4096, 256, 510, synth.AA) for i in range(4)]
    assert _plan(lib, capi, capi.make_desc("SEB8"), seb, 512, 1, "F32")[1] == [3] * 4
    _same(lib, capi, gpu, seb, "SEB8", (False, False, False), 512, 1, "f")


def test_mixed_groups_empty_batches_shared_chars_and_bcl(gpu, oracle):
    """mixed families in a group, B == 0 batches, 19 batches, a batch of only empty sequences, one chars buffer under two offset slices,
    and the (B,C,P) layout -- equal to the single calls"""
    from bioseq_amd import capi
    lib = capi.load()
    key, alpha, flags = "DNA4", "ACGT", (True, True, True)
    P = 160
    sizes = [4096, 0, 262144, 65536, 0, 4096, 262144, 1000, 3, 0, 4096, 8192, 16, 2048, 0, 512, 64, 4096, 100]
    batches = [_batch(90 + i, b, 0, P - 2, alpha) for i, b in enumerate(sizes)]
    empty = (np.zeros(0, np.uint8), np.zeros(51, np.int64))
    c, o = _batch(7, 3000, 0, P - 2, alpha)
    shared = [(c, o[:1501].copy()), (c, o[1500:].copy()), empty]
    for dc in "bf":
        _same(lib, capi, gpu, batches, key, flags, P, 0, dc)
        _same(lib, capi, gpu, shared + batches[:3], key, flags, P, 0, dc, oracle=oracle)
        _same(lib, capi, gpu, shared + batches[:6], key, flags, P, 1, dc)
    # the cnn loader's batch shape, (B,C,P)
    seb = [_batch(95 + i, 4096, 0, 512, synth.AA) for i in range(4)]
    _same(lib, capi, gpu, seb, "SEB8", (False, False, False), 512, 1, "f", oracle=oracle)


def test_masks_and_misaligned_outputs(gpu, oracle):
    """per-batch masks (some None: masked two-pass batches run alone, masked chunk-owner batches stay fused), and outputs placed off their
    natural alignment (element-aligned only: the (B,C,P) fallback; chunk heads of the (P,B,C) streams)"""
    from bioseq_amd import capi
    lib = capi.load()
    key, alpha, flags, P = "AMINO20", synth.AA, (True, True, False), 256
    batches = [_batch(120 + i, b, 0, P - 2, alpha) for i, b in enumerate([2048, 700, 4096, 33])]
    rng = np.random.default_rng(3)
    masks = [(rng.random(c.size) > 0.2).astype(np.uint8) if i % 2 == 0 else None for i, (c, _) in enumerate(batches)]
    for dc in "fbd":
        _same(lib, capi, gpu, batches, key, flags, P, 0, dc, masks=masks, oracle=oracle if dc == "f" else None)
        _same(lib, capi, gpu, batches, key, flags, P, 1, dc, masks=masks)
        _same(lib, capi, gpu, batches, key, flags, P, 0, dc, shift=8)
        _same(lib, capi, gpu, batches, key, flags, P, 1, dc, shift=8)
    big = [_batch(130 + i, 131072, 0, 160, "ACGT") for i in range(3)]
    bm = [(np.random.default_rng(i).random(c.size) > 0.5).astype(np.uint8) if i == 1 else None for i, (c, _) in enumerate(big)]
    _same(lib, capi, gpu, big, "DNA4", (True, True, True), 160, 0, "f", masks=bm)


def test_side_stream_and_invalid_last_batch(gpu):
    """a side stream (the caller's event after the call is all the ordering needed); an invalid batch LAST in the table: BSQ_ERR_INVALID_ARG
    and every earlier output still holds its sentinel"""
    import torch
    from bioseq_amd import capi
    lib = capi.load()
    key, flags, P = "DNA4", (True, True, True), 160
    batches = [_batch(140 + i, b, 0, P - 2, "ACGT") for i, b in enumerate([4096, 131072, 4096, 131072])]
    desc = capi.make_desc(key, *flags)
    run = _Run(gpu, batches)
    st, want, offs, sizes = run.launch(lib, capi, desc, P, 0, "F32", multi=False)
    capi.check(st)
    # the call on a side stream; the reader's stream waits for an event recorded on the side stream after the call -- no device-wide
    # synchronisation anywhere between the call and the read
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    reader = torch.cuda.current_stream(gpu)
    side.wait_stream(reader)  # (the sentinel fill of the output buffer is queued on the reader's stream)
    with torch.cuda.stream(side):
        st, dbuf, _, _ = run.launch(lib, capi, desc, P, 0, "F32", multi=True, stream=side.cuda_stream, host=False)
        done = torch.cuda.Event()
        done.record(side)
    capi.check(st)
    reader.wait_event(done)
    got = dbuf.to("cpu", non_blocking=False).numpy()  # a copy ordered on the reader's stream only
    for o, n in zip(offs, sizes):
        assert np.array_equal(got[o:o + n], want[o:o + n])

    def spoil(arr):
        arr[len(batches) - 1].offsets = None

    st, h, offs, sizes = run.launch(lib, capi, desc, P, 0, "F32", multi=True, table_hook=spoil)
    assert st == capi.ERR_INVALID_ARG
    assert (h == SENT).all()


def test_python_surface(gpu, bsq):
    """onehot_packed_multi against tok.onehot_packed: both layouts, outs=, masks=, validate= errors, int32 offsets"""
    import torch
    from bioseq_amd import multi
    tok = _tokenizer(bsq)
    P = 160
    batches = [_batch(150 + i, b, 0, P - 2, "ACGT") for i, b in enumerate([4096, 131072, 8192, 131072, 77])]
    dev = [(torch.from_numpy(c).to(gpu), torch.from_numpy(o).to(gpu)) for c, o in batches]
    rng = np.random.default_rng(5)
    masks = [torch.from_numpy((rng.random(c.size) > 0.3).astype(np.uint8)).to(gpu) if i in (0, 4) else None for i, (c, _) in enumerate(batches)]
    for layout in ("tbc", "bcl"):
        got = multi.onehot_packed_multi(tok, dev, P, "f", layout=layout, masks=masks)
        for (c, o), m, g in zip(dev, masks, got):
            w = tok.onehot_packed(c, o, P, "f", mask=m, layout=layout)
            assert g.shape == w.shape and torch.equal(g, w)
    C = got[0].shape[1]  # (the "bcl" results: (B, C, P))
    outs = [torch.empty((P, int(o.numel()) - 1, C), dtype=torch.float32, device=gpu) for _, o in dev]
    got = multi.onehot_packed_multi(tok, dev, P, "f", outs=outs)
    assert all(g is o for g, o in zip(got, outs))
    with pytest.raises(ValueError):
        multi.onehot_packed_multi(tok, dev, P, "f", outs=[torch.empty((P, 3, C), device=gpu)] * len(dev))
    with pytest.raises(ValueError):
        multi.onehot_packed_multi(tok, dev, P, "f", masks=[None])
    # int32 offsets with an over-long sequence: the reference's error (the offsets are converted before they are validated)
    c, o = batches[0]
    o2 = o.copy()
    o2[1:] += 400
    c2 = np.concatenate([np.full(400, ord("A"), np.uint8), c])
    bad = (torch.from_numpy(c2).to(gpu), torch.from_numpy(o2.astype(np.int32)).to(gpu))
    with pytest.raises(RuntimeError, match="seq len"):
        multi.onehot_packed_multi(tok, [dev[2], bad], P, "f")
    ok32 = [(c, o.to(torch.int32)) for c, o in dev]
    got = multi.onehot_packed_multi(tok, ok32, P, "b")
    for (c, o), g in zip(dev, got):
        assert torch.equal(g, tok.onehot_packed(c, o, P, "b"))


def test_token_multi_validates_int32_offsets(gpu, bsq):
    """the shared helper's fix: tokenize_packed_multi validates int32 offsets as the int64 offsets they are converted to"""
    import torch
    from bioseq_amd import multi
    tok = _tokenizer(bsq)
    P = 160
    c, o = _batch(160, 1024, 0, P - 2, "ACGT")
    o2 = o.copy()
    o2[1:] += 400
    c2 = np.concatenate([np.full(400, ord("A"), np.uint8), c])
    bad = (torch.from_numpy(c2).to(gpu), torch.from_numpy(o2.astype(np.int32)).to(gpu))
    with pytest.raises(RuntimeError, match="seq len"):
        multi.tokenize_packed_multi(tok, [bad], P, "b")


def _tokenizer(bsq):
    return bsq.Tokenizer("DNA4", True, True, True)
