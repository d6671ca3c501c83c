"""Device decode (k_decode_sizes, k_scan_rows, k_decode_write) and k_argmax_tokens of bsq_decode.hip at the edges their first tests do
not reach, judged by tests/decode_twin.py (pinned in tests/test_decode_twin_host.py): the row scan's carry past 1024 rows and its
partial last step, rows of different lengths, negative ids and ids past 32 bits, the invalid-token report decided between workgroups,
raw bytes and guard regions through the C ABI, and the argmax for every logit kind, both token sizes, row strides, the grid-stride lap
and the orderings of inf, NaN, signed zero, subnormals and values that tie in `float` only.  Every comparison is exact: f16 and bf16
convert to float64 without rounding, so the argmax reference is exact too."""
import ctypes

import numpy as np
import pytest

import decode_twin as twin

pytestmark = pytest.mark.gpu

KEYS = (("DNA", "111"), ("AMINO20", "111"), ("DNA", "000"))
SHAPES = ((1023, 3), (1024, 3), (1025, 3),    # the row scan's first step boundary (1024 rows per step)
          (2049, 5),                          # three steps, partial last
          (4099, 1),                          # one token per row
          (1030, 130))                        # three 64-token wave steps per row
NP_TYPES = (np.uint8, np.int16, np.int32, np.int64)
F32, F64, F16, BF16 = range(4)                # BSQ_LOGITS_* (include/bsq.h)


def outcome(fn, *args):
    try:
        return ("ok", fn(*args))
    except Exception as e:  # noqa: BLE001 -- the outcome IS what is compared
        return ("raise", type(e).__name__, str(e))


def tokenizer(bsq, key, flags):
    return bsq.Tokenizer(key, int(flags[0]), int(flags[1]), int(flags[2]))


def ids_of(lut):
    """(single-byte ids >= 0, five-byte special ids) of a table"""
    t = twin.table(lut)
    return (np.array(sorted(k for k, v in t.items() if k >= 0 and len(v) == 1), dtype=np.int64),
            np.array(sorted(k for k, v in t.items() if len(v) == 5), dtype=np.int64))


def ragged_tokens(rng, lut, shape):
    """Row r holds r % ncols five-byte specials (at random columns) among single-byte ids: row lengths differ from row to row, so a
    wrong carry or row offset shifts every later row.  Without specials (flags 000): uniformly random ids."""
    singles, specials = ids_of(lut)
    nrows, ncols = shape
    toks = rng.choice(singles, size=shape)
    if specials.size:
        want = np.arange(nrows) % ncols
        order = np.argsort(rng.random(shape), axis=1)                  # a random permutation of the columns per row
        mask = order < want[:, None]
        toks[mask] = rng.choice(specials, size=int(mask.sum()))
        assert (mask.sum(axis=1) == want).all()
    return toks


def device_views(t):
    return (t, t.T, t[:, ::3])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("key,flags", KEYS)
def test_decode_many_rows_of_different_lengths(gpu, bsq, alphabets_golden, key, flags, shape):
    import torch
    lut = twin.golden_table(alphabets_golden, key, flags)
    tok = tokenizer(bsq, key, flags)
    rng = np.random.default_rng(shape[0] * 131 + shape[1])
    singles, specials = ids_of(lut)
    mats = [ragged_tokens(rng, lut, shape), rng.choice(np.concatenate([singles, specials]), size=shape)]
    if specials.size:
        lens = [len(s) for s in twin.decode(lut, mats[0])]
        assert len(set(lens[:shape[1]])) == min(shape[1], shape[0])    # row r is r % ncols specials longer than ncols
    for m, toks in enumerate(mats):
        wants = [twin.decode(lut, v) for v in (toks, toks.T, toks[:, ::3])]
        for np_dt in NP_TYPES if m == 0 else (np.uint8, np.int64):
            dev = torch.from_numpy(toks.astype(np_dt)).to(gpu)
            for view, want in zip(device_views(dev), wants):
                assert tok.decode_tokens(view) == want, (np_dt, tuple(view.shape), view.stride())


@pytest.mark.parametrize("key,flags", KEYS)
def test_negative_and_wide_ids(gpu, bsq, alphabets_golden, key, flags):
    """tokenize.h:107-124, 145-146: int32 / int64 -1 is the reference's key -1 ("\\x00" in its dump); an int64 item counts by its low
    32 bits.  In rows on both sides of the scan's 1024-row step."""
    import torch
    lut = twin.golden_table(alphabets_golden, key, flags)
    assert lut["-1"] == "\x00"
    tok = tokenizer(bsq, key, flags)
    rng = np.random.default_rng(77)
    base = ragged_tokens(rng, lut, (1500, 7))
    base[rng.random(base.shape) < 0.2] = -1
    base[[0, 1023, 1024, 1499, 1499], [0, 6, 3, 6, 0]] = -1
    base[1100, 2] = ids_of(lut)[0][-1]
    i32 = base.astype(np.int32)
    i64 = base + (rng.choice(np.array([0, 0, 1, -1, 5, 2 ** 31 - 1, -2 ** 31 + 1]), size=base.shape) << 32)   # the same low 32 bits
    i64[1100, 2] = 2 ** 32 + int(base[1100, 2])
    i64[1499, 0] = 2 ** 32 - 1
    want = twin.decode(lut, i32)
    assert twin.decode(lut, i64) == want and want[1024].count("\x00") >= 1 and want[1499][-1] == "\x00"
    for host in (i32, i64):
        dev = torch.from_numpy(host).to(gpu)
        for view, ref in zip(device_views(dev), (host, host.T, host[:, ::3])):
            assert tok.decode_tokens(view) == twin.decode(lut, ref)
        assert tok.decode_tokens(dev[1024]) == want[1024]


def test_first_invalid_token_across_workgroups(gpu, bsq, alphabets_golden):
    """The report is a minimum over a flat index taken by 500 workgroups (4 rows each): the one named is the first in the row-major
    order of the VIEW that was passed."""
    import torch
    lut = twin.golden_table(alphabets_golden, "DNA", "111")
    tok = tokenizer(bsq, "DNA", "111")
    rng = np.random.default_rng(3)
    for np_dt in NP_TYPES:
        host = ragged_tokens(rng, lut, (2000, 40)).astype(np_dt)
        host[1500, 3], host[7, 39], host[7, 38] = 101, 102, 103
        dev = torch.from_numpy(host).to(gpu)
        assert outcome(tok.decode_tokens, dev) == outcome(twin.decode, lut, host) == ("raise", "RuntimeError", "Unexpected/invalid token 103")
        # the transposed view: (3, 1500) comes before (38, 7) and (39, 7)
        assert outcome(tok.decode_tokens, dev.T) == outcome(twin.decode, lut, host.T) == ("raise", "RuntimeError", "Unexpected/invalid token 101")
        assert outcome(tok.decode_tokens, dev[:, ::3]) == outcome(twin.decode, lut, host[:, ::3]) == \
            ("raise", "RuntimeError", "Unexpected/invalid token 102")      # columns 3 and 39 are kept: (7, 13) of the view is first
        # the smallest flat index in the LAST row (and the last workgroup)
        host = ragged_tokens(rng, lut, (2000, 40)).astype(np_dt)
        host[1999, 30], host[1999, 5] = 104, 105
        dev = torch.from_numpy(host).to(gpu)
        assert outcome(tok.decode_tokens, dev) == outcome(twin.decode, lut, host) == ("raise", "RuntimeError", "Unexpected/invalid token 105")
        assert outcome(tok.decode_tokens, dev.T) == outcome(twin.decode, lut, host.T) == ("raise", "RuntimeError", "Unexpected/invalid token 105")


@pytest.mark.parametrize("dtype,value,text", [
    ("int32", -5, 4294967291), ("int8", -1, 255), ("int16", -1, 65535), ("int64", 2 ** 32 + 99, 99),
    ("int32", 2 ** 31 - 1, 2 ** 31 - 1), ("int32", -2 ** 31, 2 ** 31), ("int64", 2 ** 31 - 1, 2 ** 31 - 1), ("int64", -2 ** 31, 2 ** 31),
    ("int32", 2 ** 31 - 128, 2 ** 31 - 128), ("int32", -129, 4294967167), ("int32", 512, 512), ("int64", -5, 4294967291)])
def test_invalid_token_text_is_the_uint32_value(gpu, bsq, alphabets_golden, dtype, value, text):
    """The message carries the item as the reference read it.  INT32_MAX and its neighbours are where `value - (-128)` overflows int32."""
    import torch
    lut = twin.golden_table(alphabets_golden, "DNA", "111")
    tok = tokenizer(bsq, "DNA", "111")
    host = ragged_tokens(np.random.default_rng(8), lut, (1100, 6)).astype(dtype)
    clean = host.copy()
    good = torch.from_numpy(clean).to(gpu)
    host[1050, 4] = value
    dev = torch.from_numpy(host).to(gpu)
    want = outcome(twin.decode, lut, host)
    assert want == ("raise", "RuntimeError", "Unexpected/invalid token %d" % text)
    assert outcome(tok.decode_tokens, dev) == want
    assert outcome(tok.decode_tokens, dev[1050]) == want
    # the flag lives in the stream's shared workspace: the next call on the stream starts clean
    assert tok.decode_tokens(good) == twin.decode(lut, clean)


# ---------------------------------------------------------------- the C ABI: bytes, guards, refusals

@pytest.fixture(scope="module")
def lib(gpu):
    from bioseq_amd import capi
    return capi.load()


def raw_decode(lib, desc, dev, nrows, ncols, row_stride, col_stride, stream, itemsize=None):
    """sizes + write through the C ABI on `stream`, the text between two 64-byte guard regions: (offsets, total, bytes)."""
    import torch
    itemsize = dev.element_size() if itemsize is None else itemsize
    offs = torch.full((nrows + 1 + 16,), -3, dtype=torch.int64, device=dev.device)    # 16 guard words behind row_offsets[nrows]
    torch.cuda.synchronize()
    total, bad = ctypes.c_int64(-7), ctypes.c_int64(-7)
    sp = ctypes.c_void_p(stream.cuda_stream)
    st = lib.bsq_decode_sizes_device(ctypes.byref(desc), dev.data_ptr(), itemsize, nrows, ncols, row_stride, col_stride, offs.data_ptr(),
                                     ctypes.byref(total), ctypes.byref(bad), sp)
    assert (st, bad.value) == (twin.OK, -1)
    out = torch.full((64 + total.value + 64,), 0xA5, dtype=torch.uint8, device=dev.device)
    torch.cuda.synchronize()
    st = lib.bsq_decode_write_device(ctypes.byref(desc), dev.data_ptr(), itemsize, nrows, ncols, row_stride, col_stride, offs.data_ptr(),
                                     out.data_ptr() + 64, sp)
    assert st == twin.OK
    stream.synchronize()
    offs, out = offs.cpu().numpy(), out.cpu().numpy()
    assert (offs[nrows + 1:] == -3).all()
    assert (out[:64] == 0xA5).all() and (out[64 + total.value:] == 0xA5).all(), "a guard region was written"
    return offs[:nrows + 1], total.value, out[64:64 + total.value].tobytes()


def test_raw_decode_bytes_offsets_and_guards(lib, gpu, alphabets_golden):
    """BYTES with flags 111: ids 0..127 and -128..-1 are all valid and the pieces of the negative ones are bytes >= 0x80, which no
    Python string carries -- so through the C ABI, on a side stream."""
    import torch
    from bioseq_amd import capi
    lut = twin.golden_bytes_table(alphabets_golden, "BYTES", "111")
    desc = capi.make_desc("BYTES", True, True, True)
    rng = np.random.default_rng(21)
    nrows, ncols = 1100, 70
    host = rng.integers(-128, 128, size=(nrows, ncols)).astype(np.int32)
    order = np.argsort(rng.random(host.shape), axis=1)
    mask = order < (np.arange(nrows) % ncols)[:, None]                 # row r: r % 70 specials
    host[mask] = rng.integers(256, 259, size=int(mask.sum()))
    host[0, :4] = (-128, -1, 127, 0)
    dev = torch.from_numpy(host).to(gpu)
    stream = torch.cuda.Stream(device=gpu)
    for view, (nr, nc, rs, cs) in ((host, (nrows, ncols, ncols * 4, 4)), (host.T, (ncols, nrows, 4, ncols * 4))):
        rows = twin.decode(lut, view)
        offs, total, text = raw_decode(lib, desc, dev, nr, nc, rs, cs, stream)
        assert offs.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in rows])]).tolist()
        assert total == offs[-1] == sum(len(r) for r in rows)
        assert text == b"".join(rows)
    assert twin.decode(lut, host)[0][:4] == b"\x80\xff\x7f\x00"


def test_raw_decode_empty_and_refusals(lib, gpu):
    import torch
    from bioseq_amd import capi
    desc = capi.make_desc("BYTES", True, True, True)
    dev = torch.zeros((8, 6), dtype=torch.int32, device=gpu)
    offs = torch.full((9,), -3, dtype=torch.int64, device=gpu)
    torch.cuda.synchronize()
    total, bad = ctypes.c_int64(-7), ctypes.c_int64(-7)

    def sizes(ptr, itemsize, nrows, ncols, rs, cs):
        return lib.bsq_decode_sizes_device(ctypes.byref(desc), ptr, itemsize, nrows, ncols, rs, cs, offs.data_ptr(), ctypes.byref(total),
                                           ctypes.byref(bad), None)

    def write(ptr, itemsize, nrows, ncols, rs, cs, out):
        return lib.bsq_decode_write_device(ctypes.byref(desc), ptr, itemsize, nrows, ncols, rs, cs, offs.data_ptr(), out.data_ptr(), None)

    assert sizes(dev.data_ptr(), 4, 0, 6, 24, 4) == capi.OK           # no rows: row_offsets[0] = 0, total 0
    torch.cuda.synchronize()
    assert (total.value, bad.value) == (0, -1) and offs.cpu().tolist() == [0] + [-3] * 8
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device=gpu)
    assert write(dev.data_ptr(), 4, 0, 6, 24, 4, out) == capi.OK
    for itemsize in (0, 3, 5, 16):
        assert sizes(dev.data_ptr(), itemsize, 8, 6, 24, 4) == capi.ERR_DTYPE
    for ptr, itemsize, rs, cs in ((dev.data_ptr() + 2, 4, 24, 4), (dev.data_ptr(), 4, 26, 4), (dev.data_ptr(), 4, 24, 6),
                                  (dev.data_ptr() + 4, 8, 48, 8), (dev.data_ptr() + 1, 2, 24, 4)):
        assert sizes(ptr, itemsize, 4, 3, rs, cs) == capi.ERR_INVALID_ARG
    assert sizes(None, 4, 8, 6, 24, 4) == capi.ERR_INVALID_ARG and sizes(dev.data_ptr(), 4, -1, 6, 24, 4) == capi.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all() and offs.cpu().tolist() == [0] + [-3] * 8   # a refused call writes nothing
    # (the write entry point is not called for a matrix the sizes call refused)


# ---------------------------------------------------------------- argmax through the C ABI

def torch_kind(kind):
    import torch
    return {F32: torch.float32, F64: torch.float64, F16: torch.float16, BF16: torch.bfloat16}[kind]


def raw_argmax(lib, logits, kind, n, C, row_stride, token_itemsize, stream=None):
    """tokens of logits (device tensor, n * row_stride items) between two 16-byte guards; (status, tokens as int64, guards intact)."""
    import torch
    buf = torch.full((16 + n * token_itemsize + 16,), 0xA5, dtype=torch.uint8, device=logits.device)
    torch.cuda.synchronize()
    st = lib.bsq_argmax_tokens_device(logits.data_ptr(), kind, n, C, row_stride, buf.data_ptr() + 16, token_itemsize, stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    body = host[16:16 + n * token_itemsize]
    intact = bool((host[:16] == 0xA5).all() and (host[16 + n * token_itemsize:] == 0xA5).all())
    return st, body.view(np.uint8 if token_itemsize == 1 else np.int32).astype(np.int64), intact


def planted_rows(kind, C):
    """[(fill, {channel: value}, expected token)] -- orderings a comparison can get wrong; all values exact in the logit kind."""
    inf, nan, last = float("inf"), float("nan"), C - 1
    if C == 1:
        return [(0.25, {}, 0), (-inf, {}, 0), (nan, {}, 0), (inf, {}, 0), (-0.0, {}, 0)]
    mid = C // 2
    rows = [(0.25, {}, 0),                                   # all equal
            (-inf, {}, 0),                                   # all -inf
            (-1.0, {mid: inf, last: inf}, mid),              # +inf twice: the first
            (-1.0, {0: -0.0, 1: 0.0}, 0),                    # signed zeros are equal: the first
            (-1.0, {0: 0.0, 1: -0.0}, 0),
            (-1.0, {last - 1: -0.0, last: 0.0}, last - 1),
            (1.0, {last: nan}, last),                        # NaN only in the last channel
            (1.0, {0: nan, last: inf}, 0),                   # NaN in channel 0, +inf later
            (nan, {}, 0),                                    # all NaN
            (1.0, {0: 100.0, 1: nan}, 1),                    # NaN after the maximum
            (1.0, {mid: nan, last: nan}, mid),               # the first NaN
            (-2.0, {last: -1.5}, last),                      # the maximum in the last channel (255 of 256 in uint8)
            (-inf, {last: -3.0e4}, last)]
    if kind == F16:
        tiny = 2.0 ** -24                                    # the smallest f16 subnormal
        rows += [(0.0, {0: 65472.0, last: 65504.0}, last), (0.0, {0: 65504.0, last: 65472.0}, 0),
                 (0.0, {last: tiny}, last), (-tiny, {last: tiny}, last), (-tiny, {0: 0.0}, 0), (tiny, {0: 0.0}, 1),
                 (-65504.0, {last: -65472.0}, last)]
    if kind == BF16:
        tiny = 2.0 ** -133                                   # the smallest bf16 subnormal (a subnormal of float as well)
        rows += [(0.0, {last: tiny}, last), (-tiny, {last: tiny}, last), (-tiny, {0: 0.0}, 0), (tiny, {0: 0.0}, 1),
                 (1.0, {last: 1.0078125}, last), (1.0078125, {0: 1.0}, 1), (256.0, {mid: 258.0}, mid), (-258.0, {last: -256.0}, last),
                 (0.0, {0: (2 - 2.0 ** -7) * 2.0 ** 127, last: (2 - 2.0 ** -6) * 2.0 ** 127}, 0)]   # the two largest finite bf16
    if kind == F32:
        tiny = 2.0 ** -149
        rows += [(0.0, {last: tiny}, last), (-tiny, {0: 0.0}, 0), (1.0, {last: 1.0 + 2.0 ** -23}, last), (16777216.0, {last: 16777218.0}, last)]
    if kind == F64:
        rows += [(1.0, {last: 1.0 + 2.0 ** -40}, last),      # ties in float
                 (1.0 + 2.0 ** -40, {0: 1.0}, 1),
                 (1e300, {last: 1e301}, last),               # both inf in float
                 (1e301, {0: 1e300}, 1),
                 (-1e301, {0: -1e300}, 0),                   # both -inf in float
                 (-1e301, {last: -1e300}, last),
                 (0.0, {last: 5e-324}, last),                # zero in float
                 (-1e-300, {mid: 1e-300}, mid)]
    return rows


def logits_matrix(kind, n, C, row_stride, seed):
    """(device-ready torch CPU tensor [n, row_stride] of the kind, float64 numpy view of its first C channels, planted expectations)"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((n, row_stride), generator=g, dtype=torch.float64)
    x = (x * 4).round() / 4 if seed % 2 else x                # (quantised: many exact ties between channels)
    planted = {}
    for k, (fill, at, want) in enumerate(planted_rows(kind, C)):
        r = 13 + 31 * k
        assert r < n
        x[r, :C] = fill
        for c, v in at.items():
            x[r, c] = v
        planted[r] = want
    x[:, C::2] = float("inf")                                 # the padding behind the channels must never win
    x[:, C + 1::2] = float("nan")
    t = x.to(torch_kind(kind))
    return t, t[:, :C].to(torch.float64).numpy(), planted


@pytest.mark.parametrize("C", (1, 2, 23, 255, 256, 257, 300))
@pytest.mark.parametrize("kind", (F32, F64, F16, BF16), ids=("f32", "f64", "f16", "bf16"))
def test_argmax_channel_classes_strides_and_orderings(lib, gpu, kind, C):
    n = 703                                                   # three workgroups, the planted rows (13 + 31 k) spread over them
    for row_stride in (C, C + 5):
        t, ref, planted = logits_matrix(kind, n, C, row_stride, seed=C * 8 + kind * 2 + (row_stride > C))
        want = twin.argmax(ref)
        assert {r: int(want[r]) for r in planted} == planted   # the twin and the hand-written expectations agree
        dev = t.to(gpu)
        for token_itemsize in ((1, 4) if C <= 256 else (4,)):
            st, got, intact = raw_argmax(lib, dev, kind, n, C, row_stride, token_itemsize)
            assert st == twin.OK and intact
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (row_stride, token_itemsize, bad[:8], got[bad[:8]], want[bad[:8]])
    if C >= 255:
        assert want.max() == C - 1                              # (the top channel is reached: 255 in a uint8 token)


@pytest.mark.parametrize("kind,token_itemsize", ((F16, 1), (F32, 4)), ids=("f16-u8", "f32-i32"))
def test_argmax_grid_stride_lap(lib, gpu, kind, token_itemsize):
    """The grid is capped at 256 * 64 workgroups of 256 rows: row 4 194 304 is the first of the second lap.  Every row is checked."""
    import torch
    n = 256 * 64 * 256 + 257
    g = torch.Generator(device="cpu").manual_seed(40 + kind)
    x = torch.randint(-3, 4, (n, 2), generator=g, dtype=torch.int8).to(torch.float32) / 4     # ties in a seventh of the rows
    x[torch.rand((n, 2), generator=g) < 0.01] = float("nan")
    t = x.to(torch_kind(kind))
    want = twin.argmax(t.to(torch.float64).numpy())
    assert 0.3 < want.mean() < 0.5 and 0.3 < want[-257:].mean() < 0.6
    st, got, intact = raw_argmax(lib, t.to(gpu), kind, n, 2, 2, token_itemsize)
    assert st == twin.OK and intact
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


def test_argmax_refusals(lib, gpu):
    import torch
    from bioseq_amd import capi
    dev = torch.zeros((4, 300), dtype=torch.float32, device=gpu)
    buf = torch.full((16 + 4 * 4 + 16,), 0xA5, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()

    def call(kind, n, C, row_stride, token_itemsize, logits=dev.data_ptr(), tokens=buf.data_ptr() + 16):
        return lib.bsq_argmax_tokens_device(logits, kind, n, C, row_stride, tokens, token_itemsize, None)

    assert call(F32, 4, 257, 257, 1) == capi.ERR_INVALID_ARG          # uint8 tokens cannot hold channel 256
    assert call(F32, 4, 23, 22, 1) == capi.ERR_INVALID_ARG            # row_stride < C
    assert call(F32, 4, 300, 299, 4) == capi.ERR_INVALID_ARG
    assert call(F32, 4, 0, 0, 4) == capi.ERR_INVALID_ARG
    assert call(F32, -1, 23, 23, 4) == capi.ERR_INVALID_ARG
    assert call(F32, 4, 23, 23, 2) == capi.ERR_DTYPE
    assert call(7, 4, 23, 23, 4) == capi.ERR_DTYPE
    assert call(F32, 4, 23, 23, 4, logits=None) == capi.ERR_INVALID_ARG
    assert call(F32, 4, 23, 23, 4, tokens=None) == capi.ERR_INVALID_ARG
    assert call(F32, 0, 23, 23, 1) == capi.OK                         # n == 0: nothing to do
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all()                          # none of them wrote a token


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16", "float64"])
def test_decode_logits_int32_token_path(gpu, bsq, alphabets_golden, dtype):
    """C = 259 (BYTES with flags 111) takes the int32 tokens; the winners are ASCII letters and the three specials, so the texts are
    strings."""
    import torch
    lut = twin.golden_bytes_table(alphabets_golden, "BYTES", "111")
    tok = bsq.Tokenizer("BYTES", 1, 1, 1)
    C = tok.alphabet_size()
    assert C == 259
    B, L = 5, 41
    rng = np.random.default_rng(12)
    letters = np.concatenate([np.arange(65, 91), np.arange(97, 123), [256, 257, 258, 256, 257, 258]])
    ids = rng.choice(letters, size=(B, L))
    g = torch.Generator(device="cpu").manual_seed(6)
    big = torch.randn((B, L, C + 41), generator=g).clamp_(-5, 5)
    big[:, :, C:] = 99.0                                                # behind the channels of the non-contiguous input
    flat = big[:, :, :C]
    flat[torch.arange(B)[:, None], torch.arange(L)[None, :], torch.from_numpy(ids)] = 50.0
    big = big.to(getattr(torch, dtype))
    am = twin.argmax(big[:, :, :C].to(torch.float64).numpy().reshape(B * L, C)).reshape(B, L)
    assert (am == ids).all()
    want = [r.decode("ascii") for r in twin.decode(lut, am)]
    want_t = [r.decode("ascii") for r in twin.decode(lut, am.T)]
    dev = big.to(gpu)
    view = dev[:, :, :C]                                                # non-contiguous, channels still adjacent
    assert not view.is_contiguous()
    assert tok.decode_logits(view.contiguous()) == want                 # (B, L, C)
    assert tok.decode_logits(view) == want                              # the same, non-contiguous
    assert tok.decode_logits(view.transpose(0, 1).contiguous(), batch_first=False) == want     # (L, B, C)
    assert tok.decode_logits(view.transpose(0, 1), batch_first=False) == want
    assert tok.decode_logits(view.contiguous(), batch_first=False) == want_t                  # read as (L, B, C): the other order
    assert tok.decode_logits(view[2]) == want[2]                        # (L, C) -> str
    assert any("<EOS>" in w for w in want) and any("<BOS>" in w for w in want) and any("<PAD>" in w for w in want)
