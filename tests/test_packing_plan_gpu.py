"""GPU: the block scan of the packing plan (count_heads / block_scan / k_pack_heads / k_pack_sums / k_pack_place of bsq_pack.hip) where
row heads lie many sequences apart -- threads and whole blocks of 4096 sequences without a head, more than 256 scan blocks, the rows = N
cut aimed at thread and block boundaries -- against the numpy twin (tests/pack_twin.py) and the library's CPU twins bit for bit; and the
crop -> pack / k-mer / masked-LM loader steps captured into HIP graphs."""
import functools

import numpy as np
import pytest

import kmer_twin
import mlm_twin
import pack_twin as twin
import views_twin
from test_packing_gpu import MODES, NP_OF, _batch, _dev, _tok

pytestmark = pytest.mark.gpu

PER_THREAD, PER_BLOCK, TILE = 16, 4096, 256  # sequences per thread and per block of the scan kernels; blocks per tile of k_pack_sums


def _heads(starts, P):
    """Row-head marks from a next-fit plan: a sequence is a head when its row differs from its predecessor's."""
    row = np.asarray(starts[:-1]) // P
    return np.concatenate([[True], row[1:] != row[:-1]])


def _headless(heads, n):
    """(aligned groups of n sequences without a head, groups in all)."""
    h = np.concatenate([heads, np.zeros(-len(heads) % n, dtype=bool)]).reshape(-1, n)
    return int((~h.any(axis=1)).sum()), h.shape[0]


# ---- 1. wide rows ---------------------------------------------------------------------------------------------------------------
# (key, B, maxlen, P, flags, a block of 4096 without a head is expected)
WIDE = [
    ("DNA4", 20000, 4, 32768, (1, 1, 1), True),     # 3 rows of about 8000 sequences
    ("DNA4", 12000, 3, 65536, (0, 0, 0), True),     # one row, a quarter of the runs of zero width: the only head is sequence 0
    ("AMINO20", 9000, 40, 2048, (1, 1, 0), False),  # about 90 sequences per row: head-less threads next to threads with a head
]
WIDE_IDS = ["B%d-P%d" % (c[1], c[3]) for c in WIDE]


@functools.lru_cache(maxsize=None)
def _wide(case):
    """(chars, offsets, {mode: the twin's pack}) of a WIDE case, computed once for the tests that share it."""
    key, B, maxlen, P, flags, _ = case
    chars, offs = _batch(np.random.default_rng(B + P), key, B, maxlen)
    return chars, offs, {mode: twin.pack(key, flags, chars, offs, P, mode) for mode in MODES}


def _assert_reach(case, exp):
    """The case reaches what it is here for: groups of 16 (and, where expected, blocks of 4096) whose head is carried in from outside."""
    key, B, maxlen, P, flags, headless_block = case
    assert flags[0] + flags[1] > 0 or exp[4] == 1  # (a run of zero width at a row's end would blur the marks)
    heads = _heads(exp[3], P)
    assert int(heads.sum()) == exp[4]
    threads, blocks = _headless(heads, PER_THREAD), _headless(heads, PER_BLOCK)
    print("wide rows B=%d P=%d: %d rows, %d of %d blocks and %d of %d threads without a head" % ((B, P, exp[4]) + blocks + threads))
    assert threads[0] >= 1
    assert blocks[0] >= 1 or not headless_block


@pytest.mark.parametrize("case", WIDE, ids=WIDE_IDS)
def test_wide_rows_plan_equals_the_twins(gpu, bsq, case):
    import torch
    from bioseq_amd import packing
    key, B, maxlen, P, flags, _ = case
    chars, offs, exps = _wide(case)
    _assert_reach(case, exps["nextfit"])
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    tok = _tok(bsq, key, flags)
    for mode in MODES:
        exp = exps[mode]
        starts, n_rows, n_placed = packing.pack_plan(tok, dch, dof, P, mode=mode)
        torch.cuda.synchronize()
        assert int(n_rows) == exp[4] and int(n_placed) == exp[5] == B, mode
        assert np.array_equal(starts.cpu().numpy(), exp[3]), mode
        host = packing.pack_plan_host(tok, offs, P, mode)
        assert np.array_equal(host[0], exp[3]) and host[1:] == (exp[4], B), mode


@pytest.mark.parametrize("case", WIDE, ids=WIDE_IDS)
def test_wide_rows_encode_equals_the_twins(gpu, bsq, case):
    import torch
    from bioseq_amd import packing
    key, B, maxlen, P, flags, _ = case
    chars, offs, exps = _wide(case)
    _assert_reach(case, exps["nextfit"])
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    tok = _tok(bsq, key, flags)
    for mode in MODES:
        exp = exps[mode]
        for dc in "bq":
            got = packing.pack_tokenize_packed(tok, dch, dof, P, dc, mode=mode)
            torch.cuda.synchronize()
            assert int(got.n_rows) == exp[4] and got.tokens.shape == (exp[4], P), (mode, dc)
            assert np.array_equal(got.starts.cpu().numpy(), exp[3]), (mode, dc)
            assert got.tokens.cpu().numpy().tobytes() == exp[0].astype(NP_OF[dc]).tobytes(), (mode, dc)
            assert np.array_equal(got.segment_ids.cpu().numpy(), exp[1]), (mode, dc)
            assert np.array_equal(got.position_ids.cpu().numpy(), exp[2]), (mode, dc)
        host = packing.pack_tokenize_host(tok, chars, offs, P, "q", mode=mode)
        assert host.n_rows == exp[4] and np.array_equal(host.starts, exp[3]), mode
        assert host.tokens.tobytes() == exp[0].astype(np.int64).tobytes(), mode
        assert np.array_equal(host.segment_ids, exp[1]) and np.array_equal(host.position_ids, exp[2]), mode


# ---- 2. more than 256 scan blocks -----------------------------------------------------------------------------------------------
BIG_B, BIG_P, BIG_FLAGS = TILE * PER_BLOCK + PER_BLOCK + 7, 4096, (1, 0, 0)


@functools.lru_cache(maxsize=None)
def _big_offsets():
    lens = np.random.default_rng(BIG_B + BIG_P).integers(0, 3, BIG_B).astype(np.int64)
    offs = np.zeros(BIG_B + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return offs


@functools.lru_cache(maxsize=None)
def _big_plan(mode, rows):
    return twin.plan(_big_offsets(), BIG_P, BIG_FLAGS[0], BIG_FLAGS[1], mode, rows)


@pytest.mark.parametrize("mode, half", [("nextfit", False), ("stream", False), ("nextfit", True)], ids=["nextfit", "stream", "nextfit-half-rows"])
def test_a_second_tile_of_scan_blocks(gpu, bsq, mode, half):
    """258 blocks of 4096 sequences: k_pack_sums walks two tiles, and what the first 256 blocks hand on (carry_c, carry_h) places
    the sequences of blocks 256 and 257.  Plan only."""
    import torch
    from bioseq_amd import packing
    assert -(-BIG_B // PER_BLOCK) == TILE + 2
    offs = _big_offsets()
    whole = _big_plan("nextfit", None)
    heads = _heads(whole[0], BIG_P)
    blocks, threads = _headless(heads, PER_BLOCK), _headless(heads, PER_THREAD)
    print("258 blocks: %d rows, %d of %d blocks and %d of %d threads without a head" % ((whole[1],) + blocks + threads))
    assert whole[1] > 2 and blocks[0] >= 1 and threads[0] >= 1
    assert not heads[TILE * PER_BLOCK:TILE * PER_BLOCK + PER_THREAD].any()  # block 256 opens inside a row: carry_h decides its starts
    assert heads[:TILE * PER_BLOCK].any() and heads[TILE * PER_BLOCK:].any()
    rows = whole[1] // 2 if half else None
    exp = _big_plan(mode, rows)
    assert (exp[2] < BIG_B) == half and exp[2] > 0
    tok = _tok(bsq, "DNA4", BIG_FLAGS)
    dch = torch.zeros(int(offs[-1]), dtype=torch.uint8, device=gpu)
    starts, n_rows, n_placed = packing.pack_plan(tok, dch, _dev(offs, gpu), BIG_P, mode=mode, rows=rows, validate=False)
    torch.cuda.synchronize()
    assert int(n_rows) == exp[1] and int(n_placed) == exp[2]
    assert np.array_equal(starts.cpu().numpy(), exp[0])
    host = packing.pack_plan_host(tok, offs, BIG_P, mode, rows)
    assert np.array_equal(host[0], exp[0]) and host[1:] == exp[1:]


# ---- 3. the rows = N cut at thread and block boundaries -------------------------------------------------------------------------
CUT_P, CUT_B, CUT_FLAGS = 64, PER_BLOCK + 64, (1, 1, 1)
CUT_TARGETS = (15, 16, 17, PER_BLOCK - 1, PER_BLOCK, PER_BLOCK + 1, CUT_B - 1, CUT_B)  # n_placed: the first unplaced sequence


@functools.lru_cache(maxsize=None)
def _cut_batch(full):
    """`full` sequences whose run fills a row, then sequences of 2 characters (runs of P / 16 positions: 16 to a row), CUT_B in all."""
    lens = np.array([CUT_P - 2] * full + [2] * (CUT_B - full), dtype=np.int64)
    chars = np.random.default_rng(full).choice(np.frombuffer(b"ACGTNacgt", np.uint8), int(lens.sum())).astype(np.uint8)
    offs = np.zeros(CUT_B + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return chars, offs


def _cut_for(target):
    """(full, N): N rows over the batch with `full` full-width runs in front place full + 16 * (N - full) sequences."""
    for full in (0, 1, 15):
        N, rest = divmod(target + 15 * full, 16)
        if rest == 0 and N >= max(full, 1):
            return full, N
    raise AssertionError(target)


@pytest.mark.parametrize("target", CUT_TARGETS)
def test_rows_n_cut_at_thread_and_block_boundaries(gpu, bsq, target):
    import torch
    from bioseq_amd import packing
    full, N = _cut_for(target)
    chars, offs = _cut_batch(full)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    tok = _tok(bsq, "DNA4", CUT_FLAGS)
    pad = twin.pad_value("DNA4", CUT_FLAGS)
    w = np.diff(offs) + 2
    for mode in MODES:
        need = twin.plan(offs, CUT_P, 1, 1, mode)[1]
        for rows in ((N, need + 3) if target == CUT_B else (N,)):
            exp = twin.pack("DNA4", CUT_FLAGS, chars, offs, CUT_P, mode, rows=rows, dtype=np.int32)
            assert exp[5] == target and exp[4] == need  # the cut is where this case aims it
            got = packing.pack_tokenize_packed(tok, dch, dof, CUT_P, "i", mode=mode, rows=rows, validate=False)
            torch.cuda.synchronize()
            starts = got.starts.cpu().numpy()
            assert int(got.n_rows) == need and int(got.n_placed) == target, (mode, rows)
            assert np.array_equal(starts, exp[3]), (mode, rows)
            assert (starts[target:CUT_B] == -1).all() and starts[CUT_B] == starts[target - 1] + w[target - 1]
            tokens, seg, pos = got.tokens.cpu().numpy(), got.segment_ids.cpu().numpy(), got.position_ids.cpu().numpy()
            assert tokens.shape == (rows, CUT_P)
            assert np.array_equal(tokens, exp[0]) and np.array_equal(seg, exp[1]) and np.array_equal(pos, exp[2]), (mode, rows)
            assert (tokens[need:] == pad).all() and (seg[need:] == 0).all() and (pos[need:] == 0).all()
            flat = tokens.reshape(-1)
            assert (flat[int(starts[CUT_B]):] == pad).all()
            plan = packing.pack_plan(tok, dch, dof, CUT_P, mode=mode, rows=rows, validate=False)
            assert np.array_equal(plan[0].cpu().numpy(), exp[3]) and int(plan[1]) == need and int(plan[2]) == target
            host = packing.pack_plan_host(tok, offs, CUT_P, mode, rows)
            assert np.array_equal(host[0], exp[3]) and host[1:] == (need, target)


def test_nothing_placed_and_n_placed_zeroed_by_every_call(gpu, bsq):
    """Stream mode, the first run longer than the whole matrix: nothing is placed, starts[B] = 0, every position is PAD.  Then the raw
    plan call over the same output buffers again and again: n_placed is this call's count, not a running sum."""
    import torch
    from bioseq_amd import capi, packing
    L = capi.load()
    B, P, N = 300, 64, 2
    lens = np.full(B, 2, dtype=np.int64)
    lens[0] = N * P + 72
    chars = np.random.default_rng(9).choice(np.frombuffer(b"ACGT", np.uint8), int(lens.sum())).astype(np.uint8)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    tok = _tok(bsq, "DNA4", CUT_FLAGS)
    exp = twin.pack("DNA4", CUT_FLAGS, chars, offs, P, "stream", rows=N, dtype=np.int8)
    assert exp[5] == 0 and exp[3][B] == 0 and (exp[3][:B] == -1).all()
    got = packing.pack_tokenize_packed(tok, dch, dof, P, "b", mode="stream", rows=N, validate=False)
    torch.cuda.synchronize()
    assert int(got.n_placed) == 0 and int(got.n_rows) == exp[4] == -(-int(offs[-1] + 2 * B) // P)
    assert np.array_equal(got.starts.cpu().numpy(), exp[3])
    assert np.array_equal(got.tokens.cpu().numpy(), exp[0]) and bool((got.tokens == twin.pad_value("DNA4", CUT_FLAGS)).all())
    assert not got.segment_ids.any() and not got.position_ids.any()
    host = packing.pack_plan_host(tok, offs, P, "stream", N)
    assert np.array_equal(host[0], exp[3]) and host[1:] == (exp[4], 0)

    starts = torch.full((B + 1,), -77, dtype=torch.int64, device=gpu)
    counts = torch.full((2,), -77, dtype=torch.int64, device=gpu)
    for mode, rows in (("stream", 40), ("stream", 40), ("nextfit", 7), ("nextfit", 7), ("stream", N), ("stream", 40), ("nextfit", 0)):
        e = twin.plan(offs, P, 1, 1, mode, rows or None)
        with capi.launching(gpu) as stream:
            capi.check(L.bsq_pack_plan_device(dof.data_ptr(), B, P, 1, 1, capi.PACK_NEXTFIT if mode == "nextfit" else capi.PACK_STREAM, rows,
                                              starts.data_ptr(), counts.data_ptr(), counts.data_ptr() + 8, stream))
        torch.cuda.synchronize()
        assert counts.cpu().tolist() == [e[1], e[2]], (mode, rows)
        assert np.array_equal(starts.cpu().numpy(), e[0]), (mode, rows)


# ---- 4. the newer loader steps as HIP graphs ------------------------------------------------------------------------------------
STEPS = ("pack-nextfit", "pack-stream", "kmer-stride1", "kmer-stridek", "mlm")


def _lut(key):
    from bioseq_amd import capi
    d = capi.make_desc(key)
    return np.frombuffer(bytes(d.lut), dtype=np.int8), int(d.nchars)


@pytest.mark.parametrize("encode", STEPS)
def test_crop_and_encode_as_one_hip_graph(gpu, bsq, oracle, encode):
    """crop_packed(index=<device tensor>) followed by the packing / k-mer / masked-LM encode are plain stream-ordered launches (the
    header's "never synchronises"; a call that synchronised would fail the capture): captured ONCE into a HIP graph and replayed on
    new index lists written into the same index tensor.  Expected: the views twin composed with the encode's twin for that list, and
    the same step run eagerly.  The seeds of the crop and of the mask are kernel arguments frozen into the graph, so a replay repeats
    the draw of a given row: replaying with the same indices gives the same bytes."""
    import torch
    from bioseq_amd import kmers, masking, packing, views
    n_store, nb, W, K = 2000, 512, 128, 6
    flags = (1, 1, 1)
    rng = np.random.default_rng(31)
    chars, offs = _batch(rng, "DNA4", n_store, 400)
    dch, dof = _dev(chars, gpu), _dev(offs, gpu)
    tok = _tok(bsq, "DNA4", flags)
    idx = torch.zeros(nb, dtype=torch.int64, device=gpu)
    crop = dict(revcomp_frac=0.5, seed=4242)
    lut, A = _lut("DNA4")

    if encode.startswith("pack"):
        mode, P = encode[5:], 512
        N = packing.pack_rows_bound(nb * W, nb, P, tok, mode)

        def enc(vch, vof):
            return tuple(packing.pack_tokenize_packed(tok, vch, vof, P, "b", mode=mode, rows=N, validate=False))

        def expect(e_chars, e_offs):
            t = twin.pack("DNA4", flags, e_chars, e_offs, P, mode, rows=N, dtype=np.int8)
            assert t[5] == nb and 0 < t[4] <= N
            return t[:4] + (np.int64(t[4]), np.int64(t[5]))
    elif encode.startswith("kmer"):
        s = 1 if encode == "kmer-stride1" else K
        P = kmers.kmer_padlen(tok, K, W, stride=s)

        def enc(vch, vof):
            return (kmers.kmer_tokenize_packed(tok, vch, vof, K, P, "h", stride=s, validate=False),)

        def expect(e_chars, e_offs):
            return (kmer_twin.rows_fast(lut, A, e_chars, e_offs, K, s, P, *flags).astype(np.int16),)
    else:
        P = W + 2
        ora = oracle.OracleTokenizer("DNA4", eos=1, bos=1, padchar=1)

        def enc(vch, vof):
            return masking.mlm_tokenize_packed(tok, vch, vof, P, "b", True, frac=0.15, seed=99, validate=False)

        def expect(e_chars, e_offs):
            plain = ora.tokenize_packed(e_chars, e_offs, P, "i", True).astype(np.int64)
            ei, el = mlm_twin.mlm(plain, lut, A, 1, 1, e_chars, e_offs, 0.15, 0.8, 0.1, tok.alphabet_size(), -100, 99, 0)
            assert (el != -100).any()
            return ei.astype(np.int8), el

    def step():
        vch, vof = views.crop_packed(dch, dof, W, index=idx, validate=False, capacity=nb * W, **crop)  # (validate=False: no status read)
        return enc(vch, vof)

    step()                                                            # warm-up outside the capture (tables, scratch)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    pick = None
    for rep in range(4):
        if rep < 3:                                                   # (the fourth replay: the third list once more)
            pick = rng.integers(0, n_store, size=nb)
            pick[:4] = (0, 1, 2, 3)                                   # the empty, the one-character and the longest sequence
            idx.copy_(torch.from_numpy(pick))
        before = [t.clone() for t in out]
        for t in out:
            t.fill_(-3)
        g.replay()
        torch.cuda.synchronize()
        e_chars, e_offs, _, strand = views_twin.crop(chars, offs, W, index=pick, **crop)
        assert 0 < strand.sum() < nb
        want = expect(e_chars, e_offs)
        assert len(want) == len(out)
        for k, (t, e) in enumerate(zip(out, want)):
            assert t.cpu().numpy().tobytes() == np.ascontiguousarray(e).tobytes(), (encode, rep, k)
        eager = step()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager)), (encode, rep)
        if rep == 3:
            assert all(torch.equal(a, b) for a, b in zip(out, before)), "a replay on the same indices drew other bytes"
