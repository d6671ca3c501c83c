"""GPU: the thresholded pair list of sketch matrices (bioseq_amd.sketch.sketch_pairs, bsq_sketch_pairs_count_device /
bsq_sketch_pairs_emit_device) against the numpy twin (tests/sketch_pairs_twin.py) and the library's host twin, byte for byte: partial
strips and tiles, the widest sketch, every split of a strip's tiles into segments, the upper form with its diagonal and skipped tiles,
every kind of threshold, the cut at max_pairs with guards around the arrays, real sketches with a planted near-duplicate, and the Python
surface."""
import ctypes

import numpy as np
import pytest

import minhash_twin
import sketch_pairs_twin as twin

pytestmark = pytest.mark.gpu

I32, U64 = 2, 3


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _same(got, exp):
    import torch
    kinds = (torch.int64, torch.int64, torch.int32, torch.int32, torch.int64)
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.dtype == kinds[k] and g.is_contiguous() and tuple(g.shape) == e.shape, "array %d: type or shape" % k
        assert g.cpu().numpy().tobytes() == e.tobytes(), "array %d differs" % k


def _check(gpu, Ba, Bb, S, dtype, upper=False, segments=(None,)):
    """sketch_pairs == the numpy twin == the host twin for every threshold of the case and every segment count; the middle threshold is
    not vacuous; ("all") match and either are sketch_compare's.  Returns (a, b, device a, device b)."""
    from bioseq_amd import sketch
    a, b = twin.case(Ba * 1000 + S, Ba, Bb, S, dtype, upper)
    compared = minhash_twin.compare(a, a if upper else b)
    da, db = _dev(a, gpu), None if upper else _dev(b, gpu)
    for name, min_match, T in twin.thresholds(S):
        exp = twin.pairs(a, b, min_match, T, compared)
        total, dense = len(exp[0]), Ba * (Ba - 1) // 2 if upper else Ba * Bb
        if name == "all":
            assert total == dense
        elif name == "mid" and Ba >= 3:
            assert 0 < total < dense and (np.diff(exp[4]) == 0).any() and (np.diff(exp[4]) > 0).any()
        elif name == "equal" and Ba >= 3:
            assert total == (3 if upper else 2)
        elif name == "none":
            assert total == 0
        host = sketch.sketch_pairs_host(a, b, min_jaccard=T / 65536, min_match=min_match)
        assert all(h.tobytes() == e.tobytes() for h, e in zip(host, exp)), (name, "host twin")
        for seg in segments:
            got = sketch.sketch_pairs(da, db, min_jaccard=T / 65536, min_match=min_match, segments=seg)
            _same(got, exp)
            if name == "all" and not upper:
                m, e = sketch.sketch_compare(da, db)
                assert bool((got[2] == m.reshape(-1)).all()) and bool((got[3] == e.reshape(-1)).all())
    only = sketch.sketch_pairs(da, db, min_jaccard=0.0, min_match=0, either=False)
    assert only[3] is None and only[2].numel() == (Ba * (Ba - 1) // 2 if upper else Ba * Bb)
    return a, b, da, db


@pytest.mark.parametrize("Ba, Bb, S", [(1, 1, 1), (3, 5, 7), (65, 130, 100), (33, 257, 16384)])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_pairs_equal_the_twins(gpu, bsq, Ba, Bb, S, dtype):
    """Partial strips and partial tiles; S = 16384: 512 chunks of 32 buckets, the widest sketch."""
    _check(gpu, Ba, Bb, S, dtype)


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_every_split_into_segments_gives_one_result(gpu, bsq, dtype):
    """200 x 330: four strips, six j tiles; 6 segments: one tile each, 64: clamped to 6, 4: segments of one and of two tiles."""
    from bioseq_amd import capi
    L = capi.load()
    assert [L.bsq_sketch_pairs_segments(200, 330, n) for n in (1, 2, 4, 6, 64)] == [1, 2, 4, 6, 6]
    _check(gpu, 200, 330, 64, dtype, segments=(None, 1, 2, 4, 6, 64))


def test_more_than_2_20_row_segment_entries(gpu, bsq):
    """16 400 rows x 64 segments: beyond 2^20 (row, segment) entries the sums of 64 counts are scanned by a launch of their own.  One
    bucket per row, so the rule is restated in a line: the pair passes when the two values are equal and not EMPTY."""
    from bioseq_amd import sketch
    Ba, Bb = 16400, 4096
    name = sketch.sketch_pairs_kernel_name(Ba, Bb, 64)
    assert "k_sketch_pairs_scan" in name and "k_sketch_pairs_scan" not in sketch.sketch_pairs_kernel_name(Ba - 16, Bb, 64)
    rng = np.random.default_rng(9)
    a, b = rng.integers(-1, 64, (Ba, 1)).astype(np.int32), rng.integers(-1, 64, (Bb, 1)).astype(np.int32)
    erow, ecol = np.nonzero((a == b.T) & (a != -1))
    assert 500000 < erow.size < 2000000
    row, col, match, either, offs = sketch.sketch_pairs(_dev(a, gpu), _dev(b, gpu), min_jaccard=1.0, segments=64)
    assert np.array_equal(row.cpu().numpy(), erow) and np.array_equal(col.cpu().numpy(), ecol)
    assert bool((match == 1).all()) and bool((either == 1).all())
    assert np.array_equal(offs.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(erow, minlength=Ba))]))
    host = sketch.sketch_pairs_host(a, b, min_jaccard=1.0)
    assert np.array_equal(host[0], erow) and np.array_equal(host[1], ecol) and np.array_equal(host[4], offs.cpu().numpy())


@pytest.mark.parametrize("B, S", [(130, 33), (64, 1024)])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_upper_lists_the_pairs_above_the_diagonal(gpu, bsq, B, S, dtype):
    """130 rows: three strips, a diagonal tile in each, with 3 segments skipped tiles in front of a segment's first tile (strip 2 owns
    nothing in segments 0 and 1); 64 rows: the diagonal tile alone.  The result is the cross call's, filtered to i < j."""
    from bioseq_amd import sketch
    a, _, da, _ = _check(gpu, B, B, S, dtype, upper=True, segments=(1, 3))
    T = twin.q16(twin.MID_JACCARD[S])
    for seg in (1, 3):
        row, col, match, either, _ = sketch.sketch_pairs(da, da, min_jaccard=T / 65536, min_match=2, segments=seg)
        up = sketch.sketch_pairs(da, min_jaccard=T / 65536, min_match=2, segments=seg)
        keep = row < col
        assert keep.any() and all(bool((u == x[keep]).all()) and u.numel() == int(keep.sum()) for u, x in zip(up[:4], (row, col, match, either)))


@pytest.mark.parametrize("dtype, upper", [(np.int32, False), (np.int64, True)])
def test_cut_at_max_pairs_and_guards(gpu, bsq, dtype, upper):
    """The raw entry points on a side stream, into 0x5A-filled arrays with guards on both sides, for max_pairs = 0, 1, total - 1, total
    and total + 7: the prefix is the twin's, entries beyond the total and the guards are untouched, pair_offsets[-1] is the true total;
    then `sketch_pairs(max_pairs=N)`: N entries, zeros behind the last pair."""
    import torch
    from bioseq_amd import capi, sketch
    L = capi.load()
    Ba, Bb, S = (130, 130, 33) if upper else (200, 330, 64)
    a, b = twin.case(Ba * 1000 + S, Ba, Bb, S, dtype, upper)
    T = twin.q16(twin.MID_JACCARD[S])
    exp = twin.pairs(a, b, 2, T)
    total = len(exp[0])
    assert total > 8
    da = _dev(a, gpu)
    db = da if upper else _dev(b, gpu)
    code = I32 if dtype == np.int32 else U64
    side = torch.cuda.Stream(device=gpu)
    guard = 16
    for segments in (0, 3):
        rule = capi.SketchPairs(2, T, int(upper), segments)
        nseg = L.bsq_sketch_pairs_segments(Ba, Bb, segments)
        for cap in (0, 1, total - 1, total, total + 7):
            segs = torch.full((Ba * nseg + 1 + 2 * guard,), 0x5A5A5A5A, dtype=torch.int64, device=gpu)
            offs = torch.full((Ba + 1 + 2 * guard,), 0x5A5A5A5A, dtype=torch.int64, device=gpu)
            outs = [torch.full((cap + 2 * guard,), 0x5A5A5A5A, dtype=dt, device=gpu) for dt in (torch.int64, torch.int64, torch.int32, torch.int32)]
            ptrs = [o.data_ptr() + guard * o.element_size() for o in outs]
            side.wait_stream(torch.cuda.current_stream())
            stream = ctypes.c_void_p(side.cuda_stream)
            capi.check(L.bsq_sketch_pairs_count_device(da.data_ptr(), Ba, db.data_ptr(), Bb, S, code, ctypes.byref(rule), segs.data_ptr() + 8 * guard,
                                                       offs.data_ptr() + 8 * guard, stream))
            capi.check(L.bsq_sketch_pairs_emit_device(da.data_ptr(), Ba, db.data_ptr(), Bb, S, code, ctypes.byref(rule), segs.data_ptr() + 8 * guard,
                                                      cap, *ptrs, stream))
            side.synchronize()
            raw = offs.cpu().numpy()
            assert (raw[:guard] == 0x5A5A5A5A).all() and (raw[-guard:] == 0x5A5A5A5A).all() and np.array_equal(raw[guard:-guard], exp[4])
            raw = segs.cpu().numpy()
            assert (raw[:guard] == 0x5A5A5A5A).all() and (raw[-guard:] == 0x5A5A5A5A).all()
            assert raw[guard] == 0 and raw[-guard - 1] == total and np.array_equal(raw[guard:-guard:nseg], exp[4])
            n = min(cap, total)
            for o, e in zip(outs, exp[:4]):
                raw = o.cpu().numpy()
                assert (raw[:guard] == 0x5A5A5A5A).all() and (raw[guard + n:] == 0x5A5A5A5A).all(), "a write past the list or its capacity"
                assert np.array_equal(raw[guard:guard + n], e[:n])
    for cap in (0, 1, total - 1, total, total + 7):
        got = sketch.sketch_pairs(da, None if upper else db, min_jaccard=T / 65536, min_match=2, max_pairs=cap, segments=2)
        n = min(cap, total)
        assert all(g.numel() == cap and np.array_equal(g.cpu().numpy()[:n], e[:n]) and not bool(g[n:].any()) for g, e in zip(got[:4], exp[:4]))
        assert np.array_equal(got[4].cpu().numpy(), exp[4])


def test_real_sketches_with_a_planted_near_duplicate(gpu, bsq):
    """The batch of test_minhash_gpu.test_jaccard_of_real_sketches: 70 random DNA rows (row 0 empty, row 1 shorter than k) and row 70, a
    copy of row 2 with ten substitutions; k = 21, S = 512, canonical.  The list at 0.5 is exactly (2, 70); de-duplication drops row 70
    alone; the empty and the short row pair with nothing at min_match = 1 and with each other at min_match = 0."""
    import torch
    from bioseq_amd import sketch
    rng = np.random.default_rng(23)
    lens = rng.integers(200, 3000, 70)
    lens[:3] = (0, 20, 2000)
    chars = rng.choice(np.frombuffer(b"ACGT" * 25 + b"Na*\xff", np.uint8), int(lens.sum())).astype(np.uint8)
    offs = np.zeros(71, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    edited = chars[offs[2]:offs[3]].copy()
    edited[rng.choice(2000, 10, replace=False)] = ord("A")
    chars = np.concatenate([chars, edited])
    offs = np.concatenate([offs, [offs[-1] + 2000]])
    tok = bsq.Tokenizer("DNA4", False, False, False)
    for dc in ("i", "q"):
        sk = sketch.minhash_packed(tok, _dev(chars, gpu), _dev(offs, gpu), 21, 512, dc, canonical=True)
        row, col, match, either, pair_offsets = sketch.sketch_pairs(sk, min_jaccard=0.5)
        assert row.tolist() == [2] and col.tolist() == [70] and 0.5 * either.item() <= match.item() < either.item()
        assert pair_offsets.tolist() == [0, 0, 0] + [1] * 69
        _same((row, col, match, either, pair_offsets), sketch.sketch_pairs_host(sk.cpu().numpy(), min_jaccard=0.5))
        keep, first = sketch.sketch_duplicates(sk, min_jaccard=0.5)
        assert keep.dtype == torch.bool and first.dtype == torch.int64
        assert keep.tolist() == [True] * 70 + [False] and first.tolist() == list(range(70)) + [2]
        hk, hf = sketch.sketch_duplicates(sk.cpu().numpy(), min_jaccard=0.5)
        assert np.array_equal(keep.cpu().numpy(), hk) and np.array_equal(first.cpu().numpy(), hf)
        keep, first, total = sketch.sketch_duplicates(sk, min_jaccard=0.5, max_pairs=16)  # nothing read back: the total comes along
        assert first.tolist() == list(range(70)) + [2] and total.item() == 1
        assert sketch.sketch_duplicates(sk, min_jaccard=0.5, max_pairs=0)[2].item() == 1  # 1 > 0: the list was cut
        low = sketch.sketch_pairs(sk, min_jaccard=0.0, min_match=1)  # every pair that shares a bucket: none with rows 0 and 1
        assert low[0].numel() >= 1 and int(low[0].min()) >= 2 and int(low[1].min()) >= 3
        cross = sketch.sketch_pairs(sk[:3].contiguous(), sk, min_jaccard=1.0, min_match=0)  # the leakage form, empty rows included
        assert list(zip(cross[0].tolist(), cross[1].tolist())) == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 2)]
        assert sketch.sketch_pairs(sk[:3].contiguous(), sk, min_jaccard=0.5)[1].unique().tolist() == [2, 70]


def test_python_surface_and_refusals(gpu, bsq):
    import torch
    from bioseq_amd import capi, sketch
    a = _dev(twin.sketch_like(np.random.default_rng(0), 70, 16, np.int32), gpu)
    b = _dev(twin.sketch_like(np.random.default_rng(1), 5, 16, np.int32), gpu)
    row, col, match, either, offs = sketch.sketch_pairs(a, b)
    assert row.device == a.device and row.dtype == col.dtype == offs.dtype == torch.int64 and match.dtype == either.dtype == torch.int32
    assert row.shape == col.shape == match.shape == either.shape == (int(offs[-1]),) and offs.shape == (71,)
    for x, y in ((a[:0], b), (a, b[:0])):  # empty sides: nothing listed, the offsets all zero
        got = sketch.sketch_pairs(x, y)
        assert all(g.shape == (0,) for g in got[:4]) and got[4].shape == (x.shape[0] + 1,) and not bool(got[4].any())
    assert sketch.sketch_pairs(a[:0])[4].tolist() == [0]
    got = sketch.sketch_pairs(a, b[:0], max_pairs=3)
    assert all(g.tolist() == [0, 0, 0] for g in got[:4])
    for call in (lambda: sketch.sketch_pairs(a.cpu().numpy(), b.cpu().numpy()), lambda: sketch.sketch_pairs(a.cpu(), b.cpu()),
                 lambda: sketch.sketch_pairs(a, b[:, :5].contiguous()), lambda: sketch.sketch_pairs(a, b.to(torch.int64)),
                 lambda: sketch.sketch_pairs(a.to(torch.float32)), lambda: sketch.sketch_pairs(a[0]), lambda: sketch.sketch_pairs(a.t()),
                 lambda: sketch.sketch_pairs(a, b, min_jaccard=1.01), lambda: sketch.sketch_pairs(a, b, min_jaccard=-0.5),
                 lambda: sketch.sketch_pairs(a, b, min_jaccard=float("nan")), lambda: sketch.sketch_pairs(a, b, min_match=17),
                 lambda: sketch.sketch_pairs(a, b, min_match=-1), lambda: sketch.sketch_pairs(a, b, max_pairs=-1),
                 lambda: sketch.sketch_pairs(a, b, segments=65), lambda: sketch.sketch_pairs(a, b, segments=-1),
                 lambda: sketch.sketch_duplicates(a.cpu())):
        with pytest.raises(ValueError):
            call()
    # the raw entry points refuse before anything is written: upper with Ba != Bb, a bad threshold, a bad type
    L = capi.load()
    segs = torch.full((71,), 0x5A, dtype=torch.int64, device=gpu)
    out = torch.full((71,), 0x5A, dtype=torch.int64, device=gpu)
    for rule, code in ((capi.SketchPairs(1, 0, 1, 0), I32), (capi.SketchPairs(1, 65537, 0, 0), I32), (capi.SketchPairs(17, 0, 0, 0), I32),
                       (capi.SketchPairs(1, 0, 0, 65), I32), (capi.SketchPairs(1, 0, 0, 0), 4)):
        st = L.bsq_sketch_pairs_count_device(a.data_ptr(), 70, b.data_ptr(), 5, 16, code, ctypes.byref(rule), segs.data_ptr(), out.data_ptr(), None)
        assert st in (capi.ERR_INVALID_ARG, capi.ERR_DTYPE)
        st = L.bsq_sketch_pairs_emit_device(a.data_ptr(), 70, b.data_ptr(), 5, 16, code, ctypes.byref(rule), segs.data_ptr(), 8, out.data_ptr(),
                                            out.data_ptr(), out.data_ptr(), None, None)
        assert st in (capi.ERR_INVALID_ARG, capi.ERR_DTYPE)
    torch.cuda.synchronize()
    assert bool((segs == 0x5A).all()) and bool((out == 0x5A).all())
