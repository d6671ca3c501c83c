"""CPU: the thresholded pair list of sketch matrices (include/bsq.h, "sketch pairs") -- the declared symbols, the header's known answers,
the library's host twin bsq_sketch_pairs_host against the numpy twin (tests/sketch_pairs_twin.py) byte for byte on the shapes the GPU
tests use, the cut at max_pairs, every refusal with the outputs left untouched, the segment rule, and `sketch_duplicates` on a hand-made
chain.  No device is needed."""
import ctypes

import numpy as np
import pytest

import minhash_twin
import sketch_pairs_twin as twin

I32, U64 = 2, 3
E = 4294967295
# (Ba, Bb, S, upper): the shapes of tests/test_sketch_pairs_gpu.py
SHAPES = [(1, 1, 1, False), (3, 5, 7, False), (65, 130, 100, False), (33, 257, 16384, False), (200, 330, 64, False), (130, 130, 33, True),
          (64, 64, 1024, True)]


def _lib():
    from bioseq_amd import capi
    return capi, capi.load()


def _same(got, exp, either=True):
    """the five arrays of a result against the twin's, types included"""
    for k, (g, e) in enumerate(zip(got, exp)):
        if k == 3 and not either:
            assert g is None
            continue
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == e.dtype and g.shape == e.shape and g.tobytes() == e.tobytes(), "array %d differs" % k


def test_new_symbols_are_declared_and_exported():
    import bioseq_amd
    capi, L = _lib()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_sketch_pairs_segments", "bsq_sketch_pairs_count_device", "bsq_sketch_pairs_emit_device", "bsq_sketch_pairs_host",
              "bsq_sketch_pairs_kernel_name"):
        assert n in names and hasattr(L, n), n
    assert L.bsq_abi_version() == 7
    for n in ("sketch_pairs", "sketch_pairs_host", "sketch_duplicates", "sketch_pairs_kernel_name"):
        assert n in bioseq_amd.sketch.__all__ and callable(getattr(bioseq_amd.sketch, n))
    assert ctypes.sizeof(capi.SketchPairs) == 16


def test_known_answers():
    """The answers of include/bsq.h on the plain sketches of the MinHash section's batch, from the numpy twin and the host twin."""
    from bioseq_amd import sketch
    sk = np.array([[1282424135, 2136608625, E, E], [1282424135, 2136608625, E, E], [E] * 4, [E] * 4, [E, E, 1516739009, E]], np.uint32)
    square = [(0, 0), (0, 1), (1, 0), (1, 1), (4, 4)]
    empties = sorted(square + [(2, 2), (2, 3), (3, 2), (3, 3)])
    for dtype in (np.int32, np.int64):
        a = sk.view(np.int32) if dtype == np.int32 else np.where(sk == E, -1, sk.astype(np.int64))
        cases = [(None, 1, 0.5, [(0, 1)], [0, 1, 1, 1, 1, 1]), (a, 1, 1.0, square, [0, 2, 4, 4, 4, 5]), (a, 0, 1.0, empties, [0, 2, 4, 6, 8, 9]),
                 (a, 0, 0.0, [(i, j) for i in range(5) for j in range(5)], [0, 5, 10, 15, 20, 25])]
        for b, min_match, min_jaccard, want, offsets in cases:
            exp = twin.pairs(a, b, min_match, twin.q16(min_jaccard))
            assert list(zip(exp[0].tolist(), exp[1].tolist())) == want and exp[4].tolist() == offsets
            _same(sketch.sketch_pairs_host(a, b, min_jaccard=min_jaccard, min_match=min_match), exp)
        row, col, match, either, _ = sketch.sketch_pairs_host(a, a, min_jaccard=0.0, min_match=0)
        assert (match[1], either[1]) == (2, 2) and (row[4], col[4], match[4], either[4]) == (0, 4, 0, 3)
    assert twin.q16(0.5) == 32768 and twin.q16(1.0) == 65536 and twin.q16(0.0) == 0 and twin.q16(0.9) == 58982


@pytest.mark.parametrize("Ba, Bb, S, upper", SHAPES)
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_host_twin_equals_numpy_twin(Ba, Bb, S, upper, dtype):
    """Every threshold of the GPU tests' cases; the middle one is not vacuous; the cut at max_pairs keeps the prefix and the total."""
    from bioseq_amd import sketch
    a, b = twin.case(Ba * 1000 + S, Ba, Bb, S, dtype, upper)
    compared = minhash_twin.compare(a, a if upper else b)
    for name, min_match, T in twin.thresholds(S):
        exp = twin.pairs(a, b, min_match, T, compared)
        total = len(exp[0])
        if name == "all":
            assert total == (Ba * (Ba - 1) // 2 if upper else Ba * Bb)
        if name == "mid" and Ba >= 3:
            assert 0 < total < (Ba * (Ba - 1) // 2 if upper else Ba * Bb) and (np.diff(exp[4]) == 0).any() and (np.diff(exp[4]) > 0).any()
        if name == "equal" and Ba >= 3:
            assert total == 3 if upper else total == 2
        if name == "none":
            assert total == 0
        _same(sketch.sketch_pairs_host(a, b, min_jaccard=T / 65536, min_match=min_match), exp)
        if name == "mid":
            _same(sketch.sketch_pairs_host(a, b, min_jaccard=T / 65536, min_match=min_match, either=False), exp, either=False)
            for cap in sorted({0, 1, max(total - 1, 0), total, total + 7}):
                got = sketch.sketch_pairs_host(a, b, min_jaccard=T / 65536, min_match=min_match, max_pairs=cap)
                n = min(cap, total)
                assert all(len(x) == cap and np.array_equal(x[:n], e[:n]) and not x[n:].any() for x, e in zip(got[:4], exp[:4]))
                assert np.array_equal(got[4], exp[4])
    if upper:  # the pairs i < j of the cross call
        row, col, match, either, _ = sketch.sketch_pairs_host(a, a, min_jaccard=0.0, min_match=0)
        keep = row < col
        _same(sketch.sketch_pairs_host(a, min_jaccard=0.0, min_match=0)[:4], (row[keep], col[keep], match[keep], either[keep]))


def test_q16_round_trip():
    """min_jaccard = T / 65536 gives back T for every T the tests use (the Python surface rounds, the rule takes T)."""
    for T in [0, 1, 32768, 65535, 65536] + [twin.q16(v) for v in twin.MID_JACCARD.values()]:
        assert int(T / 65536 * 65536 + 0.5) == T


def test_segments_rule():
    capi, L = _lib()
    seg = L.bsq_sketch_pairs_segments
    assert seg(200, 330, 1) == 1 and seg(200, 330, 6) == 6 and seg(200, 330, 64) == 6 and seg(200, 330, 4) == 4  # min(n, tiles_j)
    assert seg(64, 64, 0) == 1 and seg(64, 65, 0) == 2 and seg(64, 64 * 100, 0) == 64  # never more than 64 or the tiles
    assert seg(64 * 4096, 64 * 4096, 0) == 1 and seg(64 * 4097, 64 * 4096, 0) == 1  # the strips alone fill the device
    assert seg(64 * 128, 64 * 128, 0) == 32 and seg(64 * 2048, 64 * 128, 0) == 2  # strips x segments reaches 4096
    assert seg(0, 5, 0) == 1 and seg(5, 0, 7) == 1
    assert seg(-1, 5, 0) == 0 and seg(5, 5, -1) == 0 and seg(5, 5, 65) == 0
    from bioseq_amd import sketch
    assert sketch.sketch_pairs_kernel_name(5, 5) == "k_sketch_pairs<count>+k_sketch_pairs_sums+k_sketch_pairs_place;k_sketch_pairs<emit>"
    assert sketch.sketch_pairs_kernel_name(16384, 4096, 64) == sketch.sketch_pairs_kernel_name(5, 5)  # 2^20 (row, segment) entries
    assert sketch.sketch_pairs_kernel_name(16385, 4096, 64) == \
        "k_sketch_pairs<count>+k_sketch_pairs_sums+k_sketch_pairs_scan+k_sketch_pairs_place;k_sketch_pairs<emit>"
    assert sketch.sketch_pairs_kernel_name(0, 5) == "hipMemsetAsync" and sketch.sketch_pairs_kernel_name(5, 5, 65) == ""


def test_refusals_write_nothing():
    capi, L = _lib()
    a = twin.sketch_like(np.random.default_rng(0), 6, 8, np.int32)
    b = twin.sketch_like(np.random.default_rng(1), 4, 8, np.int32)
    offs = np.full(7, 0x5A, np.int64)
    arrays = [np.full(24, 0x5A, np.int64), np.full(24, 0x5A, np.int64), np.full(24, 0x5A, np.int32), np.full(24, 0x5A, np.int32)]

    def call(rule, Ba=6, Bb=4, S=8, t=I32, max_pairs=24, offsets=offs):
        return L.bsq_sketch_pairs_host(a.ctypes.data, Ba, b.ctypes.data, Bb, S, t, ctypes.byref(capi.SketchPairs(*rule)) if rule else None,
                                       offsets.ctypes.data if offsets is not None else None, max_pairs, *(x.ctypes.data for x in arrays))

    bad = [((1, -1, 0, 0), {}), ((1, 65537, 0, 0), {}),  # T outside 0 .. 65536
           ((9, 0, 0, 0), {}), ((-1, 0, 0, 0), {}),  # min_match outside 0 .. S
           ((1, 0, 1, 0), {}), ((1, 0, 2, 0), {}),  # upper with Ba != Bb; upper not 0 / 1
           ((1, 0, 0, -1), {}), ((1, 0, 0, 65), {}),  # segments outside 0 .. 64
           ((1, 0, 0, 0), {"S": 0}), ((1, 0, 0, 0), {"S": (1 << 14) + 1}), ((1, 0, 0, 0), {"Ba": -1}), ((1, 0, 0, 0), {"max_pairs": -1}),
           ((1, 0, 0, 0), {"offsets": None}), (None, {})]
    for rule, kw in bad:
        assert call(rule, **kw) == capi.ERR_INVALID_ARG and L.bsq_last_error(), (rule, kw)
    for t in (0, 1, 4, 5):
        assert call((1, 0, 0, 0), t=t) == capi.ERR_DTYPE
    assert (offs == 0x5A).all() and all((x == 0x5A).all() for x in arrays)
    assert call((1, 0, 0, 0)) == capi.OK and offs[0] == 0
    # empty sides: BSQ_OK, pair_offsets all zero, nothing else written
    for x in arrays + [offs]:
        x[:] = 0x5A
    assert call((1, 0, 0, 0), Bb=0) == capi.OK and not offs.any() and all((x == 0x5A).all() for x in arrays)
    offs[:] = 0x5A
    assert call((1, 0, 0, 0), Ba=0) == capi.OK and offs[0] == 0 and (offs[1:] == 0x5A).all()
    # the Python surface: ValueError before anything is computed
    from bioseq_amd import sketch
    for refused in (lambda: sketch.sketch_pairs_host(a, b, min_jaccard=1.5), lambda: sketch.sketch_pairs_host(a, b, min_jaccard=-0.1),
                 lambda: sketch.sketch_pairs_host(a, b, min_jaccard=float("nan")), lambda: sketch.sketch_pairs_host(a, b, min_match=9),
                 lambda: sketch.sketch_pairs_host(a, b, min_match=-1), lambda: sketch.sketch_pairs_host(a, b, min_match=1.5),
                 lambda: sketch.sketch_pairs_host(a, b, max_pairs=-1), lambda: sketch.sketch_pairs_host(a, b[:, :5]),
                 lambda: sketch.sketch_pairs_host(a, b.astype(np.int64)), lambda: sketch.sketch_pairs_host(a.astype(np.float32), b),
                 lambda: sketch.sketch_pairs_host(a[0], b)):
        with pytest.raises(ValueError):
            refused()
    row, col, match, either, offsets = sketch.sketch_pairs_host(a[:0], b)
    assert row.shape == (0,) and row.dtype == np.int64 and match.dtype == np.int32 and offsets.tolist() == [0]


def test_duplicates_of_a_chain():
    """Rows A ~ B ~ C with A and C not similar, a far row D and a second copy of D: B, C and the copy are dropped, and `first` names the
    smallest earlier partner -- C's is B, not A."""
    from bioseq_amd import sketch
    S = 20
    A = np.arange(100, 100 + S)
    B = A.copy()
    B[:4] = np.arange(200, 204)  # A ~ B: 16 of 20
    C = B.copy()
    C[4:8] = np.arange(300, 304)  # B ~ C: 16 of 20; A ~ C: 12 of 20
    D = np.arange(400, 400 + S)
    empty = np.full(S, -1)
    a = np.stack([A, D, B, empty, C, D, empty]).astype(np.int32)
    row, col, match, either, _ = sketch.sketch_pairs_host(a, min_jaccard=0.75)
    assert list(zip(row.tolist(), col.tolist(), match.tolist(), either.tolist())) == [(0, 2, 16, 20), (1, 5, 20, 20), (2, 4, 16, 20)]
    for matrix in (a, a.astype(np.int64)):
        keep, first = sketch.sketch_duplicates(matrix, min_jaccard=0.75)
        assert first.dtype == np.int64 and keep.dtype == np.bool_
        assert first.tolist() == [0, 1, 0, 3, 2, 1, 6] and keep.tolist() == [True, True, False, True, False, False, True]
        exp = twin.duplicates(7, row, col)
        assert np.array_equal(keep, exp[0]) and np.array_equal(first, exp[1])
    keep, first = sketch.sketch_duplicates(a, min_jaccard=0.55)  # now A ~ C is listed too: C's first partner is A
    assert first.tolist() == [0, 1, 0, 3, 0, 1, 6]
    keep, first = sketch.sketch_duplicates(a, min_jaccard=0.75, max_pairs=3)
    assert first.tolist() == [0, 1, 0, 3, 2, 1, 6]
    with pytest.raises(ValueError):
        sketch.sketch_duplicates(a, min_jaccard=0.75, max_pairs=2)  # a cut list is no answer
    keep, first = sketch.sketch_duplicates(a, min_jaccard=0.75, min_match=0)  # the two EMPTY rows pair at min_match = 0
    assert first.tolist() == [0, 1, 0, 3, 2, 1, 3]
