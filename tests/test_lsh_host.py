"""CPU: the LSH candidates of a sketch matrix (include/bsq.h, "LSH candidates of a sketch matrix") -- the declared symbols and the Python
surface, the header's known answers, the library's host twins (bsq_lsh_keys_host, bsq_sketch_compare_list_host, bsq_lsh_pairs_host)
against the plain-Python twin (tests/lsh_twin.py) bit for bit, the properties the header states, every refusal, and the recall
formulas at hand-checked values.  No device is needed."""
import ctypes

import numpy as np
import pytest

import lsh_twin as twin

I64 = np.int64
E = -1


def _lib():
    from bioseq_amd import capi
    return capi, capi.load()


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None and w is None) or (g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes())


def _check_pairs(a, b=None, **kw):
    """host twin == Python twin, bit for bit.  Returns the host twin's result."""
    from bioseq_amd import sketch
    got = sketch.lsh_pairs(a, b, **kw)
    _same(got, twin.lsh_pairs(a, b, **kw))
    cand_kw = {k: v for k, v in kw.items() if k in ("rows_per_band", "max_bucket", "seed")}
    row, col = sketch.lsh_candidates(a, b, **cand_kw)
    assert row.dtype == I64 and col.dtype == I64
    assert list(zip(row.tolist(), col.tolist())) == twin.candidates(a, b, **cand_kw)[0]
    return got


def test_new_symbols_are_declared_and_exported():
    import bioseq_amd
    capi, L = _lib()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_lsh_keys_device", "bsq_lsh_keys_host", "bsq_lsh_count_device", "bsq_lsh_emit_device", "bsq_sketch_compare_list_device",
              "bsq_sketch_compare_list_host", "bsq_lsh_pairs_host", "bsq_lsh_kernel_name"):
        assert n in names and hasattr(L, n), n
    assert L.bsq_abi_version() == 7
    for n in ("lsh_pairs", "lsh_candidates", "lsh_keys", "lsh_keys_host", "sketch_compare_list", "sketch_compare_list_host", "lsh_recall",
              "lsh_rows_per_band", "lsh_kernel_name"):
        assert n in bioseq_amd.sketch.__all__ and callable(getattr(bioseq_amd.sketch, n))
    assert ctypes.sizeof(capi.Lsh) == 24 and capi.Lsh.seed.offset == 8 and capi.Lsh.reserved.offset == 16


def test_kernel_names():
    from bioseq_amd import sketch
    head = "k_lsh_keys+k_lsh_count+k_lsh_emit;"
    assert sketch.lsh_kernel_name(128) == head + "k_sketch_compare_list<16>"        # 512-byte rows
    assert sketch.lsh_kernel_name(32) == head + "k_sketch_compare_list<4>"          # 128 bytes
    assert sketch.lsh_kernel_name(36) == head + "k_sketch_compare_list<16>"
    assert sketch.lsh_kernel_name(256) == head + "k_sketch_compare_list<16>"        # 1 KiB
    assert sketch.lsh_kernel_name(260) == head + "k_sketch_compare_list<64>"
    assert sketch.lsh_kernel_name(128, "q") == head + "k_sketch_compare_list<16>" and sketch.lsh_kernel_name(130, "q") == head + "k_sketch_compare_list<64>"
    assert sketch.lsh_kernel_name(3) == head + "k_sketch_compare_list<4, elements>" and sketch.lsh_kernel_name(129) == head + "k_sketch_compare_list<16, elements>"
    assert sketch.lsh_kernel_name(3, "q") == head + "k_sketch_compare_list<4, elements>"
    assert sketch.lsh_kernel_name(0) == "" and sketch.lsh_kernel_name((1 << 14) + 1) == ""


def test_header_known_answers():
    from bioseq_amd import sketch
    m = twin.header_batch()
    k1 = sketch.lsh_keys(m, 1)
    assert k1.dtype == I64 and k1.shape == (4, 6)
    assert k1.tolist() == [[5027150649341863934, 5027150649341863934, E, E, E, 5027150649341863934], [E, E, E, E, 4172740380461416370, E],
                           [4432986889740121373, 4432986889740121373, E, E, E, 2075462142187623361], [E] * 6]
    assert sketch.lsh_keys(m, 2).tolist() == [[5679660576557730032, 5679660576557730032, E, E, 1824924355021282908, 5679660576557730032],
                                              [7335292338109055888, 7335292338109055888, E, E, E, 7855000670364763218]]
    assert sketch.lsh_keys(m, 3).tolist() == [[140436569112452715, 140436569112452715, E, E, 4637186175826648359, 8262566470542649784]]
    assert sketch.lsh_keys(m, 2, seed=1)[0].tolist() == [2738558360980352134, 2738558360980352134, E, E, 5308736278640590164, 2738558360980352134]
    for r in (1, 2):
        row, col, match, either, offs = sketch.lsh_pairs(m, rows_per_band=r)
        assert (row.tolist(), col.tolist(), match.tolist(), either.tolist(), offs.tolist()) == ([0, 0, 1], [1, 5, 5], [2, 1, 1], [2, 2, 2], [0, 2, 3, 3, 3, 3, 3])
    row, col, match, either, offs = sketch.lsh_pairs(m, rows_per_band=1, max_bucket=2)
    assert (row.tolist(), col.tolist(), offs.tolist()) == ([0, 0], [1, 5], [0, 2, 2, 2, 2, 2, 2])
    assert [x.tolist() for x in sketch.lsh_candidates(m, rows_per_band=4)] == [[0], [1]]
    assert sketch.lsh_pairs(m, rows_per_band=4)[4].tolist() == [0, 1, 1, 1, 1, 1, 1]
    row, col, match, either, offs = sketch.lsh_pairs(m[:2], m[2:], rows_per_band=1)
    assert (row.tolist(), col.tolist(), match.tolist(), either.tolist(), offs.tolist()) == ([0, 1], [3, 3], [1, 1], [2, 2], [0, 1, 2])
    # the candidates before the union, through the C ABI: 4, and 3 under the centre rule
    capi, L = _lib()
    for mb, want in ((32, 4), (2, 3)):
        total, offs = ctypes.c_int64(-1), np.zeros(7, I64)
        rule = capi.Lsh(1, mb, 0, 0)
        capi.check(L.bsq_lsh_pairs_host(m.ctypes.data, 6, None, 0, 4, capi.I32, ctypes.byref(rule), None, -1, ctypes.byref(total), offs.ctypes.data,
                                        0, None, None, None, None))
        assert total.value == want


@pytest.mark.parametrize("S,r", [(128, 1), (128, 4), (128, 5), (128, 128), (3, 2), (1, 1), (33, 33)])
def test_keys_equal_the_python_twin_in_both_element_types(S, r):
    from bioseq_amd import sketch
    for N in (0, 1, 37):
        v = twin.random_sketches(S + N, N, S, np.uint64, fill=0.6)
        if N:
            v[0] = twin.MASK  # EMPTY throughout
        want = twin.keys(v, r, seed=3)
        for dt in (np.int32, np.int64, np.uint64):
            got = sketch.lsh_keys(twin.as_dtype(np.where(v == twin.MASK, twin.EMPTY, v), dt), r, seed=3)
            assert got.dtype == I64 and got.shape == (S // r, N) and got.tobytes() == want.tobytes(), (S, r, N, dt)
        assert (want >= -1).all() and (N == 0 or (want[:, 0] == -1).all())


def test_void_bands_partly_empty_bands_and_the_ignored_tail():
    from bioseq_amd import sketch
    a = twin.as_dtype([[1, 2, 3, 4, 5], [1, 2, 3, 4, 6], [twin.EMPTY, twin.EMPTY, 3, twin.EMPTY, 5], [twin.EMPTY] * 4 + [5]], np.int32)
    k = sketch.lsh_keys(a, 2)  # bands (0, 1) and (2, 3); bucket 4 is the tail
    assert k.shape == (2, 4) and k.tobytes() == twin.keys(a, 2).tobytes()
    assert k[0, 0] == k[0, 1] and k[1, 0] == k[1, 1]      # rows 0 and 1 differ in the tail only
    assert k[0, 2] == -1 and k[1, 2] not in (-1, k[1, 0])  # void; partly EMPTY: an ordinary key
    assert (k[:, 3] == -1).all()                           # filled in the tail only: void in every band
    row, col = sketch.lsh_candidates(a, rows_per_band=2)
    assert (row.tolist(), col.tolist()) == ([0], [1])
    # EMPTY is a value like any other: two rows that agree on a partly EMPTY band collide
    b = twin.as_dtype([[twin.EMPTY, 7], [twin.EMPTY, 7], [twin.EMPTY, twin.EMPTY], [twin.EMPTY, twin.EMPTY]], np.int64)
    assert [x.tolist() for x in sketch.lsh_candidates(b, rows_per_band=2)] == [[0], [1]]
    assert sketch.lsh_pairs(b, rows_per_band=2, min_match=0, min_jaccard=0.0)[0].tolist() == [0]  # rows 2 and 3: void, never candidates


@pytest.mark.parametrize("n", [2, 3, 4, 5])
def test_runs_around_max_bucket(n):
    """n identical rows among others at max_bucket = 4: all pairs up to 4 rows, the centre's pairs for 5"""
    from bioseq_amd import sketch
    group = [11, 3, 17, 8, 14][:n]
    a = twin.random_sketches(n, 20, 8, groups=[group])
    got = _check_pairs(a, rows_per_band=2, max_bucket=4)
    g = sorted(group)
    want = [(g[0], j) for j in g[1:]] if n > 4 else [(g[x], g[y]) for x in range(n) for y in range(x + 1, n)]
    assert list(zip(got[0].tolist(), got[1].tolist())) == sorted(want)
    assert (got[2] == 8).all() and (got[3] == 8).all()
    row, col = sketch.lsh_candidates(a, rows_per_band=2, max_bucket=4, max_candidates=4 * len(want))
    assert len(row) == len(want)


@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.uint64])
def test_pairs_equal_the_python_twin_and_are_a_subset_of_sketch_pairs(dtype):
    from bioseq_amd import sketch
    a = twin.near_duplicates(5, 120, 32, dtype, share=0.3, keep=0.8, fill=0.7)
    for kw in ({"rows_per_band": 2}, {"rows_per_band": 1, "max_bucket": 2}, {"rows_per_band": 3, "min_jaccard": 0.8, "min_match": 3, "seed": 9},
               {"rows_per_band": 5, "min_jaccard": 0.0, "min_match": 0}, {"rows_per_band": 32}):
        got = _check_pairs(a, **kw)
        assert got[4].shape == (121,) and got[4][-1] == got[0].size and (np.diff(got[4]) >= 0).all()
        assert (np.bincount(got[0], minlength=120) == np.diff(got[4])).all()
        full = sketch.sketch_pairs_host(a, min_jaccard=kw.get("min_jaccard", 0.5), min_match=kw.get("min_match", 1))
        index = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(full[0], full[1]))}
        at = [index[(int(i), int(j))] for i, j in zip(got[0], got[1])]  # (KeyError: a listed pair that sketch_pairs does not list)
        assert at == sorted(at) and (full[2][at] == got[2]).all() and (full[3][at] == got[3]).all()
        if kw.get("max_bucket", 32) > 2:  # no run is cut: exactly the colliding pairs of the full list
            cand = set(twin.candidates(a, rows_per_band=kw["rows_per_band"], seed=kw.get("seed", 0))[0])
            assert [k for k, p in enumerate(zip(full[0].tolist(), full[1].tolist())) if p in cand] == at
        assert sketch.lsh_pairs(a, either=False, **kw)[3] is None


def test_two_matrices_are_the_concatenation_rule():
    from bioseq_amd import sketch
    whole = twin.near_duplicates(6, 90, 16, share=0.4, keep=0.7)
    a, b = whole[:35], whole[35:]
    for kw in ({"rows_per_band": 2, "min_jaccard": 0.3}, {"rows_per_band": 1, "max_bucket": 2, "min_jaccard": 0.2}):
        got = _check_pairs(a, b, **kw)
        one = sketch.lsh_pairs(whole, **kw) if kw.get("max_bucket", 32) > 2 else None
        if one is not None:  # the cross block of the one-matrix list
            cross = (one[0] < 35) & (one[1] >= 35)
            assert got[0].tolist() == one[0][cross].tolist() and got[1].tolist() == (one[1][cross] - 35).tolist()
        assert got[4].shape == (36,)
    for x, y in ((whole[:0], None), (whole[:0], whole), (whole, whole[:0]), (whole[:1], None)):
        got = sketch.lsh_pairs(x, y, rows_per_band=2)
        assert got[0].size == 0 and got[4].tolist() == [0] * (x.shape[0] + 1)
        assert sketch.lsh_keys(x, 2).shape == (8, x.shape[0])


def test_list_compare_equals_the_python_twin_and_the_dense_entries():
    from bioseq_amd import sketch
    for S in (1, 3, 16, 129):
        for dt in (np.int32, np.int64):
            a = twin.near_duplicates(S, 12, S, dt, share=0.5, fill=0.7)
            b = twin.near_duplicates(S + 50, 7, S, dt, share=0.5, fill=0.7)
            row = np.array([0, 0, 3, 3, 11, 11, -1, 12, 5, np.iinfo(I64).min, np.iinfo(I64).max, 2], I64)
            col = np.array([0, 6, 3, 3, 6, 7, 0, 0, -1, 0, 0, np.iinfo(I64).max], I64)
            for other in (b, None):
                m, e = sketch.sketch_compare_list(a, row, col, other)
                tm, te = twin.compare_list(a, row, col, other)
                assert m.dtype == np.int32 and m.tobytes() == tm.tobytes() and e.tobytes() == te.tobytes()
                dm, de = sketch.sketch_compare_host(a, other)
                hi = (a if other is None else other).shape[0]
                ok = (row >= 0) & (row < 12) & (col >= 0) & (col < hi)
                assert (m[~ok] == -1).all() and (e[~ok] == -1).all() and ok.sum() >= 5
                assert (m[ok] == dm[row[ok], col[ok]]).all() and (e[ok] == de[row[ok], col[ok]]).all()
                assert sketch.sketch_compare_list(a, row, col, other, either=False)[1] is None
            m, e = sketch.sketch_compare_list(a, np.zeros(0, I64), np.zeros(0, I64))
            assert m.shape == (0,) and e.shape == (0,)


def test_max_candidates_raises_before_the_list_exists():
    from bioseq_amd import sketch
    a = twin.random_sketches(3, 40, 8, groups=[list(range(10, 30))])  # 20 identical rows: 190 pairs in each of 4 bands
    total = twin.candidates(a, rows_per_band=2)[1]
    assert total == 4 * 190
    for call in (sketch.lsh_pairs, sketch.lsh_candidates):
        with pytest.raises(ValueError, match=r"760 candidates.*max_candidates = 759.*max_bucket.*rows_per_band"):
            call(a, rows_per_band=2, max_candidates=759)
        assert len(call(a, rows_per_band=2, max_candidates=760)[0]) == 190
        assert len(call(a, rows_per_band=2, max_bucket=19, max_candidates=4 * 19)[0]) == 19  # the centre rule is the way out
        assert len(call(a, rows_per_band=2, max_candidates=None)[0]) == 190


def test_every_argument_rule_raises():
    from bioseq_amd import sketch
    a = twin.random_sketches(1, 6, 8)
    for kw in ({"rows_per_band": 0}, {"rows_per_band": 9}, {"rows_per_band": 2.5}, {"rows_per_band": True}, {"rows_per_band": 2, "max_bucket": 1},
               {"rows_per_band": 2, "max_bucket": 2 ** 31}, {"rows_per_band": 2, "max_bucket": 2.5}, {"rows_per_band": 2, "max_candidates": -1},
               {"rows_per_band": 2, "max_candidates": 1.5}):
        for call in (sketch.lsh_pairs, sketch.lsh_candidates):
            with pytest.raises(ValueError):
                call(a, **kw)
    for kw in ({"min_jaccard": 1.5}, {"min_jaccard": float("nan")}, {"min_match": -1}, {"min_match": 9}, {"min_match": 1.5}):
        with pytest.raises(ValueError):
            sketch.lsh_pairs(a, rows_per_band=2, **kw)
    with pytest.raises(TypeError):
        sketch.lsh_pairs(a)  # rows_per_band has no default
    for bad in (a.astype(np.int16), a.astype(np.float32), a[0], a.reshape(2, 3, 8)):
        with pytest.raises(ValueError):
            sketch.lsh_pairs(bad, rows_per_band=1)
        with pytest.raises(ValueError):
            sketch.lsh_keys(bad, 1)
        with pytest.raises(ValueError):
            sketch.sketch_compare_list(bad, np.zeros(1, I64), np.zeros(1, I64))
    for b in (a[:, :4], a.astype(np.int64)):  # another width, another element type
        with pytest.raises(ValueError):
            sketch.lsh_pairs(a, b, rows_per_band=2)
        with pytest.raises(ValueError):
            sketch.sketch_compare_list(a, np.zeros(1, I64), np.zeros(1, I64), b)
    with pytest.raises(ValueError):
        sketch.lsh_pairs([[1, 2]], rows_per_band=1)  # neither a numpy matrix nor a tensor
    for r in (0, 9, 1.5):
        with pytest.raises(ValueError):
            sketch.lsh_keys(a, r)
    for row, col in ((np.zeros(2, I64), np.zeros(3, I64)), (np.zeros(2, np.int32), np.zeros(2, np.int32)), (np.zeros((2, 1), I64), np.zeros((2, 1), I64))):
        with pytest.raises(ValueError):
            sketch.sketch_compare_list(a, row, col)
    # tensors that are not on a device are refused without touching one
    import torch
    t = torch.from_numpy(a.copy())
    for call in (lambda: sketch.lsh_pairs(t, rows_per_band=2), lambda: sketch.lsh_keys(t, 2), lambda: sketch.lsh_candidates(t, rows_per_band=2),
                 lambda: sketch.sketch_compare_list(t, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))):
        with pytest.raises(ValueError, match="device"):
            call()


def test_the_c_abi_refuses_what_the_header_says():
    capi, L = _lib()
    a = twin.random_sketches(1, 6, 8)
    keys, offs, total = np.full((4, 6), -77, I64), np.full(7, -77, I64), ctypes.c_int64(-77)
    good = capi.Lsh(2, 32, 0, 0)
    for rule in (capi.Lsh(0, 32, 0, 0), capi.Lsh(9, 32, 0, 0), capi.Lsh(2, 1, 0, 0), capi.Lsh(2, 32, 0, 1)):
        assert L.bsq_lsh_keys_host(a.ctypes.data, 6, 8, capi.I32, ctypes.byref(rule), keys.ctypes.data, 6) == capi.ERR_INVALID_ARG
        assert L.bsq_lsh_pairs_host(a.ctypes.data, 6, None, 0, 8, capi.I32, ctypes.byref(rule), None, -1, ctypes.byref(total), offs.ctypes.data, 0,
                                    None, None, None, None) == capi.ERR_INVALID_ARG
        assert L.bsq_last_error()
    for args in ((a.ctypes.data, -1, 8, capi.I32, ctypes.byref(good), keys.ctypes.data, 6), (a.ctypes.data, 6, 0, capi.I32, ctypes.byref(good), keys.ctypes.data, 6),
                 (a.ctypes.data, 6, (1 << 14) + 1, capi.I32, ctypes.byref(good), keys.ctypes.data, 6), (a.ctypes.data, 6, 8, capi.I32, None, keys.ctypes.data, 6),
                 (None, 6, 8, capi.I32, ctypes.byref(good), keys.ctypes.data, 6), (a.ctypes.data, 6, 8, capi.I32, ctypes.byref(good), None, 6),
                 (a.ctypes.data, 6, 8, capi.I32, ctypes.byref(good), keys.ctypes.data, 5), (a.ctypes.data, 1 << 31, 8, capi.I32, ctypes.byref(good), keys.ctypes.data, 1 << 31)):
        assert L.bsq_lsh_keys_host(*args) == capi.ERR_INVALID_ARG, args[1:4]
    assert L.bsq_lsh_keys_host(a.ctypes.data, 6, 8, capi.I8, ctypes.byref(good), keys.ctypes.data, 6) == capi.ERR_DTYPE
    assert (keys == -77).all()  # a refusal writes nothing
    assert L.bsq_lsh_keys_host(None, 0, 8, capi.I32, ctypes.byref(good), None, 0) == capi.OK
    row, m = np.zeros(2, I64), np.full(2, -77, np.int32)
    for args in ((a.ctypes.data, -1, a.ctypes.data, 6, 8, capi.I32, row.ctypes.data, row.ctypes.data, 2, m.ctypes.data, None),
                 (a.ctypes.data, 6, a.ctypes.data, 6, 0, capi.I32, row.ctypes.data, row.ctypes.data, 2, m.ctypes.data, None),
                 (a.ctypes.data, 6, a.ctypes.data, 6, 8, capi.I32, None, row.ctypes.data, 2, m.ctypes.data, None),
                 (a.ctypes.data, 6, a.ctypes.data, 6, 8, capi.I32, row.ctypes.data, row.ctypes.data, 2, None, None),
                 (a.ctypes.data, 6, a.ctypes.data, 6, 8, capi.I32, row.ctypes.data, row.ctypes.data, -1, m.ctypes.data, None),
                 (None, 6, a.ctypes.data, 6, 8, capi.I32, row.ctypes.data, row.ctypes.data, 2, m.ctypes.data, None),
                 (a.ctypes.data, 1 << 31, a.ctypes.data, 6, 8, capi.I32, row.ctypes.data, row.ctypes.data, 2, m.ctypes.data, None)):
        assert L.bsq_sketch_compare_list_host(*args) == capi.ERR_INVALID_ARG
    assert L.bsq_sketch_compare_list_host(a.ctypes.data, 6, a.ctypes.data, 6, 8, capi.F32, row.ctypes.data, row.ctypes.data, 2, m.ctypes.data, None) == capi.ERR_DTYPE
    assert (m == -77).all()
    # no rows at all: every index is outside
    assert L.bsq_sketch_compare_list_host(None, 0, None, 0, 8, capi.I32, row.ctypes.data, row.ctypes.data, 2, m.ctypes.data, None) == capi.OK and (m == -1).all()
    bad_rule = [capi.SketchPairs(-1, 0, 0, 0), capi.SketchPairs(9, 0, 0, 0), capi.SketchPairs(1, 65537, 0, 0), capi.SketchPairs(1, 0, 1, 0), capi.SketchPairs(1, 0, 0, 1)]
    for pr in bad_rule:
        assert L.bsq_lsh_pairs_host(a.ctypes.data, 6, None, 0, 8, capi.I32, ctypes.byref(good), ctypes.byref(pr), -1, ctypes.byref(total), offs.ctypes.data,
                                    0, None, None, None, None) == capi.ERR_INVALID_ARG
    ok_rule = capi.SketchPairs(1, 32768, 0, 0)
    for args in ((a.ctypes.data, -1, None, 0), (a.ctypes.data, 6, None, 3), (None, 6, None, 0), (a.ctypes.data, 1 << 30, a.ctypes.data, 1 << 30)):
        assert L.bsq_lsh_pairs_host(*args, 8, capi.I32, ctypes.byref(good), ctypes.byref(ok_rule), -1, ctypes.byref(total), offs.ctypes.data, 0, None, None,
                                    None, None) == capi.ERR_INVALID_ARG
    assert L.bsq_lsh_pairs_host(a.ctypes.data, 6, None, 0, 8, capi.I32, ctypes.byref(good), ctypes.byref(ok_rule), -1, None, offs.ctypes.data, 0, None, None,
                                None, None) == capi.ERR_INVALID_ARG
    assert L.bsq_lsh_pairs_host(a.ctypes.data, 6, None, 0, 8, capi.I32, ctypes.byref(good), ctypes.byref(ok_rule), -1, ctypes.byref(total), offs.ctypes.data, 3,
                                None, None, None, None) == capi.ERR_INVALID_ARG
    assert (offs == -77).all() and total.value == -77
    assert L.bsq_lsh_kernel_name(8, capi.F32) == b"" and L.bsq_lsh_kernel_name(8, capi.I32) != b""
    # the device entry points refuse the same arguments before they touch a device
    for rule in (capi.Lsh(0, 32, 0, 0), capi.Lsh(2, 1, 0, 0)):
        assert L.bsq_lsh_keys_device(a.ctypes.data, 6, 8, capi.I32, ctypes.byref(rule), keys.ctypes.data, 6, None) == capi.ERR_INVALID_ARG
    assert L.bsq_lsh_count_device(keys.ctypes.data, 4, 6, ctypes.byref(capi.Lsh(2, 1, 0, 0)), keys.ctypes.data, None) == capi.ERR_INVALID_ARG
    assert L.bsq_lsh_count_device(keys.ctypes.data, -1, 6, ctypes.byref(good), keys.ctypes.data, None) == capi.ERR_INVALID_ARG
    assert L.bsq_lsh_count_device(None, 4, 6, ctypes.byref(good), keys.ctypes.data, None) == capi.ERR_INVALID_ARG
    assert L.bsq_lsh_count_device(keys.ctypes.data, 4, 6, ctypes.byref(good), None, None) == capi.ERR_INVALID_ARG
    assert L.bsq_lsh_emit_device(keys.ctypes.data, keys.ctypes.data, 4, 6, ctypes.byref(good), keys.ctypes.data, -1, keys.ctypes.data, None) == capi.ERR_INVALID_ARG
    assert L.bsq_lsh_emit_device(keys.ctypes.data, None, 4, 6, ctypes.byref(good), keys.ctypes.data, 5, keys.ctypes.data, None) == capi.ERR_INVALID_ARG
    assert L.bsq_sketch_compare_list_device(a.ctypes.data, 6, a.ctypes.data, 6, 0, capi.I32, row.ctypes.data, row.ctypes.data, 2, m.ctypes.data, None, None) == capi.ERR_INVALID_ARG
    assert L.bsq_lsh_count_device(keys.ctypes.data, 0, 6, ctypes.byref(good), keys.ctypes.data, None) == capi.OK  # no band: nothing launched


def test_recall_formulas_at_hand_checked_values():
    from bioseq_amd import sketch
    assert sketch.lsh_recall(0.5, 1, 1) == 0.5
    assert sketch.lsh_recall(0.5, 2, 2) == 1 - 0.75 ** 2 == 0.4375
    assert sketch.lsh_recall(1.0, 7, 3) == 1.0 and sketch.lsh_recall(0.0, 7, 3) == 0.0 and sketch.lsh_recall(0.3, 2, 0) == 0.0
    assert abs(sketch.lsh_recall(0.5, 3, 42) - (1 - 0.875 ** 42)) < 1e-15 and 0.9963 < sketch.lsh_recall(0.5, 3, 42) < 0.9964
    assert 0.873 < sketch.lsh_recall(0.5, 4, 32) < 0.874
    # S = 128 at 0.5: r = 3 (42 bands) reaches 0.95, r = 4 (32 bands) does not
    assert sketch.lsh_rows_per_band(128, 0.5) == 3
    assert sketch.lsh_rows_per_band(128, 0.5, recall=0.85) == 4
    # S = 4 at 0.5: r = 1 gives 1 - 0.5^4 = 0.9375, r = 2 gives 1 - 0.75^2 = 0.4375
    assert sketch.lsh_rows_per_band(4, 0.5, recall=0.9) == 1 and sketch.lsh_rows_per_band(4, 0.5, recall=0.4) == 2
    assert sketch.lsh_rows_per_band(4, 0.5, recall=0.99) == 1  # nothing reaches it: the most sensitive banding
    assert sketch.lsh_rows_per_band(128, 1.0) == 128 and sketch.lsh_rows_per_band(1024, 0.9) >= sketch.lsh_rows_per_band(1024, 0.5)
    for bad in ((1.5, 1, 1), (-0.1, 1, 1), (0.5, 0, 1), (0.5, 1, -1)):
        with pytest.raises(ValueError):
            sketch.lsh_recall(*bad)
    with pytest.raises(ValueError):
        sketch.lsh_rows_per_band(0, 0.5)
    with pytest.raises(ValueError):
        sketch.lsh_rows_per_band(128, 0.5, recall=1.5)
