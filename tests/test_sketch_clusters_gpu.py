"""GPU: the single-linkage clusters of a sketch matrix (bioseq_amd.sketch.sketch_clusters / cluster_pairs, bsq_sketch_clusters_device /
bsq_cluster_pairs_device) against the numpy twin (tests/sketch_clusters_twin.py) and the library's host twin, byte for byte: partial
strips and tiles, the widest sketch, every split of a strip's tiles into runs, a path whose unions arrive in scrambled order from
different workgroups, groups of identical rows that hammer one root, guards around the labels, a scratch that is not cleared between
calls, edge lists with padding and indices out of range, real sketches with a planted family, and the Python surface."""
import ctypes

import numpy as np
import pytest

import minhash_twin
import sketch_clusters_twin as twin
import sketch_pairs_twin as pairs_twin

pytestmark = pytest.mark.gpu

I32, U64 = 2, 3
HALF = pairs_twin.q16(0.5)
CLIQUES = (130, 65, 64, 2, 1) + (1,) * 68  # 330 rows


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _check(gpu, a, min_match, T, segments=(None,), compared=None):
    """sketch_clusters on the device == the numpy twin == the host twin for every segment count.  Returns the twin's labels."""
    import torch
    from bioseq_amd import sketch
    exp = twin.labels(a, min_match, T, compared)
    assert sketch.sketch_clusters_host(a, min_jaccard=T / 65536, min_match=min_match).tobytes() == exp.tobytes(), "host twin"
    da = _dev(a, gpu)
    for seg in segments:
        got = sketch.sketch_clusters(da, min_jaccard=T / 65536, min_match=min_match, segments=seg)
        assert got.dtype == torch.int64 and got.device == da.device and got.is_contiguous() and tuple(got.shape) == exp.shape
        assert got.cpu().numpy().tobytes() == exp.tobytes(), ("segments", seg)
    return exp


@pytest.mark.parametrize("B, S", [(1, 1), (3, 7), (65, 100), (33, 16384)])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_clusters_equal_the_twins(gpu, bsq, B, S, dtype):
    """Partial strips and tiles, a diagonal tile in every strip; S = 16384: the widest sketch."""
    a, _ = pairs_twin.case(B * 1000 + S, B, B, S, dtype, upper=True)
    compared = minhash_twin.compare(a, a)
    for name, min_match, T in pairs_twin.thresholds(S):
        exp = _check(gpu, a, min_match, T, compared=compared)
        if name == "all":
            assert not exp.any()
        elif name == "none":
            assert (exp == np.arange(B)).all()


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_every_split_into_segments_gives_one_result(gpu, bsq, dtype):
    """200 rows x 64: four strips, so links cross strips and runs; "all" makes every tile full of hits, the middle threshold leaves
    clusters of several sizes."""
    a, _ = pairs_twin.case(200 * 1000 + 64, 200, 200, 64, dtype, upper=True)
    compared = minhash_twin.compare(a, a)
    for name, min_match, T in pairs_twin.thresholds(64):
        exp = _check(gpu, a, min_match, T, segments=(None, 1, 2, 4), compared=compared)
        if name == "mid":
            assert 1 < len(set(exp.tolist())) < 200


@pytest.mark.parametrize("B, S", [(330, 64), (200, 8)])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_chains_whole_and_cut(gpu, bsq, B, S, dtype):
    """One path of B - 1 links laid through the rows by a permutation: neighbours sit in different strips and tiles, so the unions of
    one component arrive from different workgroups in no order; cut, it falls into pieces and singletons."""
    whole = twin.chain(B, S, B + S, dtype)
    assert not _check(gpu, whole, 1, HALF, segments=(None, 1, 3)).any()
    assert (_check(gpu, whole, 1, HALF + 1) == np.arange(B)).all()
    exp = _check(gpu, twin.chain(B, S, B + S, dtype, cut=True), 1, HALF, segments=(None, 1, 3))
    sizes = twin.table(exp)[1]
    assert (len(sizes), int((sizes == 1).sum())) == {200: (8, 4), 330: (13, 6)}[B]


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_cliques_hammer_one_root(gpu, bsq, dtype):
    """Groups of 130, 65, 64, 2 and 1 identical rows scattered over six strips: every pair of a group passes, so whole tiles of hits from
    several workgroups end under one root -- the cached roots, the tile's own union-find and the retry after a lost swap."""
    exp = _check(gpu, twin.cliques(330, 64, CLIQUES, 11, dtype), 1, 65536, segments=(None, 1, 2, 6))
    assert sorted(twin.table(exp)[1].tolist()) == sorted(CLIQUES)


def test_guards_and_a_scratch_that_is_not_cleared(gpu, bsq):
    """The raw entry points on a side stream: labels between guard words that stay intact; a second call with another threshold into
    the same scratch, left as the first call left it and then filled with junk, gives that threshold's labels."""
    import torch
    from bioseq_amd import capi
    L = capi.load()
    a = twin.cliques(330, 64, CLIQUES, 11)
    da = _dev(a, gpu)
    guard = 16
    scratch = torch.full((330 + 2 * guard,), 0x5A5A5A5A, dtype=torch.int64, device=gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    stream = ctypes.c_void_p(side.cuda_stream)
    for min_match, T in ((1, 65536), (0, 0), (1, 65536)):
        exp = twin.labels(a, min_match, T)
        for junk in (False, True):
            if junk:
                scratch.fill_(-3)  # (on the current stream: order it before the side stream's call)
                side.wait_stream(torch.cuda.current_stream())
            labels = torch.full((330 + 2 * guard,), 0x5A5A5A5A, dtype=torch.int64, device=gpu)
            side.wait_stream(torch.cuda.current_stream())
            rule = capi.SketchPairs(min_match, T, 1, 2)
            capi.check(L.bsq_sketch_clusters_device(da.data_ptr(), 330, 64, I32, ctypes.byref(rule), scratch.data_ptr() + 8 * guard,
                                                    labels.data_ptr() + 8 * guard, stream))
            side.synchronize()
            raw = labels.cpu().numpy()
            assert (raw[:guard] == 0x5A5A5A5A).all() and (raw[-guard:] == 0x5A5A5A5A).all() and np.array_equal(raw[guard:-guard], exp)
            raw = scratch.cpu().numpy()
            assert (raw[:guard] == (-3 if junk else 0x5A5A5A5A)).all() and (raw[-guard:] == raw[0]).all()
            assert (raw[guard:-guard] <= np.arange(330)).all()  # the invariant of the parent array
        scratch.fill_(0x5A5A5A5A)
        side.wait_stream(torch.cuda.current_stream())


def test_cluster_pairs_equals_sketch_clusters(gpu, bsq):
    """The labels of the pair list are the labels of the matrix; a list cut with max_pairs above the total has zeros behind it; entries
    out of range and self-edges are ignored unread; numpy arrays and device tensors agree."""
    import torch
    from bioseq_amd import sketch
    for a, min_jaccard in ((twin.chain(330, 64, 5, np.int32, cut=True), 0.5), (twin.cliques(330, 64, CLIQUES, 11), 1.0),
                           (pairs_twin.case(200064, 200, 200, 64, np.int64, upper=True)[0], 0.14)):
        da = _dev(a, gpu)
        want = sketch.sketch_clusters(da, min_jaccard=min_jaccard)
        assert want.cpu().numpy().tobytes() == twin.labels(a, 1, pairs_twin.q16(min_jaccard)).tobytes()
        row, col = sketch.sketch_pairs(da, min_jaccard=min_jaccard, either=False)[:2]
        assert row.numel() > 0 and torch.equal(sketch.cluster_pairs(row, col, len(a)), want)
        cut = sketch.sketch_pairs(da, min_jaccard=min_jaccard, either=False, max_pairs=row.numel() + 100)
        assert int(cut[4][-1]) == row.numel() and not bool(cut[0][row.numel():].any())
        assert torch.equal(sketch.cluster_pairs(cut[0], cut[1], len(a)), want)
        junk_r = torch.tensor([5, -1, 3, len(a), 2 ** 62, 0, -2 ** 63], dtype=torch.int64, device=gpu)
        junk_c = torch.tensor([5, 3, -1, 0, 1, len(a), 1], dtype=torch.int64, device=gpu)
        mixed = sketch.cluster_pairs(torch.cat([junk_r, col, junk_c]), torch.cat([junk_c, row, junk_r]), len(a))
        assert torch.equal(mixed, want)
        assert np.array_equal(sketch.cluster_pairs(row.cpu().numpy(), col.cpu().numpy(), len(a)), want.cpu().numpy())
    ident = sketch.cluster_pairs(junk_r, junk_c, 6)
    assert ident.tolist() == [0, 1, 2, 3, 4, 5]
    assert sketch.cluster_pairs(row[:0], col[:0], 3).tolist() == [0, 1, 2] and sketch.cluster_pairs(row[:0], col[:0], 0).shape == (0,)


def test_real_sketches_with_a_planted_family(gpu, bsq):
    """40 random DNA rows (row 0 empty, row 1 shorter than k) and a family: rows 40 .. 43 are row 2 with 10, 20, 30 and 40 cumulative
    substitutions; k = 21, S = 512, canonical.  At 0.75 the neighbours are linked (0.80 .. 0.85) and the ends are not (row 2 and row 43:
    0.55), yet the family and row 2 are one cluster -- single linkage -- and nothing else is with it; the split keeps them together."""
    import torch
    from bioseq_amd import sketch
    rng = np.random.default_rng(29)
    lens = rng.integers(200, 3000, 40)
    lens[:3] = (0, 20, 2000)
    chars = rng.choice(np.frombuffer(b"ACGT" * 25 + b"Na*\xff", np.uint8), int(lens.sum())).astype(np.uint8)
    offs = np.zeros(41, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    member = chars[offs[2]:offs[3]].copy()
    for _ in range(4):
        member = member.copy()
        member[rng.choice(2000, 10, replace=False)] = ord("A")
        chars = np.concatenate([chars, member])
        offs = np.concatenate([offs, [offs[-1] + 2000]])
    tok = bsq.Tokenizer("DNA4", False, False, False)
    want = list(range(40)) + [2] * 4
    for dc in ("i", "q"):
        sk = sketch.minhash_packed(tok, _dev(chars, gpu), _dev(offs, gpu), 21, 512, dc, canonical=True)
        labels = sketch.sketch_clusters(sk, min_jaccard=0.75)
        assert labels.tolist() == want
        pairs = sketch.sketch_pairs(sk, min_jaccard=0.75)
        assert (2, 40) in zip(pairs[0].tolist(), pairs[1].tolist()) and (2, 43) not in zip(pairs[0].tolist(), pairs[1].tolist())
        assert np.array_equal(sketch.sketch_clusters(sk.cpu().numpy(), min_jaccard=0.75), labels.cpu().numpy())
        assert sketch.sketch_clusters(sk, min_jaccard=0.0, min_match=0).tolist() == [0] * 44
        assert sketch.sketch_clusters(sk, min_jaccard=1.0, min_match=0).tolist() == [0, 0] + list(range(2, 44))  # the two EMPTY rows
        reps, sizes, dense = sketch.cluster_table(labels)
        assert reps.tolist() == list(range(40)) and sizes.tolist() == [1, 1, 5] + [1] * 37 and dense.tolist() == want
        split = sketch.cluster_split(labels, (0.5, 0.5), seed=3)
        assert split.device == labels.device and split.dtype == torch.int64
        assert np.array_equal(split.cpu().numpy(), twin.split(np.array(want), (0.5, 0.5), 3)) and len(set(split[[2, 40, 41, 42, 43]].tolist())) == 1


def test_python_surface_and_refusals(gpu, bsq):
    import torch
    from bioseq_amd import capi, sketch
    a = _dev(pairs_twin.sketch_like(np.random.default_rng(0), 70, 16, np.int32), gpu)
    assert sketch.sketch_clusters(a[:0]).shape == (0,) and sketch.sketch_clusters(a[:0]).dtype == torch.int64  # B == 0
    assert sketch.sketch_clusters_kernel_name(70) == sketch.sketch_clusters_kernel_name(262144) == "k_cluster_init+k_sketch_link+k_cluster_labels"
    assert sketch.sketch_clusters_kernel_name(0) == "" and sketch.sketch_clusters_kernel_name(70, 65) == ""
    edges = torch.zeros(4, dtype=torch.int64, device=gpu)
    for call in (lambda: sketch.sketch_clusters(a.cpu()), lambda: sketch.sketch_clusters(a.to(torch.float32)), lambda: sketch.sketch_clusters(a[0]),
                 lambda: sketch.sketch_clusters(a.t()), lambda: sketch.sketch_clusters(a, min_jaccard=1.01),
                 lambda: sketch.sketch_clusters(a, min_jaccard=float("nan")), lambda: sketch.sketch_clusters(a, min_match=17),
                 lambda: sketch.sketch_clusters(a, segments=65), lambda: sketch.cluster_pairs(edges, edges[:3], 6),
                 lambda: sketch.cluster_pairs(edges[::2], edges[:2], 6),  # a row that is not contiguous
                 lambda: sketch.cluster_pairs(edges.to(torch.int32), edges.to(torch.int32), 6), lambda: sketch.cluster_pairs(edges, edges.cpu(), 6),
                 lambda: sketch.cluster_pairs(edges, edges, -1), lambda: sketch.cluster_pairs(edges, edges, 2 ** 31)):
        with pytest.raises(ValueError):
            call()
    # the raw entry points refuse before anything is written: upper == 0, a bad threshold, a bad type, labels == scratch, B == 0 writes nothing
    L = capi.load()
    scratch = torch.full((70,), 0x5A, dtype=torch.int64, device=gpu)
    out = torch.full((70,), 0x5A, dtype=torch.int64, device=gpu)
    for rule, code, labels in ((capi.SketchPairs(1, 0, 0, 0), I32, out), (capi.SketchPairs(1, 65537, 1, 0), I32, out), (capi.SketchPairs(17, 0, 1, 0), I32, out),
                               (capi.SketchPairs(1, 0, 1, 65), I32, out), (capi.SketchPairs(1, 0, 1, 0), 4, out), (capi.SketchPairs(1, 0, 1, 0), I32, scratch)):
        st = L.bsq_sketch_clusters_device(a.data_ptr(), 70, 16, code, ctypes.byref(rule), scratch.data_ptr(), labels.data_ptr(), None)
        assert st in (capi.ERR_INVALID_ARG, capi.ERR_DTYPE)
    rule = capi.SketchPairs(1, 0, 1, 0)
    assert L.bsq_sketch_clusters_device(a.data_ptr(), 0, 16, I32, ctypes.byref(rule), scratch.data_ptr(), out.data_ptr(), None) == capi.OK
    assert L.bsq_cluster_pairs_device(edges.data_ptr(), edges.data_ptr(), 4, 70, scratch.data_ptr(), scratch.data_ptr(), None) == capi.ERR_INVALID_ARG
    assert L.bsq_cluster_pairs_device(edges.data_ptr(), edges.data_ptr(), -1, 70, scratch.data_ptr(), out.data_ptr(), None) == capi.ERR_INVALID_ARG
    assert L.bsq_cluster_pairs_device(edges.data_ptr(), edges.data_ptr(), 4, 0, scratch.data_ptr(), out.data_ptr(), None) == capi.OK
    torch.cuda.synchronize()
    assert bool((scratch == 0x5A).all()) and bool((out == 0x5A).all())
