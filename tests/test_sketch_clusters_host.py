"""CPU: the single-linkage clusters of a sketch matrix (include/bsq.h, "sketch clusters") -- the declared symbols, the header's known
answers, the library's host twins bsq_sketch_clusters_host and bsq_cluster_pairs_host against the numpy twin
(tests/sketch_clusters_twin.py) byte for byte on the inputs the GPU tests use, the invariants of a label array, `cluster_table` and
`cluster_split` in their numpy and torch forms, and every refusal.  No device is needed."""
import ctypes

import numpy as np
import pytest

import minhash_twin
import sketch_clusters_twin as twin
import sketch_pairs_twin as pairs_twin

I32, U64 = 2, 3
E = 4294967295
HALF = pairs_twin.q16(0.5)
CLIQUES = (130, 65, 64, 2, 1) + (1,) * 68  # 330 rows


def _lib():
    from bioseq_amd import capi
    return capi, capi.load()


def _check(a, min_match, T, compared=None):
    """host twin == numpy twin, byte for byte; the invariants; the edge-list twin on the pair list gives the same.  Returns the labels."""
    from bioseq_amd import sketch
    exp = twin.labels(a, min_match, T, compared)
    got = sketch.sketch_clusters_host(a, min_jaccard=T / 65536, min_match=min_match)
    assert got.dtype == np.int64 and got.shape == (len(a),) and got.tobytes() == exp.tobytes()
    assert (got <= np.arange(len(a))).all() and (got[got] == got).all()
    row, col = sketch.sketch_pairs_host(a, min_jaccard=T / 65536, min_match=min_match, either=False)[:2]
    assert sketch.cluster_pairs_host(row, col, len(a)).tobytes() == exp.tobytes()
    return got


def test_new_symbols_are_declared_and_exported():
    import bioseq_amd
    capi, L = _lib()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_sketch_clusters_device", "bsq_sketch_clusters_host", "bsq_cluster_pairs_device", "bsq_cluster_pairs_host",
              "bsq_sketch_clusters_kernel_name"):
        assert n in names and hasattr(L, n), n
    assert L.bsq_abi_version() == 7
    for n in ("sketch_clusters", "sketch_clusters_host", "cluster_pairs", "cluster_pairs_host", "sketch_clusters_kernel_name", "cluster_table",
              "cluster_split"):
        assert n in bioseq_amd.sketch.__all__ and callable(getattr(bioseq_amd.sketch, n))


def test_known_answers():
    """The answers of include/bsq.h on the plain sketches of the MinHash section's batch, from the numpy twin and the host twin."""
    sk = np.array([[1282424135, 2136608625, E, E], [1282424135, 2136608625, E, E], [E] * 4, [E] * 4, [E, E, 1516739009, E]], np.uint32)
    for dtype in (np.int32, np.int64):
        a = sk.view(np.int32) if dtype == np.int32 else np.where(sk == E, -1, sk.astype(np.int64))
        for min_match, T, want in ((1, 32768, [0, 0, 2, 3, 4]), (0, 65536, [0, 0, 2, 2, 4]), (0, 0, [0, 0, 0, 0, 0])):
            assert _check(a, min_match, T).tolist() == want


@pytest.mark.parametrize("B, S", [(1, 1), (3, 7), (65, 100), (200, 64)])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_host_twin_equals_numpy_twin(B, S, dtype):
    """Every threshold of the pair tests' upper cases: one cluster, a middle one with clusters of several sizes, the planted rows alone,
    singletons only."""
    a, _ = pairs_twin.case(B * 1000 + S, B, B, S, dtype, upper=True)
    compared = minhash_twin.compare(a, a)
    for name, min_match, T in pairs_twin.thresholds(S):
        got = _check(a, min_match, T, compared)
        if name == "all":
            assert not got.any()
        elif name == "equal" and B >= 3:
            assert got[B // 2] == got[B - 1] == 0 and len(set(got.tolist())) == B - 2
        elif name == "none":
            assert (got == np.arange(B)).all()
    if (B, S) == (200, 64):
        mid = _check(a, *pairs_twin.thresholds(S)[1][1:], compared)
        assert 1 < len(set(mid.tolist())) < B  # (not vacuous)


@pytest.mark.parametrize("B, S", [(200, 8), (330, 64), (5, 2)])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_chains_whole_and_cut(B, S, dtype):
    """A path of B - 1 links through scrambled rows is one cluster; at T + 1 nothing is linked; cut at every 50th position it falls into
    pieces with singletons between them."""
    a = twin.chain(B, S, B + S, dtype)
    assert len(pairs_twin.pairs(a, None, 1, HALF)[0]) == B - 1 and len(pairs_twin.pairs(a, None, 1, HALF + 1)[0]) == 0
    assert not _check(a, 1, HALF).any()
    assert (_check(a, 1, HALF + 1) == np.arange(B)).all()
    got = _check(twin.chain(B, S, B + S, dtype, cut=True), 1, HALF)
    sizes = twin.table(got)[1]
    assert (len(sizes), int((sizes == 1).sum())) == {200: (8, 4), 330: (13, 6), 5: (1, 0)}[B]


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_cliques(dtype):
    got = _check(twin.cliques(330, 64, CLIQUES, 11, dtype), 1, 65536)
    assert sorted(twin.table(got)[1].tolist()) == sorted(CLIQUES)
    got = _check(twin.cliques(262, 8, (1, 2, 64, 65, 130), 12, dtype), 1, 65536)
    assert sorted(twin.table(got)[1].tolist()) == [1, 2, 64, 65, 130]


def test_cluster_pairs_ignores_padding_self_edges_and_out_of_range():
    from bioseq_amd import sketch
    a = twin.chain(200, 8, 1, np.int32, cut=True)
    exp = twin.labels(a, 1, HALF)
    row, col = sketch.sketch_pairs_host(a, min_jaccard=0.5, max_pairs=300, either=False)[:2]  # 192 pairs and (0, 0) padding behind them
    assert len(row) == 300 and not row[192:].any() and row[:192].any()
    assert sketch.cluster_pairs_host(row, col, 200).tobytes() == exp.tobytes()
    junk_r = np.array([5, 7, -1, 3, 200, 2 ** 62, 0, -2 ** 63], np.int64)
    junk_c = np.array([5, 7, 3, -1, 0, 1, 200, 1], np.int64)
    mixed_r, mixed_c = np.concatenate([junk_r, row, junk_r]), np.concatenate([junk_c, col, junk_c])
    assert sketch.cluster_pairs_host(mixed_r, mixed_c, 200).tobytes() == exp.tobytes()
    assert twin.labels_of_pairs(mixed_r, mixed_c, 200).tobytes() == exp.tobytes()
    assert sketch.cluster_pairs(mixed_c, mixed_r, 200).tobytes() == exp.tobytes()  # (numpy input: the host twin; an edge has no direction)
    assert sketch.cluster_pairs_host(junk_r, junk_c, 6).tolist() == [0, 1, 2, 3, 4, 5]
    assert sketch.cluster_pairs_host(row[:0], col[:0], 3).tolist() == [0, 1, 2] and sketch.cluster_pairs_host(row[:0], col[:0], 0).shape == (0,)
    # the order in which the links are met does not matter
    order = np.random.default_rng(4).permutation(192)
    assert sketch.cluster_pairs_host(col[:192][order], row[:192][order], 200).tobytes() == exp.tobytes()


def test_cluster_table_and_split_forms_agree():
    import torch
    from bioseq_amd import sketch
    lab = twin.labels(twin.cliques(330, 64, CLIQUES, 11), 1, 65536)
    exp = twin.table(lab)
    for got in (sketch.cluster_table(lab), [x.numpy() for x in sketch.cluster_table(torch.from_numpy(lab))]):
        assert all(g.dtype == np.int64 and g.tobytes() == e.tobytes() for g, e in zip(got, exp))
    assert exp[1].sum() == 330 and (exp[0][exp[2]] == lab).all()
    assert all(x.shape == (0,) for x in sketch.cluster_table(lab[:0])) and all(x.shape == (0,) for x in sketch.cluster_table(torch.from_numpy(lab[:0])))
    for fractions in ((0.8, 0.1, 0.1), (0.5, 0.5), (1.0,), (0.25, 0.25, 0.25, 0.25)):
        for seed in (0, 1, 12345, 2 ** 63, 2 ** 64 - 1, -7):
            want = twin.split(lab, fractions, seed)
            a, b = sketch.cluster_split(lab, fractions, seed), sketch.cluster_split(torch.from_numpy(lab), fractions, seed)
            assert a.dtype == np.int64 and b.dtype == torch.int64 and a.tobytes() == want.tobytes() and b.numpy().tobytes() == want.tobytes()
            assert (a == a[lab]).all() and a.max() < len(fractions)  # constant within every cluster
    assert (sketch.cluster_split(lab, (0.5, 0.5), 1) != sketch.cluster_split(lab, (0.5, 0.5), 2)).any()
    # rows appended behind keep the splits in front of them
    more = np.concatenate([lab, np.array([330, 5, 331, 331], np.int64)])
    assert (sketch.cluster_split(more, (0.8, 0.1, 0.1), 3)[:330] == sketch.cluster_split(lab, (0.8, 0.1, 0.1), 3)).all()
    for bad in ((), (0.5, 0.6), (0.5, 0.4), (1.2, -0.2), (0.5, 0.5, 0.0), (float("nan"), 0.5)):
        for form in (lab, torch.from_numpy(lab)):
            with pytest.raises(ValueError):
                sketch.cluster_split(form, bad)


def test_split_shares_of_singletons():
    """10 000 singleton clusters, fractions (0.8, 0.1, 0.1): a share is a binomial mean with sigma <= 0.004, so 0.02 is five sigma and more."""
    from bioseq_amd import sketch
    lab = np.arange(10000, dtype=np.int64)
    for seed in (0, 9):
        share = np.bincount(sketch.cluster_split(lab, (0.8, 0.1, 0.1), seed), minlength=3) / 10000.0
        assert np.abs(share - np.array([0.8, 0.1, 0.1])).max() < 0.02, share


def test_refusals_write_nothing():
    capi, L = _lib()
    from bioseq_amd import sketch
    a = pairs_twin.sketch_like(np.random.default_rng(0), 6, 8, np.int32)
    labels = np.full(6, 0x5A, np.int64)

    def call(rule, B=6, S=8, t=I32, out=labels):
        return L.bsq_sketch_clusters_host(a.ctypes.data, B, S, t, ctypes.byref(capi.SketchPairs(*rule)) if rule else None,
                                          out.ctypes.data if out is not None else None)

    for rule, kw in [((1, 0, 0, 0), {}), ((1, 0, 2, 0), {}),  # upper == 0 is not a clustering rule; upper not 0 / 1
                     ((1, -1, 1, 0), {}), ((1, 65537, 1, 0), {}), ((9, 0, 1, 0), {}), ((-1, 0, 1, 0), {}), ((1, 0, 1, 65), {}),
                     ((1, 0, 1, 0), {"S": 0}), ((1, 0, 1, 0), {"S": (1 << 14) + 1}), ((1, 0, 1, 0), {"B": -1}), ((1, 0, 1, 0), {"out": None}),
                     (None, {})]:
        assert call(rule, **kw) == capi.ERR_INVALID_ARG and L.bsq_last_error(), (rule, kw)
    for t in (0, 1, 4, 5):
        assert call((1, 0, 1, 0), t=t) == capi.ERR_DTYPE
    assert (labels == 0x5A).all()
    assert call((1, 0, 1, 0), B=0) == capi.OK and (labels == 0x5A).all()  # B == 0 writes nothing
    assert call((1, 0, 1, 0)) == capi.OK and labels[0] == 0
    edges = np.zeros(4, np.int64)
    labels[:] = 0x5A
    for n_pairs, n, row in ((-1, 6, edges), (4, -1, edges), (4, 2 ** 31, edges), (4, 6, None)):
        st = L.bsq_cluster_pairs_host(row.ctypes.data if row is not None else None, edges.ctypes.data, n_pairs, n, labels.ctypes.data)
        assert st == capi.ERR_INVALID_ARG
    assert L.bsq_cluster_pairs_host(edges.ctypes.data, edges.ctypes.data, 4, 6, None) == capi.ERR_INVALID_ARG
    assert L.bsq_cluster_pairs_host(edges.ctypes.data, edges.ctypes.data, 4, 0, labels.ctypes.data) == capi.OK and (labels == 0x5A).all()
    for refused in (lambda: sketch.sketch_clusters_host(a, min_jaccard=1.5), lambda: sketch.sketch_clusters_host(a, min_match=9),
                    lambda: sketch.sketch_clusters_host(a.astype(np.float32)), lambda: sketch.sketch_clusters_host(a[0]),
                    lambda: sketch.sketch_clusters(a, min_jaccard=float("nan")), lambda: sketch.sketch_clusters(a, segments=65),
                    lambda: sketch.sketch_clusters(np.zeros((2, (1 << 14) + 1), np.int32)), lambda: sketch.sketch_clusters([[1, 2]]),
                    lambda: sketch.cluster_pairs_host(edges, edges[:3], 6), lambda: sketch.cluster_pairs_host(edges.astype(np.int32), edges, 6),
                    lambda: sketch.cluster_pairs_host(edges, edges, -1), lambda: sketch.cluster_pairs_host(edges, edges, 2 ** 31),
                    lambda: sketch.cluster_pairs(edges.tolist(), edges.tolist(), 6)):
        with pytest.raises(ValueError):
            refused()
    assert sketch.sketch_clusters_host(a[:0]).shape == (0,)
    assert sketch.sketch_clusters_kernel_name(5) == sketch.sketch_clusters_kernel_name(262144, 2) == "k_cluster_init+k_sketch_link+k_cluster_labels"
    assert sketch.sketch_clusters_kernel_name(0) == sketch.sketch_clusters_kernel_name(5, 65) == sketch.sketch_clusters_kernel_name(2 ** 31) == ""
