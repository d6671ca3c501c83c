"""CPU: greedy representatives of an edge list (include/bsq.h, "greedy representatives") -- the declared symbols and the Python surface,
the header's known answers, the library's host twin bsq_greedy_pairs_host against the plain-Python twin (tests/greedy_twin.py) byte for
byte over every key / weight combination, the consequences the header states, `length_key`, the labels through `cluster_table` and
`cluster_split`, every refusal, and the planted-family pipeline on the host twins.  No device is needed."""
import ctypes

import numpy as np
import pytest

import greedy_twin as twin

I64 = np.int64


def _lib():
    from bioseq_amd import capi
    return capi, capi.load()


def _arr(values, dtype=I64):
    return np.array(values, dtype)


def _check(row, col, n, key=None, weight=None):
    """host twin == Python twin, byte for byte, and the consequences.  Returns rep."""
    from bioseq_amd import sketch
    exp = twin.greedy_reps(row, col, n, key, weight)
    got = sketch.greedy_pairs_host(row, col, n, key=key, weight=weight)
    assert got.dtype == I64 and got.shape == (n,) and got.tobytes() == exp.tobytes()
    twin.check_consequences(row, col, n, got, key)
    assert sketch.greedy_pairs(row, col, n, key=key, weight=weight).tobytes() == exp.tobytes()  # (numpy in: the twin)
    return got


def test_new_symbols_are_declared_and_exported():
    import bioseq_amd
    capi, L = _lib()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_greedy_scratch_bytes", "bsq_greedy_pairs_device", "bsq_greedy_pairs_host", "bsq_greedy_kernel_name"):
        assert n in names and hasattr(L, n), n
    assert L.bsq_abi_version() == 7
    for n in ("greedy_pairs", "greedy_pairs_host", "greedy_kernel_name", "length_key"):
        assert n in bioseq_amd.sketch.__all__ and callable(getattr(bioseq_amd.sketch, n))


def test_kernel_names_and_scratch_size():
    from bioseq_amd import sketch
    _, L = _lib()
    assert sketch.greedy_kernel_name() == "k_greedy_mark+k_greedy_decide;k_greedy_clear+k_greedy_best<index>+k_greedy_rep"
    assert sketch.greedy_kernel_name(key=True) == "k_greedy_mark+k_greedy_decide;k_greedy_clear+k_greedy_best<key>+k_greedy_best<index>+k_greedy_rep"
    assert sketch.greedy_kernel_name(weight=True) == "k_greedy_mark+k_greedy_decide;k_greedy_clear+k_greedy_best<weight>+k_greedy_best<index>+k_greedy_rep"
    assert sketch.greedy_kernel_name(key=True, weight=True) == ("k_greedy_mark+k_greedy_decide;k_greedy_clear+k_greedy_best<weight>+"
                                                                "k_greedy_best<key>+k_greedy_best<index>+k_greedy_rep")
    # 64 + 28 n, whatever the list's length
    assert L.bsq_greedy_scratch_bytes(0, 0) == 64 and L.bsq_greedy_scratch_bytes(1000, 5) == L.bsq_greedy_scratch_bytes(1000, 10 ** 9) == 28064
    assert L.bsq_greedy_scratch_bytes(2 ** 31 - 1, 0) == 64 + 28 * (2 ** 31 - 1)
    for n, m in ((-1, 0), (0, -1), (2 ** 31, 0)):
        assert L.bsq_greedy_scratch_bytes(n, m) < 0


def test_known_answers():
    """The answers of include/bsq.h."""
    a, b = twin.path(5)
    assert _check(a, b, 5).tolist() == [0, 0, 2, 2, 4]
    assert _check(a, b, 5, key=_arr([0, 0, 0, -1, 0])).tolist() == [0, 0, 3, 3, 3]
    assert _check(_arr([0, 0, 1, 2]), _arr([1, 2, 2, 3]), 4).tolist() == [0, 0, 0, 3]  # a triangle and a pendant
    r, c = _arr([0, 1]), _arr([2, 2])  # a member with two representative neighbours
    assert _check(r, c, 3).tolist() == [0, 1, 0]
    assert _check(r, c, 3, weight=_arr([1, 5], np.int32)).tolist() == [0, 1, 1]
    assert _check(r, c, 3, weight=_arr([5, 5], np.int32)).tolist() == [0, 1, 0]
    assert _check(r, c, 3, key=_arr([0, -1, 0])).tolist() == [0, 1, 1]  # by order: 1 comes first
    # of duplicate entries the largest weight counts, whichever way round they stand
    assert _check(_arr([0, 1, 2]), _arr([2, 2, 0]), 3, weight=_arr([1, 5, 9], np.int32)).tolist() == [0, 1, 0]
    # a representative neighbour that comes after the member is never chosen: 1 falls to 0, not to 2
    assert _check(_arr([0, 1]), _arr([1, 2]), 3, weight=_arr([1, 9], np.int32)).tolist() == [0, 0, 2]


@pytest.mark.parametrize("n, m", [(1, 0), (2, 1), (7, 30), (60, 90), (300, 700), (500, 5000)])
@pytest.mark.parametrize("has_key", [False, True])
@pytest.mark.parametrize("has_weight", [False, True])
def test_host_twin_equals_python_twin(n, m, has_key, has_weight):
    """Seeded random lists with junk entries, duplicates and both orientations; keys and weights with many ties."""
    row, col = twin.random_list(n * 31 + m, n, m)
    key, weight = twin.keys_and_weights(n + m, n, m)
    rep = _check(row, col, n, key if has_key else None, weight if has_weight else None)
    if n == 500:
        assert 0 < (rep == np.arange(n)).sum() < n  # (representatives and members both)


def test_shapes():
    """A path, the path through a permutation, a complete graph, a star whose centre comes last, an empty list."""
    from bioseq_amd import sketch
    a, b = twin.path(300)
    assert _check(a, b, 300).tolist() == [i - i % 2 for i in range(300)]
    perm = np.random.default_rng(7).permutation(300).astype(I64)
    _check(*twin.path(300, perm), 300)
    assert (_check(*twin.complete(64), 64) == 0).all()
    star = _check(np.full(9, 9, I64), np.arange(9, dtype=I64), 10)
    assert star.tolist() == list(range(9)) + [0]
    assert _check(np.full(9, 0, I64), np.arange(1, 10, dtype=I64), 10, key=_arr([1] + [0] * 9)).tolist() == [1] + list(range(1, 10))
    assert _check(np.zeros(0, I64), np.zeros(0, I64), 5).tolist() == [0, 1, 2, 3, 4]
    assert sketch.greedy_pairs_host(np.zeros(0, I64), np.zeros(0, I64), 0).size == 0


def test_result_depends_on_the_edges_and_the_order_alone():
    """A shuffled list with its ends exchanged gives the same bytes; a key with every value equal is index order; keys that order the
    nodes alike give the same representatives."""
    from bioseq_amd import sketch
    n, m = 400, 3000
    row, col = twin.random_list(11, n, m)
    key, weight = twin.keys_and_weights(11, n, m)
    p = np.random.default_rng(3).permutation(m)
    for k in (None, key):
        for w in (None, weight):
            want = sketch.greedy_pairs_host(row, col, n, key=k, weight=w)
            got = sketch.greedy_pairs_host(np.ascontiguousarray(col[p]), np.ascontiguousarray(row[p]), n, key=k, weight=None if w is None else np.ascontiguousarray(w[p]))
            assert got.tobytes() == want.tobytes()
    plain = sketch.greedy_pairs_host(row, col, n)
    assert sketch.greedy_pairs_host(row, col, n, key=np.full(n, -7, I64)).tobytes() == plain.tobytes()
    assert sketch.greedy_pairs_host(row, col, n, key=np.arange(n, dtype=I64) * 5 - 9).tobytes() == plain.tobytes()
    assert sketch.greedy_pairs_host(row, col, n, key=key * 3 + 1).tobytes() == sketch.greedy_pairs_host(row, col, n, key=key).tobytes()
    # the extreme keys are keys like any other
    ext = key.copy()
    ext[::3], ext[1::3] = np.iinfo(I64).min, np.iinfo(I64).max
    _check(row, col, n, key=ext, weight=np.where(weight > 0, np.iinfo(np.int32).max, np.iinfo(np.int32).min).astype(np.int32))


def test_length_key():
    import torch
    from bioseq_amd import sketch
    offs = _arr([0, 5, 5, 17, 20])
    assert sketch.length_key(offs).dtype == I64 and sketch.length_key(offs).tolist() == [-5, 0, -12, -3]
    assert sketch.length_key([0, 2, 3]).tolist() == [-2, -1]
    t = sketch.length_key(torch.from_numpy(offs))
    assert t.dtype == torch.int64 and t.is_contiguous() and t.tolist() == [-5, 0, -12, -3]
    # longest first, rows of one length to the earlier row: 2 (12), 0 (5), 3 (3), 1 (0)
    rep = sketch.greedy_pairs(*twin.complete(4), 4, key=sketch.length_key(offs))
    assert rep.tolist() == [2, 2, 2, 2]


def test_rep_serves_as_labels():
    """`cluster_table` and `cluster_split` take rep unchanged, in numpy and in torch."""
    import torch
    from bioseq_amd import sketch
    n = 300
    row, col = twin.random_list(5, n, 400)
    rep = sketch.greedy_pairs(row, col, n)
    reps, sizes, dense = sketch.cluster_table(rep)
    assert (reps == np.nonzero(rep == np.arange(n))[0]).all() and sizes.sum() == n and (reps[dense] == rep).all()
    assert all(sizes[k] == (rep == reps[k]).sum() for k in range(reps.size))
    split = sketch.cluster_split(rep, [0.5, 0.5], seed=1)
    assert (split == split[rep]).all() and set(split.tolist()) == {0, 1}
    treps, tsizes, tdense = sketch.cluster_table(torch.from_numpy(rep))
    assert treps.numpy().tobytes() == reps.tobytes() and tsizes.numpy().tobytes() == sizes.tobytes() and tdense.numpy().tobytes() == dense.tobytes()
    assert sketch.cluster_split(torch.from_numpy(rep), [0.5, 0.5], seed=1).numpy().tobytes() == split.tobytes()


def test_refusals():
    from bioseq_amd import sketch
    capi, L = _lib()
    row, col, rep = _arr([0, 1]), _arr([1, 2]), np.full(3, 7, I64)
    p = lambda a: a.ctypes.data
    assert L.bsq_greedy_pairs_host(p(row), p(col), None, -1, 3, None, p(rep)) == capi.ERR_INVALID_ARG
    assert L.bsq_greedy_pairs_host(p(row), p(col), None, 2, -1, None, p(rep)) == capi.ERR_INVALID_ARG
    assert L.bsq_greedy_pairs_host(p(row), p(col), None, 2, 2 ** 31, None, p(rep)) == capi.ERR_INVALID_ARG
    assert b"2^31" in L.bsq_last_error()
    assert L.bsq_greedy_pairs_host(None, p(col), None, 2, 3, None, p(rep)) == capi.ERR_INVALID_ARG
    assert L.bsq_greedy_pairs_host(p(row), None, None, 2, 3, None, p(rep)) == capi.ERR_INVALID_ARG
    assert L.bsq_greedy_pairs_host(p(row), p(col), None, 2, 3, None, None) == capi.ERR_INVALID_ARG
    assert L.bsq_greedy_pairs_host(p(row), p(col), None, 2, 0, None, None) == capi.OK  # n == 0 writes nothing
    assert rep.tolist() == [7, 7, 7]
    # the device call refuses before it touches a device
    args = (p(row), p(col), None, 2, 3, None)
    assert L.bsq_greedy_pairs_device(*args, None, 0, 1, p(rep), p(rep), None) == capi.ERR_INVALID_ARG
    assert L.bsq_greedy_pairs_device(*args, p(rep), 0, 1, None, p(rep), None) == capi.ERR_INVALID_ARG
    assert L.bsq_greedy_pairs_device(*args, p(rep), 0, 1, p(rep), None, None) == capi.ERR_INVALID_ARG
    assert L.bsq_greedy_pairs_device(*args, p(rep) + 4, 0, 1, p(rep), p(rep), None) == capi.ERR_INVALID_ARG
    assert L.bsq_greedy_pairs_device(*args, p(rep), -1, 1, p(rep), p(rep), None) == capi.ERR_INVALID_ARG
    assert L.bsq_greedy_pairs_device(*args, p(rep), 0, -1, p(rep), p(rep), None) == capi.ERR_INVALID_ARG
    assert L.bsq_greedy_pairs_device(*args, p(rep), 2 ** 30 - 1, 1, p(rep), p(rep), None) == capi.ERR_INVALID_ARG
    assert b"31 bits" in L.bsq_last_error()
    assert L.bsq_greedy_pairs_device(*args, p(rep), 1, 2 ** 62, p(rep), p(rep), None) == capi.ERR_INVALID_ARG
    assert L.bsq_greedy_pairs_device(None, p(col), None, 2, 3, None, p(rep), 0, 1, p(rep), p(rep), None) == capi.ERR_INVALID_ARG
    assert L.bsq_greedy_pairs_device(p(row), p(col), None, 2, 2 ** 31, None, p(rep), 0, 1, p(rep), p(rep), None) == capi.ERR_INVALID_ARG
    assert L.bsq_greedy_pairs_device(p(row), p(col), None, 2, 0, None, None, 0, 1, None, None, None) == capi.OK  # n == 0: nothing launched
    assert rep.tolist() == [7, 7, 7]
    # the wrapper's own rules
    for bad in (dict(row=row.astype(np.int32)), dict(col=col[:1]), dict(n=-1), dict(n=2 ** 31), dict(n=True), dict(key=_arr([0, 0])),
                dict(key=np.zeros(3, np.int32)), dict(weight=np.zeros(2, I64)), dict(weight=np.zeros(3, np.int32)), dict(max_rounds=-1),
                dict(max_rounds=2 ** 30), dict(rounds_per_call=0), dict(rounds_per_call=1.5)):
        kw = dict(row=row, col=col, n=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            sketch.greedy_pairs(kw.pop("row"), kw.pop("col"), kw.pop("n"), **kw)
    with pytest.raises(ValueError):
        sketch.greedy_pairs([0, 1], [1, 2], 3)  # neither numpy arrays nor device tensors
    rep2, left = sketch.greedy_pairs(row, col, 3, max_rounds=0)  # (numpy: the twin is always complete)
    assert rep2.tolist() == [0, 0, 2] and left == 0


def pipeline_host(tok):
    """The planted-family pipeline on the host twins: (rep, parent)."""
    from bioseq_amd import align, sketch
    chars, offsets, parent = twin.families()
    sk = sketch.minhash_host(tok, chars, offsets, 11, 128)
    row, col, *_ = sketch.sketch_pairs_host(sk, min_jaccard=0.2)
    keep, dist = align.verify_pairs_host(tok, chars, offsets, row, col, min_identity=0.9)
    rep = sketch.greedy_pairs(np.ascontiguousarray(row[keep]), np.ascontiguousarray(col[keep]), parent.size, key=sketch.length_key(offsets),
                              weight=np.ascontiguousarray(-dist[keep]))
    return rep, parent


def test_planted_families_on_the_host_twins():
    """12 families of one parent of 200 characters and 4 children (2 % substitutions, 0 .. 4 characters trimmed): minhash_host ->
    sketch_pairs_host(0.2) -> verify_pairs_host(0.9) -> greedy_pairs with length_key.  The representatives are exactly the 12 parents and
    every child maps to its parent (the GPU test relies on this seed)."""
    import bioseq_amd
    rep, parent = pipeline_host(bioseq_amd.Tokenizer("DNA4", False, False, False))
    assert rep.tolist() == parent.tolist() and (rep == np.arange(rep.size)).sum() == 12
