"""GPU: greedy representatives of an edge list on the device (include/bsq.h, "greedy representatives"; csrc/bsq_greedy.hip): the device
result equals the plain-Python twin (tests/greedy_twin.py) equals the library's host twin, byte for byte -- sizes around a workgroup, a
random list that spans hundreds of workgroups under every key / weight combination and in shuffled order, a path that needs as many
rounds as it has nodes (the resume loop, explicit pieces through the C ABI, a run cut short), dense and hub shapes, guard words, a dirty
scratch, surplus rounds, and the planted-family pipeline."""
import functools

import numpy as np
import pytest

import greedy_twin as twin

pytestmark = pytest.mark.gpu

I64 = np.int64
N_BIG, M_BIG = 20000, 200000


def _dev(gpu, a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).to(gpu)  # (a copy: the shared lists are read-only)


def _device_rep(gpu, row, col, n, key=None, weight=None, **kw):
    from bioseq_amd import sketch
    out = sketch.greedy_pairs(_dev(gpu, row), _dev(gpu, col), n, key=_dev(gpu, key), weight=_dev(gpu, weight), **kw)
    if isinstance(out, tuple):
        return out[0].cpu().numpy(), int(out[1].item())
    assert out.device.type == "cuda" and out.shape == (n,)
    return out.cpu().numpy()


def _check(gpu, row, col, n, key=None, weight=None, want=None, **kw):
    """device == Python twin == host twin, byte for byte.  Returns rep."""
    from bioseq_amd import sketch
    want = twin.greedy_reps(row, col, n, key, weight) if want is None else want
    assert sketch.greedy_pairs_host(row, col, n, key=key, weight=weight).tobytes() == want.tobytes()
    got = _device_rep(gpu, row, col, n, key, weight, **kw)
    assert got.dtype == I64 and got.tobytes() == want.tobytes()
    return got


@functools.lru_cache(maxsize=None)
def _big():
    """The random list of 20 000 nodes and 200 000 entries (junk included), its key and weight, and the twin's answer for each of the
    four combinations: computed once, never changed."""
    row, col = twin.random_list(2024, N_BIG, M_BIG)
    key, weight = twin.keys_and_weights(2024, N_BIG, M_BIG)
    want = {(k, w): twin.greedy_reps(row, col, N_BIG, key if k else None, weight if w else None) for k in (False, True) for w in (False, True)}
    for a in (row, col, key, weight, *want.values()):
        a.setflags(write=False)
    return row, col, key, weight, want


def _raw_call(gpu, row, col, n, pieces, key=None, weight=None, dirty=False):
    """bsq_greedy_pairs_device through the C ABI in the given (round0, rounds) pieces, with guard words around rep and undecided and,
    with `dirty`, a scratch of 0xFF bytes: (rep after the last piece, undecided after each piece)."""
    import torch
    from bioseq_amd import capi
    L = capi.load()
    drow, dcol, dkey, dw = _dev(gpu, row), _dev(gpu, col), _dev(gpu, key), _dev(gpu, weight)
    nbytes = L.bsq_greedy_scratch_bytes(n, len(row))
    assert nbytes == 64 + 28 * n
    scratch = torch.full((nbytes + 16,), 0xFF if dirty else 0, dtype=torch.uint8, device=gpu)  # (8 guard bytes behind the scratch)
    out = torch.full((n + 16,), -77, dtype=torch.int64, device=gpu)  # rep at 8 .. 8 + n, guard words on both sides
    left = torch.full((3,), -77, dtype=torch.int64, device=gpu)      # undecided at 1
    assert scratch.data_ptr() % 8 == 0
    counts = []
    for round0, rounds in pieces:
        with capi.launching(gpu) as stream:
            capi.check(L.bsq_greedy_pairs_device(drow.data_ptr(), dcol.data_ptr(), None if dw is None else dw.data_ptr(), len(row), n,
                                                 None if dkey is None else dkey.data_ptr(), scratch.data_ptr(), round0, rounds,
                                                 out.data_ptr() + 64, left.data_ptr() + 8, stream))
        counts.append(int(left[1].item()))
    host, tail = out.cpu().numpy(), scratch[nbytes:].cpu().numpy()
    assert (host[:8] == -77).all() and (host[8 + n:] == -77).all() and left.cpu().tolist()[::2] == [-77, -77]
    assert (tail == (0xFF if dirty else 0)).all()
    return host[8:8 + n].copy(), counts


@pytest.mark.parametrize("n, m", [(1, 0), (5, 0), (2, 1), (40, 257), (300, 513)])
def test_small_sizes(gpu, bsq, n, m):
    """One node, an empty list, lists one entry above a multiple of the workgroup size."""
    row, col = twin.random_list(n + m, n, m)
    key, weight = twin.keys_and_weights(n, n, m)
    for k in (None, key):
        for w in (None, weight):
            _check(gpu, row, col, n, k, w)


def test_no_nodes(gpu, bsq):
    import torch
    from bioseq_amd import sketch
    e = torch.zeros(0, dtype=torch.int64, device=gpu)
    assert sketch.greedy_pairs(e, e, 0).shape == (0,)
    rep, left = sketch.greedy_pairs(e, e, 0, max_rounds=3)
    assert rep.shape == (0,) and int(left.item()) == 0


@pytest.mark.parametrize("has_key", [False, True])
@pytest.mark.parametrize("has_weight", [False, True])
def test_large_random_list(gpu, bsq, has_key, has_weight):
    """782 workgroups of entries, 79 of nodes; the list shuffled with its ends exchanged gives the same bytes."""
    row, col, key, weight, want = _big()
    k, w = key if has_key else None, weight if has_weight else None
    rep = _check(gpu, row, col, N_BIG, k, w, want=want[has_key, has_weight])
    assert 0 < (rep == np.arange(N_BIG)).sum() < N_BIG
    p = np.random.default_rng(1).permutation(M_BIG)
    got = _device_rep(gpu, col[p], row[p], N_BIG, k, None if w is None else w[p])
    assert got.tobytes() == rep.tobytes()


def test_large_list_consequences(gpu, bsq):
    row, col, key, weight, want = _big()
    twin.check_consequences(row, col, N_BIG, _device_rep(gpu, row, col, N_BIG, key, weight), key)


def test_surplus_rounds(gpu, bsq):
    """1000 rounds in one call where about ten are needed: the same bytes, nothing left."""
    row, col, key, weight, want = _big()
    rep, left = _device_rep(gpu, row, col, N_BIG, key, weight, max_rounds=1000)
    assert rep.tobytes() == want[True, True].tobytes() and left == 0


def test_random_list_cut_short(gpu, bsq):
    """After 2 rounds: rep is -1 or final, the count is the number of -1 entries, and some of both exist."""
    row, col, key, weight, want = _big()
    for k, w in ((None, None), (key, weight)):
        rep, left = _device_rep(gpu, row, col, N_BIG, k, w, max_rounds=2)
        open_ = rep == -1
        assert 0 < open_.sum() == left < N_BIG
        assert (rep[~open_] == want[k is not None, w is not None][~open_]).all()


def test_member_waits_for_an_open_earlier_neighbour(gpu, bsq):
    """0 -- 1 -- 2 -- 5 -- 4: after two rounds 5 is a member (4 is kept) but 2 is still open and will be its representative: rep[5] is
    -1 until 2 is decided."""
    row, col = np.array([0, 1, 2, 4], I64), np.array([1, 2, 5, 5], I64)
    rep, left = _device_rep(gpu, row, col, 6, max_rounds=1)
    assert rep.tolist() == [0, -1, -1, 3, 4, -1] and left == 3
    rep, left = _device_rep(gpu, row, col, 6, max_rounds=2)
    assert rep.tolist() == [0, 0, -1, 3, 4, -1] and left == 2
    rep, left = _device_rep(gpu, row, col, 6, max_rounds=3)
    assert rep.tolist() == [0, 0, 2, 3, 4, 2] and left == 0
    _check(gpu, row, col, 6)


def test_path_in_index_order(gpu, bsq):
    """300 rounds: the resume loop goes through 16 + 32 + 64 + 128 + 256."""
    a, b = twin.path(300)
    assert _check(gpu, a, b, 300).tolist() == [i - i % 2 for i in range(300)]
    _check(gpu, a, b, 300, rounds_per_call=1)  # 1 + 2 + 4 + ... + 256
    _check(gpu, a, b, 300, rounds_per_call=300)


def test_path_in_resumed_pieces(gpu, bsq):
    """Explicit pieces through the C ABI equal one call; the count falls by one a round."""
    a, b = twin.path(300)
    want = twin.greedy_reps(a, b, 300)
    whole, counts = _raw_call(gpu, a, b, 300, [(0, 400)])
    assert whole.tobytes() == want.tobytes() and counts == [0]
    rep, counts = _raw_call(gpu, a, b, 300, [(0, 7), (7, 43), (50, 0), (50, 100), (150, 200)], dirty=True)
    assert rep.tobytes() == want.tobytes() and counts == [293, 250, 250, 150, 0]
    rep, counts = _raw_call(gpu, a, b, 300, [(0, 0), (0, 300)], dirty=True)  # (no round: everything open; a run may start twice)
    assert rep.tobytes() == want.tobytes() and counts == [300, 0]


def test_path_cut_after_five_rounds(gpu, bsq):
    a, b = twin.path(300)
    rep, left = _device_rep(gpu, a, b, 300, max_rounds=5)
    assert left == 295
    assert (rep[5:] == -1).all() and rep[:5].tolist() == [0, 0, 2, 2, 4]


def test_scrambled_path(gpu, bsq):
    perm = np.random.default_rng(7).permutation(300).astype(I64)
    a, b = twin.path(300, perm)
    _check(gpu, a, b, 300)
    _check(gpu, a, b, 300, key=np.argsort(perm).astype(I64))  # the key that restores the path's own order: 300 rounds again


def test_dense_and_hub_shapes(gpu, bsq):
    """The complete graph on 64 nodes (2016 entries on 63 marks); a star whose centre comes last (4999 entries on one mark), by index
    and by key, with weights."""
    assert (_check(gpu, *twin.complete(64), 64) == 0).all()
    n = 5000
    leaves = np.arange(n - 1, dtype=I64)
    rep = _check(gpu, np.full(n - 1, n - 1, I64), leaves, n)
    assert rep[-1] == 0 and (rep[:-1] == leaves).all()
    key = np.zeros(n, I64)
    key[0] = 1  # the centre 0 comes last
    weight = (np.arange(n - 1) % 7).astype(np.int32)
    rep = _check(gpu, np.zeros(n - 1, I64), leaves + 1, n, key, weight)
    assert rep[0] == 7  # the first leaf of weight 6 is node 7


def test_key_ties(gpu, bsq):
    """A key with every value equal is index order."""
    row, col, _, weight, want = _big()
    got = _device_rep(gpu, row, col, N_BIG, np.full(N_BIG, 5, I64), weight)
    assert got.tobytes() == want[False, True].tobytes()


def test_guards_and_dirty_scratch(gpu, bsq):
    """Guard words around rep, undecided and the scratch stay; a scratch of 0xFF bytes is initialised by a round0 = 0 call."""
    row, col, key, weight, want = _big()
    rep, counts = _raw_call(gpu, row, col, N_BIG, [(0, 64)], key, weight, dirty=True)
    assert rep.tobytes() == want[True, True].tobytes() and counts == [0]
    rep, counts = _raw_call(gpu, row, col, N_BIG, [(0, 3), (3, 61)], dirty=True)
    assert rep.tobytes() == want[False, False].tobytes() and counts[0] > 0 and counts[1] == 0


def test_pipeline_on_the_device(gpu, bsq):
    """The planted-family pipeline on the device equals the pipeline on the host twins bit for bit (tests/test_greedy_host.py asserts
    what that answer is)."""
    import torch
    from bioseq_amd import align, sketch
    from test_greedy_host import pipeline_host
    tok = bsq.Tokenizer("DNA4", False, False, False)
    want, parent = pipeline_host(tok)
    chars, offsets, _ = twin.families()
    dc, do = _dev(gpu, chars), _dev(gpu, offsets)
    sk = sketch.minhash_packed(tok, dc, do, 11, 128)
    row, col, *_ = sketch.sketch_pairs(sk, min_jaccard=0.2)
    keep, dist = align.verify_pairs(tok, dc, do, row, col, min_identity=0.9)
    rep = sketch.greedy_pairs(row[keep], col[keep], parent.size, key=sketch.length_key(do), weight=-dist[keep])
    assert rep.cpu().numpy().tobytes() == want.tobytes() == parent.tobytes()
    assert (rep == torch.arange(parent.size, device=gpu)).sum().item() == 12


def test_surface_and_refusals(gpu, bsq):
    import torch
    from bioseq_amd import sketch
    row, col = _dev(gpu, np.array([0, 1], I64)), _dev(gpu, np.array([1, 2], I64))
    key, weight = torch.zeros(3, dtype=torch.int64, device=gpu), torch.zeros(2, dtype=torch.int32, device=gpu)
    rep = sketch.greedy_pairs(row, col, 3, key=key, weight=weight)
    assert rep.dtype == torch.int64 and rep.device == row.device and rep.tolist() == [0, 0, 2]
    rep, left = sketch.greedy_pairs(row, col, 3, max_rounds=0)
    assert rep.tolist() == [-1, -1, -1] and left.dtype == torch.int64 and left.device == row.device and left.item() == 3
    for bad in (dict(row=row.cpu()), dict(col=col.cpu()), dict(row=row.to(torch.int32)), dict(col=col[:1]), dict(row=torch.zeros(4, dtype=torch.int64, device=gpu)[::2]),
                dict(key=key.cpu()), dict(key=key.to(torch.int32)), dict(key=key[:2]), dict(key=key.cpu().numpy()), dict(weight=weight.cpu()),
                dict(weight=weight.to(torch.int64)), dict(weight=torch.zeros(3, dtype=torch.int32, device=gpu)), dict(n=-1), dict(n=2 ** 31),
                dict(max_rounds=-1), dict(rounds_per_call=0)):
        kw = dict(row=row, col=col, n=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            sketch.greedy_pairs(kw.pop("row"), kw.pop("col"), kw.pop("n"), **kw)
