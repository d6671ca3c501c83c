"""GPU: the LSH candidates of a sketch matrix on the device (include/bsq.h, "LSH candidates of a sketch matrix"; csrc/bsq_lsh.hip) against
the library's host twins, bit for bit, at the smallest shapes that can go wrong: the keys at widths and row counts around a workgroup's
64 x 64 tile, count and emit over planted groups whose runs cross positions 64 and 256 of a band, the list compare at every lane
ladder step and load form, and the whole call against `sketch_pairs` restricted to the pairs the plain-Python twin (tests/lsh_twin.py)
says collide."""
import ctypes
import functools

import numpy as np
import pytest

import lsh_twin as twin

pytestmark = pytest.mark.gpu

I64 = np.int64
NP = {"i": np.int32, "q": np.int64}


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.array(a)).to(gpu)  # (a copy: the shared matrices are read-only)


def _edge_rows(v):
    """row 0 EMPTY throughout (an empty sequence), the last row with a single filled bucket"""
    v = v.copy()
    v[0] = -1
    if v.shape[0] > 1:
        v[-1] = -1
        v[-1, v.shape[1] // 2] = 12345
    return v


# ---- keys ----
@pytest.mark.parametrize("destchar", ["i", "q"])
@pytest.mark.parametrize("S,r", [(128, 1), (128, 4), (128, 5), (128, 128), (1024, 8), (3, 2)])
def test_keys_equal_the_host_twin(gpu, S, r, destchar):
    from bioseq_amd import sketch
    for N in (1, 63, 65, 300):
        a = _edge_rows(twin.random_sketches(S * 1000 + N, N, S, NP[destchar], fill=0.7))
        want = sketch.lsh_keys_host(a, r, seed=5)
        got = sketch.lsh_keys(_dev(gpu, a), r, seed=5)
        assert got.device.type == "cuda" and tuple(got.shape) == (S // r, N) == want.shape
        assert got.cpu().numpy().tobytes() == want.tobytes(), (S, r, N)
        assert (want[:, 0] == -1).all()  # the EMPTY row: void in every band
        if N > 1:
            assert (want[:, -1] != -1).sum() == 1  # the single filled bucket: one band is not void (S // 2 lies inside the first T r)


def test_keys_of_b_are_written_behind_those_of_a_and_nothing_else(gpu):
    """the raw call with a pitch: two matrices into one key matrix, guard columns untouched"""
    import torch
    from bioseq_amd import capi, sketch
    L = capi.load()
    a, b = twin.random_sketches(1, 70, 128, fill=0.8), twin.random_sketches(2, 130, 128, fill=0.8)
    rule = capi.Lsh(4, 32, 9, 0)
    pitch = 70 + 130 + 3
    keys = torch.full((32, pitch), -77, dtype=torch.int64, device=gpu)
    da, db = _dev(gpu, a), _dev(gpu, b)
    with capi.launching(gpu) as stream:
        capi.check(L.bsq_lsh_keys_device(da.data_ptr(), 70, 128, capi.I32, ctypes.byref(rule), keys.data_ptr(), pitch, stream))
        capi.check(L.bsq_lsh_keys_device(db.data_ptr(), 130, 128, capi.I32, ctypes.byref(rule), keys.data_ptr() + 8 * 70, pitch, stream))
    host = keys.cpu().numpy()
    assert (host[:, 200:] == -77).all()
    assert host[:, :200].tobytes() == sketch.lsh_keys_host(np.concatenate([a, b]), 4, seed=9).tobytes()


# ---- count / emit ----
GROUPS_N = 300


def _expected_runs(skeys, order, max_bucket):
    """(counts, codes in position order) of sorted bands, by a plain walk of the runs"""
    T, N = skeys.shape
    counts, codes = np.zeros((T, N), I64), []
    for t in range(T):
        head = 0
        while head < N:
            end = head
            while end < N and skeys[t, end] == skeys[t, head]:
                end += 1
            if skeys[t, head] != -1:
                long_run = end - head > max_bucket
                for p in range(head + 1, end):
                    mine = [head] if long_run else range(head, p)
                    counts[t, p] = len(mine)
                    codes += [int(order[t, e]) * N + int(order[t, p]) for e in mine]
            head = end
    return counts, np.array(codes, I64)


GROUP_BANDS = (20, 21)  # the buckets (bands at r = 1) that hold the groups of max_bucket and max_bucket + 1 rows


@functools.lru_cache(maxsize=None)
def _grouped(max_bucket):
    """300 rows of 128 buckets, r = 1.  Whole rows made identical in disjoint groups of 2, 3 and 70 scattered rows: each is a run in
    every band, at 128 different places, some across position 64, some across position 256.  Groups of max_bucket and max_bucket + 1
    scattered rows made identical in ONE bucket each (GROUP_BANDS: at max_bucket = 128 the two together exceed 300 rows, so they
    cannot be disjoint whole rows): a run that yields all its pairs and one that yields its centre's.  Bucket 7 EMPTY in every row (a
    band in which every row is void) and bucket 9 equal in every row (a band in which all rows share one key)."""
    rng = np.random.default_rng(2029 + max_bucket)
    rows = rng.permutation(GROUPS_N)
    groups, at = [], 0
    for n in (2, 3, 70):
        groups.append(sorted(int(x) for x in rows[at:at + n]))
        at += n
    a = twin.random_sketches(77, GROUPS_N, 128, fill=0.9, groups=groups).copy()
    for band, n in zip(GROUP_BANDS, (max_bucket, max_bucket + 1)):
        a[:, band] = np.arange(1000, 1000 + GROUPS_N)  # (every row its own value, then the group's)
        a[rng.choice(GROUPS_N, n, replace=False), band] = 555
    a[:, 7] = -1
    a[:, 9] = 4242
    a.setflags(write=False)
    return a, groups


def _run_lengths(keys):
    """the lengths of the runs of one sorted band"""
    edges = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1], [True]]))
    return set(np.diff(edges).tolist())


@pytest.mark.parametrize("max_bucket", [4, 128, 69, 70])  # (69 / 70: the whole-row group of 70 on either side of the rule)
def test_count_and_emit_over_planted_groups(gpu, max_bucket):
    import torch
    from bioseq_amd import capi, sketch
    L = capi.load()
    a, groups = _grouped(max_bucket)
    N, T = GROUPS_N, 128
    keys = sketch.lsh_keys(_dev(gpu, a), 1)
    assert keys.cpu().numpy().tobytes() == sketch.lsh_keys_host(a, 1).tobytes()
    skeys, order = torch.sort(keys, dim=1, stable=True)
    hk, ho = skeys.cpu().numpy(), order.cpu().numpy()
    # the shapes this test is about, read from the sorted keys
    crosses = lambda t, at: hk[t, at - 1] == hk[t, at] != -1
    assert any(crosses(t, 64) for t in range(T)) and any(crosses(t, 256) for t in range(T))
    assert (hk[7] == -1).all() and (hk[9] == hk[9, 0]).all() and hk[9, 0] != -1
    assert _run_lengths(hk[GROUP_BANDS[0]]) == {1, max_bucket} and _run_lengths(hk[GROUP_BANDS[1]]) == {1, max_bucket + 1}
    want_counts, want_codes = _expected_runs(hk, ho, max_bucket)
    rule = capi.Lsh(1, max_bucket, 0, 0)
    counts = torch.full((T * N + 2,), -77, dtype=torch.int64, device=gpu)  # guard words on both sides
    with capi.launching(gpu) as stream:
        capi.check(L.bsq_lsh_count_device(skeys.data_ptr(), T, N, ctypes.byref(rule), counts.data_ptr() + 8, stream))
    hc = counts.cpu().numpy()
    assert hc[0] == -77 and hc[-1] == -77 and hc[1:-1].tobytes() == want_counts.tobytes()
    assert want_counts[9].sum() == N - 1  # the shared key: a long run at every max_bucket, the centre's pairs
    assert want_counts[GROUP_BANDS[0]].sum() == max_bucket * (max_bucket - 1) // 2 and want_counts[GROUP_BANDS[1]].sum() == max_bucket
    starts = torch.cumsum(counts[1:-1], 0) - counts[1:-1]
    total = int(want_counts.sum())
    codes = torch.full((total + 2,), -77, dtype=torch.int64, device=gpu)
    with capi.launching(gpu) as stream:
        capi.check(L.bsq_lsh_emit_device(skeys.data_ptr(), order.data_ptr(), T, N, ctypes.byref(rule), starts.data_ptr(), total,
                                         codes.data_ptr() + 8, stream))
    he = codes.cpu().numpy()
    assert he[0] == -77 and he[-1] == -77 and he[1:-1].tobytes() == want_codes.tobytes()
    # a capacity below the total: nothing at or past it
    short = torch.full((total,), -77, dtype=torch.int64, device=gpu)
    with capi.launching(gpu) as stream:
        capi.check(L.bsq_lsh_emit_device(skeys.data_ptr(), order.data_ptr(), T, N, ctypes.byref(rule), starts.data_ptr(), total // 2,
                                         short.data_ptr(), stream))
    hs = short.cpu().numpy()
    assert hs[:total // 2].tobytes() == want_codes[:total // 2].tobytes() and (hs[total // 2:] == -77).all()
    # the union is the rule's candidate set (the plain-Python twin), and the public call returns it
    cand, before = twin.candidates(a, rows_per_band=1, max_bucket=max_bucket)
    assert before == total and sorted(set((int(c) // N, int(c) % N) for c in want_codes)) == cand
    row, col = sketch.lsh_candidates(_dev(gpu, a), rows_per_band=1, max_bucket=max_bucket)
    assert list(zip(row.cpu().tolist(), col.cpu().tolist())) == cand
    with pytest.raises(ValueError, match="max_bucket.*rows_per_band"):
        sketch.lsh_candidates(_dev(gpu, a), rows_per_band=1, max_bucket=max_bucket, max_candidates=total - 1)
    assert sketch.lsh_candidates(_dev(gpu, a), rows_per_band=1, max_bucket=max_bucket, max_candidates=total)[0].numel() == len(cand)
    for g in groups:  # every planted group is inside the candidates as the rule says: all pairs, or the centre's
        inside = {(i, j) for i, j in cand if i in g and j in g}
        assert {(g[0], j) for j in g[1:]} <= inside


# ---- list compare ----
@pytest.mark.parametrize("destchar", ["i", "q"])
@pytest.mark.parametrize("S", [1, 3, 128, 129, 1024, 16384])
def test_list_compare_equals_the_dense_entries(gpu, S, destchar):
    import torch
    from bioseq_amd import sketch
    Ba, Bb = 40, 25
    a = _edge_rows(twin.near_duplicates(S, Ba, S, NP[destchar], share=0.3, fill=0.8))
    b = twin.near_duplicates(S + 1, Bb, S, NP[destchar], share=0.3, fill=0.8)
    b[3] = a[5]
    da, db = _dev(gpu, a), _dev(gpu, b)
    dense = {False: [x.cpu().numpy() for x in sketch.sketch_compare(da, db)], True: [x.cpu().numpy() for x in sketch.sketch_compare(da)]}
    rng = np.random.default_rng(S)
    for same in (False, True):
        hi = Ba if same else Bb
        for n in (0, 1, 63, 65, 1000):
            row, col = rng.integers(0, Ba, n).astype(I64), rng.integers(0, hi, n).astype(I64)
            if n >= 63:
                row[:4], col[:4] = (5, 5, 7, 7), (3, 3, 7, 7)  # repeats, and i = j
                row[10], col[11], row[12], col[13] = -1, -1, Ba, hi  # outside, at both ends
                row[14], col[14] = np.iinfo(I64).min, np.iinfo(I64).max
            by_row = np.argsort(row, kind="stable")  # (the list arrives sorted by row)
            row, col = row[by_row], col[by_row]
            ok = (row >= 0) & (row < Ba) & (col >= 0) & (col < hi)
            wm = np.where(ok, dense[same][0][np.where(ok, row, 0), np.where(ok, col, 0)], -1).astype(np.int32)
            we = np.where(ok, dense[same][1][np.where(ok, row, 0), np.where(ok, col, 0)], -1).astype(np.int32)
            hm, he = sketch.sketch_compare_list_host(a, row, col, None if same else b)
            assert hm.tobytes() == wm.tobytes() and he.tobytes() == we.tobytes()
            gm, ge = sketch.sketch_compare_list(da, _dev(gpu, row), _dev(gpu, col), None if same else db)
            assert gm.dtype == torch.int32 and gm.cpu().numpy().tobytes() == wm.tobytes() and ge.cpu().numpy().tobytes() == we.tobytes(), (S, n, same)
            gm, ge = sketch.sketch_compare_list(da, _dev(gpu, row), _dev(gpu, col), None if same else db, either=False)
            assert ge is None and gm.cpu().numpy().tobytes() == wm.tobytes()


def test_list_compare_takes_element_loads_for_a_view_off_16_bytes(gpu):
    """a contiguous view that starts 4 bytes into an allocation: the same answers by the element form"""
    import torch
    from bioseq_amd import sketch
    a = twin.near_duplicates(8, 33, 128, share=0.5)
    flat = torch.empty(33 * 128 + 1, dtype=torch.int32, device=gpu)
    view = flat[1:].view(33, 128)
    view.copy_(_dev(gpu, a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    row, col = np.arange(33, dtype=I64), np.arange(33, dtype=I64)[::-1].copy()
    wm, we = sketch.sketch_compare_list_host(a, row, col)
    gm, ge = sketch.sketch_compare_list(view, _dev(gpu, row), _dev(gpu, col))
    assert gm.cpu().numpy().tobytes() == wm.tobytes() and ge.cpu().numpy().tobytes() == we.tobytes()


# ---- the whole call ----
def _reads(seed, B, L=300):
    """random DNA reads; a tenth of them copies of an earlier read with 1 % substitutions, rows 3 and 4 exact copies of row 2, rows 5 and
    6 empty: (chars, offsets) as numpy"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 4, (B, L), dtype=np.uint8)
    dup = rng.choice(np.arange(7, B), B // 10, replace=False)
    src = (rng.random(dup.size) * dup).astype(I64)
    ids[dup] = ids[src]
    edits = rng.integers(0, L, (dup.size, max(1, L // 100)))
    ids[dup[:, None], edits] = rng.integers(0, 4, edits.shape, dtype=np.uint8)
    ids[3] = ids[4] = ids[2]
    lens = np.full(B, L, I64)
    lens[5] = lens[6] = 0
    chars = np.concatenate([np.frombuffer(b"ACGT", np.uint8)[ids[i, :lens[i]]] for i in range(B)])
    return chars, np.concatenate([[0], np.cumsum(lens)]).astype(I64)


@functools.lru_cache(maxsize=None)
def _store(B):
    """the int32 sketches of _reads(B) from the library's host twin, the twin's colliding pairs at r = 3, read-only"""
    from bioseq_amd import Tokenizer, sketch
    chars, offs = _reads(B, B)
    a = sketch.minhash_host(Tokenizer("DNA4", False, False, False), chars, offs, 21, 128, canonical=True)
    cand, _ = twin.candidates(a, rows_per_band=3, max_bucket=B)
    a.setflags(write=False)
    return a, cand


@pytest.mark.parametrize("B", [300, 2000])
def test_whole_call_is_sketch_pairs_restricted_to_colliding_pairs(gpu, B):
    import torch
    from bioseq_amd import sketch
    a, cand = _store(B)
    da = _dev(gpu, a)
    got = sketch.lsh_pairs(da, rows_per_band=3, max_bucket=B)
    host = sketch.lsh_pairs(a, rows_per_band=3, max_bucket=B)
    assert all(g.device.type == "cuda" for g in got)
    assert [g.dtype for g in got] == [torch.int64, torch.int64, torch.int32, torch.int32, torch.int64]
    for g, h in zip(got, host):
        assert g.cpu().numpy().dtype == h.dtype and g.cpu().numpy().tobytes() == h.tobytes()
    full = [x.cpu().numpy() for x in sketch.sketch_pairs(da, min_jaccard=0.5)]
    colliding = set(cand)
    keep = np.array([(int(i), int(j)) in colliding for i, j in zip(full[0], full[1])], bool)
    assert keep.sum() >= B // 20 and keep.sum() >= 0.9 * keep.size  # most planted copies pass 0.5 (J ~ 0.63), and LSH loses hardly any (predicted recall 0.996)
    for g, f in zip(got[:4], full[:4]):
        assert g.cpu().numpy().tobytes() == f[keep].tobytes()
    assert got[4].cpu().numpy().tobytes() == np.searchsorted(full[0][keep], np.arange(B + 1)).astype(I64).tobytes()
    listed = set(zip(got[0].cpu().tolist(), got[1].cpu().tolist()))
    assert {(2, 3), (2, 4), (3, 4)} <= listed                       # identical rows: always
    assert not any(5 in p or 6 in p for p in listed)               # EMPTY throughout: never
    # the default max_bucket changes nothing here (no run is that long), either=False drops one output only
    again = sketch.lsh_pairs(da, rows_per_band=3, either=False)
    assert again[3] is None and all(torch.equal(x, y) for x, y in zip(again[:3] + again[4:], got[:3] + got[4:]))
    # another seed: other keys, the identical rows still listed
    assert not torch.equal(sketch.lsh_keys(da, 3, seed=1), sketch.lsh_keys(da, 3))
    seeded = sketch.lsh_pairs(da, rows_per_band=3, seed=1)
    assert {(2, 3), (2, 4), (3, 4)} <= set(zip(seeded[0].cpu().tolist(), seeded[1].cpu().tolist()))
    assert seeded[0].cpu().numpy().tobytes() == sketch.lsh_pairs(a, rows_per_band=3, seed=1)[0].tobytes()


def test_whole_call_with_two_matrices_and_the_centre_rule(gpu):
    from bioseq_amd import sketch
    a, _ = _store(300)
    top, rest = a[:120], a[120:]
    for kw in ({"rows_per_band": 3}, {"rows_per_band": 1, "max_bucket": 2, "min_jaccard": 0.3}, {"rows_per_band": 128, "min_match": 0}):
        got = sketch.lsh_pairs(_dev(gpu, top), _dev(gpu, rest), **kw)
        host = sketch.lsh_pairs(top, rest, **kw)
        for g, h in zip(got, host):
            assert g.cpu().numpy().tobytes() == h.tobytes(), kw
        assert got[4].numel() == 121 and int(got[4][-1]) == got[0].numel()
        one = sketch.lsh_pairs(_dev(gpu, a), **kw)
        assert one[0].cpu().numpy().tobytes() == sketch.lsh_pairs(a, **kw)[0].tobytes()
    want = twin.lsh_pairs(top, rest, rows_per_band=3)
    for g, w in zip(sketch.lsh_pairs(_dev(gpu, top), _dev(gpu, rest), rows_per_band=3), want):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    # int64 sketches of the same batch: the same list
    wide = twin.as_dtype(a.view(np.uint32), np.int64)
    assert sketch.lsh_pairs(_dev(gpu, wide), rows_per_band=3)[0].cpu().numpy().tobytes() == sketch.lsh_pairs(a, rows_per_band=3)[0].tobytes()
    # empty sides
    for x, y in ((a[:0], None), (a[:0], a), (a, a[:0])):
        got = sketch.lsh_pairs(_dev(gpu, x), None if y is None else _dev(gpu, y), rows_per_band=3)
        assert got[0].numel() == 0 and got[4].cpu().tolist() == [0] * (x.shape[0] + 1)
    # what the device calls refuse: a `b` of another width or element type; a row that is not contiguous, an int32 row, two lengths
    import torch
    da, idx = _dev(gpu, a), torch.zeros(4, dtype=torch.int64, device=gpu)
    for call in (lambda: sketch.lsh_pairs(da, da[:, :64].contiguous(), rows_per_band=3), lambda: sketch.lsh_pairs(da, _dev(gpu, wide), rows_per_band=3),
                 lambda: sketch.sketch_compare_list(da, idx[::2], idx[:2]), lambda: sketch.sketch_compare_list(da, idx.to(torch.int32), idx),
                 lambda: sketch.sketch_compare_list(da, idx, idx[:3]), lambda: sketch.sketch_compare_list(da, idx, idx, da[:, :64].contiguous()),
                 lambda: sketch.sketch_compare_list(da, idx, idx, _dev(gpu, wide))):
        with pytest.raises(ValueError):
            call()


def test_whole_call_on_a_side_stream_feeds_the_clustering_calls(gpu):
    import torch
    from bioseq_amd import sketch
    a, _ = _store(300)
    want = sketch.lsh_pairs(a, rows_per_band=3)
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        da = _dev(gpu, a)
        row, col, match, _, offs = sketch.lsh_pairs(da, rows_per_band=3)
        labels = sketch.cluster_pairs(row, col, 300)
        rep = sketch.greedy_pairs(row, col, 300, weight=match)
    side.synchronize()
    assert row.cpu().numpy().tobytes() == want[0].tobytes() and offs.cpu().numpy().tobytes() == want[4].tobytes()
    assert labels.cpu().numpy().tobytes() == sketch.cluster_pairs(want[0], want[1], 300).tobytes()
    assert rep.cpu().numpy().tobytes() == sketch.greedy_pairs(want[0], want[1], 300, weight=want[2]).tobytes()
    assert labels[3] == 2 and labels[4] == 2 and rep[3] == 2 and rep[4] == 2
