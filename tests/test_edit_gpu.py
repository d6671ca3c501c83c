"""GPU: the edit distance of row pairs (bioseq_amd.align, bsq_edit_pairs_device) against the plain dynamic programme of
tests/edit_twin.py and the library's host twin, byte for byte: shorter sides at every block and group edge with four longer sides each,
a text much longer than a tile, every form on the pairs it holds, waves whose groups finish at different steps with guards around the
output, the codes, two stores and one, unmapped bytes, the Python surface on a side stream, and the pipeline from sketches to
exact-identity clusters."""
import ctypes
import functools

import numpy as np
import pytest

import edit_twin as twin

pytestmark = pytest.mark.gpu

LETTERS = {"DNA4": "ACGT", "AMINO20": "ACDEFGHIKLMNPQRSTVWY"}
EDGES = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096)


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _tok(key):
    import bioseq_amd
    return bioseq_amd.Tokenizer(key, False, False, False)


def _lut(tok):
    from bioseq_amd import capi
    d = capi.desc_of(tok)
    return np.array(list(d.lut), np.int64), d.nchars


def _device(gpu, tok, ca, oa, row, col, cb=None, ob=None, **kw):
    """edit_distance_pairs on uploaded copies, as a numpy array; the result is an int32 device tensor of the list's length."""
    import torch
    from bioseq_amd import align
    b = () if cb is None else (_dev(cb, gpu), _dev(ob, gpu))
    got = align.edit_distance_pairs(tok, _dev(ca, gpu), _dev(oa, gpu), _dev(row, gpu), _dev(col, gpu), *b, **kw)
    assert got.dtype == torch.int32 and got.device == gpu and got.is_contiguous() and tuple(got.shape) == (len(row),)
    return got.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _edges(key):
    """Every shorter side of EDGES against longer sides m, m + 1, m + 70 and 2 m + 3, unrelated and related: the stores, the list, the
    plain dynamic programme's answers (computed once per alphabet) and, per pair, (m, n, related)."""
    rng = np.random.default_rng(len(key))
    pairs, meta = [], []
    for m in EDGES:
        for n in (m, m + 1, m + 70, 2 * m + 3):
            pairs.append((twin.random_row(rng, m, LETTERS[key]), twin.random_row(rng, n, LETTERS[key])))
            pairs.append(twin.related_pair(rng, m, n, LETTERS[key]))
            meta += [(m, n, False), (m, n, True)]
    for k in range(1, len(pairs), 4):  # (the shorter side in store B as often as in store A)
        pairs[k] = pairs[k][::-1]
    ca, oa, cb, ob, row, col = twin.store_of(pairs)
    lut, nchars = _lut(_tok(key))
    return ca, oa, cb, ob, row, col, twin.edit_pairs(lut, nchars, ca, oa, cb, ob, row, col), meta


@pytest.mark.parametrize("key", ["DNA4", "AMINO20"])
def test_block_and_group_edges(gpu, bsq, key):
    """One block, a last block of 1, 63 and 64 rows, the first row of a second block, the last lane of every form and one past it."""
    from bioseq_amd import align
    ca, oa, cb, ob, row, col, exp, meta = _edges(key)
    for k, (m, n, related) in enumerate(meta):
        if related and m >= 63:
            assert 0 < exp[k] < n, (m, n)  # (not vacuous: neither equal rows nor a distance any alignment reaches)
    tok = _tok(key)
    assert align.edit_distance_host(tok, ca, oa, row, col, cb, ob).tobytes() == exp.tobytes(), "host twin"
    got = _device(gpu, tok, ca, oa, row, col, cb, ob)
    assert got.tobytes() == exp.tobytes(), [(meta[k], int(got[k]), int(exp[k])) for k in np.nonzero(got != exp)[0][:8]]


def test_long_text(gpu, bsq):
    """4096 x 20 001: 313 text tiles of 64 columns in the widest form; 1 x 20 001 and 0 x 20 001 in every form."""
    from bioseq_amd import align
    rng = np.random.default_rng(11)
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    short, long_ = twin.related_pair(rng, 4096, 20001, "ACGT")
    chars, offs = twin.pack([short, long_, np.frombuffer(b"G", np.uint8), np.zeros(0, np.uint8)])
    row, col = np.array([0, 1, 2, 1, 3, 1], np.int64), np.array([1, 0, 1, 2, 1, 3], np.int64)
    exp = twin.edit_pairs(lut, nchars, chars, offs, chars, offs, row, col)
    assert 0 < exp[0] < 20001 and exp[0] == exp[1] and exp[2] == 20000 and exp[4] == 20001
    assert align.edit_distance_host(tok, chars, offs, row, col).tobytes() == exp.tobytes()
    assert _device(gpu, tok, chars, offs, row, col).tobytes() == exp.tobytes()
    for form in (1, 2, 3):
        assert _device(gpu, tok, chars, offs, row[2:], col[2:], max_len=16, form=form).tobytes() == exp[2:].tobytes(), form


@pytest.mark.parametrize("key", ["DNA4", "AMINO20"])
def test_every_form_gives_one_result(gpu, bsq, key):
    from bioseq_amd import align
    ca, oa, cb, ob, row, col, exp, meta = _edges(key)
    tok = _tok(key)
    m = np.array([x[0] for x in meta])
    for max_len, forms in ((256, (None, 1, 2, 3)), (1024, (None, 2, 3))):
        sel = np.nonzero(m <= max_len)[0]
        for form in forms:
            got = _device(gpu, tok, ca, oa, row[sel], col[sel], cb, ob, max_len=max_len, form=form)
            assert got.tobytes() == exp[sel].tobytes(), (max_len, form)
    with pytest.raises(ValueError):
        align.edit_distance_pairs(tok, _dev(ca, gpu), _dev(oa, gpu), _dev(row, gpu), _dev(col, gpu), max_len=257, form=1)
    with pytest.raises(ValueError):
        align.edit_distance_pairs(tok, _dev(ca, gpu), _dev(oa, gpu), _dev(row, gpu), _dev(col, gpu), max_len=1025, form=2)


def test_ragged_waves_and_guards(gpu, bsq):
    """Form 1: sixteen pairs share a wave, lengths 0 .. 256 mixed, so the groups of a wave finish at different steps; lists that fill a
    wave, leave one ragged and spread over many workgroups, with repeated indices and pairs (i, i); guard words around dist stay."""
    import torch
    from bioseq_amd import capi
    L = capi.load()
    rng = np.random.default_rng(3)
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    lengths = [0, 1, 2, 63, 64, 65, 128, 255, 256] + rng.integers(0, 257, size=31).tolist()
    rows = [twin.random_row(rng, n, "ACGT") for n in lengths]
    rows += [twin.fit(rng, twin.mutate(rng, rows[k], "ACGT", 0.03), len(rows[k]) + k % 3, "ACGT") for k in range(3, 40, 4)]
    chars, offs = twin.pack(rows)
    B = len(rows)
    known = {}

    def reference(row, col):
        for i, j in zip(row.tolist(), col.tolist()):
            if (i, j) not in known:
                one = twin.edit_pairs(lut, nchars, chars, offs, chars, offs, [i], [j], max_len=256)
                known[(i, j)] = known[(j, i)] = int(one[0])
        return np.array([known[p] for p in zip(row.tolist(), col.tolist())], np.int32)

    dc, do = _dev(chars, gpu), _dev(offs, gpu)
    desc, e, guard = capi.desc_of(tok), capi.Edit(256, 1), 16
    for n_pairs in (1, 15, 17, 65, 1000):
        row, col = rng.integers(0, B, size=n_pairs), rng.integers(0, 40, size=n_pairs)  # (few columns: indices repeat)
        row[::7] = col[::7]  # pairs (i, i)
        exp = reference(row, col)
        assert (exp[::7] == 0).all() and (n_pairs < 17 or len(set(exp.tolist())) > 8)
        dist = torch.full((n_pairs + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
        dr, dl = _dev(row, gpu), _dev(col, gpu)
        with capi.launching(gpu) as stream:
            capi.check(L.bsq_edit_pairs_device(ctypes.byref(desc), dc.data_ptr(), do.data_ptr(), B, dc.data_ptr(), do.data_ptr(), B, dr.data_ptr(),
                                               dl.data_ptr(), n_pairs, ctypes.byref(e), dist.data_ptr() + 4 * guard, stream))
        raw = dist.cpu().numpy()
        assert (raw[:guard] == 0x5A5A5A5A).all() and (raw[-guard:] == 0x5A5A5A5A).all(), n_pairs
        assert raw[guard:-guard].tobytes() == exp.tobytes(), n_pairs


def test_codes(gpu, bsq):
    """A shorter side of max_len + 1 gets -1 between neighbours that stay correct, at max_len 100 and 4096; indices -1, Ba and 2^40 get
    -2 and are not followed; an empty list gives an empty tensor."""
    import torch
    from bioseq_amd import align
    rng = np.random.default_rng(5)
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    rows = [twin.random_row(rng, n, "ACGT") for n in (99, 100, 101, 300, 4095, 4096, 4097, 4200)]
    chars, offs = twin.pack(rows)
    for max_len, base in ((100, 0), (4096, 4)):
        row = np.array([base, base + 1, base + 2, base + 1, base + 2, base + 2, -1, 0, 8, 1 << 40, 0, base], np.int64)
        col = np.array([3 + base // 4 * 4, 3 + base // 4 * 4, 3 + base // 4 * 4, base + 1, base + 2, base, 0, 8, 8, 0, -(1 << 40), base + 1], np.int64)
        exp = twin.edit_pairs(lut, nchars, chars, offs, chars, offs, row, col, max_len=max_len)
        assert exp[0] > 0 and exp[1] > 0 and exp[2] == -1 and exp[3] == 0 and exp[4] == -1 and exp[5] > 0 and exp[6:11].tolist() == [-2] * 5 and exp[11] > 0
        assert align.edit_distance_host(tok, chars, offs, row, col, max_len=max_len).tobytes() == exp.tobytes()
        assert _device(gpu, tok, chars, offs, row, col, max_len=max_len).tobytes() == exp.tobytes(), max_len
    empty = torch.zeros(0, dtype=torch.int64, device=gpu)
    got = align.edit_distance_pairs(tok, _dev(chars, gpu), _dev(offs, gpu), empty, empty)
    assert got.dtype == torch.int32 and got.device == gpu and tuple(got.shape) == (0,)
    none = align.edit_distance_pairs(tok, torch.zeros(0, dtype=torch.uint8, device=gpu), torch.zeros(1, dtype=torch.int64, device=gpu),
                                     _dev(np.array([0, 1], np.int64), gpu), _dev(np.array([0, 0], np.int64), gpu), _dev(chars, gpu), _dev(offs, gpu))
    assert none.tolist() == [-2, -2]  # a store without rows


def test_two_stores_and_one_store(gpu, bsq):
    """A (23 rows) against B (37 rows) in a crossed list, the stores swapped, and one store against itself."""
    rng = np.random.default_rng(8)
    tok = _tok("AMINO20")
    lut, nchars = _lut(tok)
    letters = LETTERS["AMINO20"]
    ra = [twin.random_row(rng, n, letters) for n in rng.integers(0, 300, size=23)]
    rb = [twin.fit(rng, twin.mutate(rng, ra[k % 23], letters, 0.04), len(ra[k % 23]) + k % 5, letters) for k in range(37)]
    ca, oa = twin.pack(ra)
    cb, ob = twin.pack(rb)
    row, col = rng.integers(0, 23, size=200), rng.integers(0, 37, size=200)
    col[:60] = row[:60] + 23 * rng.integers(0, 2, size=60) * (row[:60] < 14)  # related pairs among them
    exp = twin.edit_pairs(lut, nchars, ca, oa, cb, ob, row, col)
    assert len(set(exp.tolist())) > 50
    assert _device(gpu, tok, ca, oa, row, col, cb, ob, max_len=512).tobytes() == exp.tobytes()
    assert _device(gpu, tok, cb, ob, col, row, ca, oa, max_len=512).tobytes() == exp.tobytes(), "the stores swapped"
    col = rng.integers(0, 23, size=200)
    exp = twin.edit_pairs(lut, nchars, ca, oa, ca, oa, row, col)
    assert _device(gpu, tok, ca, oa, row, col, max_len=512).tobytes() == exp.tobytes(), "one store"
    assert not _device(gpu, tok, ca, oa, row, row).any(), "dist(x, x)"


def test_unmapped_bytes(gpu, bsq):
    """N, '-', lower case and bytes >= 0x80 in DNA4: one unmapped class that matches itself and nothing else."""
    from bioseq_amd import align
    rng = np.random.default_rng(13)
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    pool = np.frombuffer(b"ACGTacgtNNn--\x80\xc3\xff", np.uint8)
    rows = [pool[rng.integers(0, pool.size, size=n)] for n in (5, 64, 65, 130, 200, 257, 300)]
    rows += [np.frombuffer(b"ACNNGT", np.uint8), np.frombuffer(b"ac-\xffgt", np.uint8), np.frombuffer(b"ACANGT", np.uint8)]
    chars, offs = twin.pack(rows)
    row, col = [a.ravel().astype(np.int64) for a in np.meshgrid(np.arange(10), np.arange(10), indexing="ij")]
    exp = twin.edit_pairs(lut, nchars, chars, offs, chars, offs, row, col)
    assert exp[7 * 10 + 8] == 0 and exp[7 * 10 + 9] == 1 and not exp[::11].any()
    assert align.edit_distance_host(tok, chars, offs, row, col).tobytes() == exp.tobytes()
    assert _device(gpu, tok, chars, offs, row, col).tobytes() == exp.tobytes()
    assert _device(gpu, tok, chars, offs, row, col, max_len=300, form=2).tobytes() == exp.tobytes()


def test_surface_on_a_side_stream(gpu, bsq):
    """verify_pairs == verify_pairs_host, pair_lengths, pair_identity against float64, the kernel names, and a call on a stream that is
    not the default one."""
    import torch
    from bioseq_amd import align
    rng = np.random.default_rng(21)
    tok = _tok("DNA4")
    rows = [twin.random_row(rng, n, "ACGT") for n in (150, 150, 0, 0, 90, 700)]
    rows += [twin.fit(rng, twin.mutate(rng, rows[0], "ACGT", rate), 150, "ACGT") for rate in (0.0, 0.01, 0.02, 0.03, 0.05, 0.08)]
    chars, offs = twin.pack(rows)
    row = np.array([0, 0, 0, 0, 0, 0, 0, 2, 2, 4, 5, 5, -1, 0], np.int64)
    col = np.array([6, 7, 8, 9, 10, 11, 1, 3, 0, 5, 5, 0, 0, 12], np.int64)
    keep_h, dist_h = align.verify_pairs_host(tok, chars, offs, row, col, min_identity=0.9, max_len=600)
    assert keep_h[0] and keep_h[7] and not keep_h[6] and dist_h[10] == -1 and dist_h[-2:].tolist() == [-2, -2] and 0 < keep_h[:6].sum() < 6
    dc, do, dr, dl = _dev(chars, gpu), _dev(offs, gpu), _dev(row, gpu), _dev(col, gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        keep, dist = align.verify_pairs(tok, dc, do, dr, dl, min_identity=0.9, max_len=600)
    side.synchronize()
    assert keep.dtype == torch.bool and dist.dtype == torch.int32 and keep.device == gpu
    assert dist.cpu().numpy().tobytes() == dist_h.tobytes() and keep.cpu().numpy().tobytes() == keep_h.tobytes()
    for T in (0.0, 0.5, 0.95, 1.0):
        assert align.verify_pairs(tok, dc, do, dr, dl, min_identity=T, max_len=600)[0].cpu().numpy().tobytes() == \
            align.verify_pairs_host(tok, chars, offs, row, col, min_identity=T, max_len=600)[0].tobytes(), T
    la, lb = align.pair_lengths(do, dr[:12], None, dl[:12])
    lens = np.diff(offs)
    assert la.tolist() == lens[row[:12]].tolist() and lb.tolist() == lens[col[:12]].tolist()
    ident = align.pair_identity(dist[:12], la, lb)
    assert ident.dtype == torch.float32 and ident.device == gpu
    d64, L64 = dist_h[:12].astype(np.float64), np.maximum(lens[row[:12]], lens[col[:12]]).astype(np.float64)
    want = np.where(L64 > 0, 1.0 - d64 / np.maximum(L64, 1.0), 1.0)
    got = ident.cpu().numpy().astype(np.float64)
    ok = dist_h[:12] >= 0
    assert np.isnan(got[~ok]).all() and (~ok).sum() == 1 and np.abs(got[ok] - want[ok]).max() <= 1e-6 and got[7] == 1.0
    assert [align.edit_kernel_name(m) for m in (100, 600, 4096)] == ["k_edit_pairs<4>", "k_edit_pairs<16>", "k_edit_pairs<64>"]
    assert align.edit_kernel_name(100, form=3) == "k_edit_pairs<64>" and align.edit_kernel_name(257, form=1) == ""
    with pytest.raises(ValueError):
        align.edit_distance_pairs(tok, chars, offs, row, col)  # numpy arrays are the host twin's
    with pytest.raises(ValueError):
        align.edit_distance_pairs(tok, dc, do, dr.to(torch.int32), dl)
    for bad_row, bad_col in ((torch.stack([dr, dr], 1)[:, 0], dl), (dr, dl[:-1])):  # a row that is not contiguous; two lengths
        with pytest.raises(ValueError):
            align.edit_distance_pairs(tok, dc, do, bad_row, bad_col)
    with pytest.raises(ValueError):
        align.verify_pairs(tok, dc, do, dr, dl, min_identity=1.1)


def test_sketches_to_exact_identity_clusters(gpu, bsq):
    """300 reads of 150 characters, 20 of them mutated copies (substitution, insertion and deletion at 4 % each) of earlier reads:
    minhash_packed -> sketch_pairs(0.2) -> verify_pairs(0.9) -> cluster_pairs gives the labels that the plain dynamic programme gives
    over the same candidates; the seed is one at which candidates are both kept and rejected."""
    from bioseq_amd import align, sketch
    rng = np.random.default_rng(2)
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    rows = [twin.random_row(rng, 150, "ACGT") for _ in range(280)]
    rows += [twin.fit(rng, twin.mutate(rng, rows[7 * k], "ACGT", 0.04), 150, "ACGT") for k in range(20)]
    chars, offs = twin.pack(rows)
    dc, do = _dev(chars, gpu), _dev(offs, gpu)
    sk = sketch.minhash_packed(tok, dc, do, 8, 256)
    row, col, *_ = sketch.sketch_pairs(sk, min_jaccard=0.2)
    keep, dist = align.verify_pairs(tok, dc, do, row, col, min_identity=0.9, max_len=150)
    labels = sketch.cluster_pairs(row[keep].contiguous(), col[keep].contiguous(), 300)
    r, c = row.cpu().numpy(), col.cpu().numpy()
    exp = twin.edit_pairs(lut, nchars, chars, offs, chars, offs, r, c, max_len=150)
    passed = twin.passes(exp, np.full(r.size, 150), np.full(r.size, 150), 0.9)
    assert dist.cpu().numpy().tobytes() == exp.tobytes() and keep.cpu().numpy().tobytes() == passed.tobytes()
    assert passed.any() and not passed.all(), "a candidate kept and a candidate rejected"
    want = sketch.cluster_pairs_host(r[passed], c[passed], 300)
    assert labels.cpu().numpy().tobytes() == want.tobytes() and 0 < (want != np.arange(300)).sum() <= 20
