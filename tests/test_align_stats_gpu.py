"""GPU: the alignment statistics of row pairs (bioseq_amd.align, bsq_align_stats_device) against the library's host twin, bit for bit,
and on small cases against the cell-by-cell programme of tests/align_stats_twin.py: pattern lengths at every lane and form edge, text
lengths at the tile edges, forced forms, waves that mix orientations, empty rows and codes with guards around both outputs, alignments
that cross a lane's 32-row boundary, lists full of ties in every form, both packed fields at the top of their range, a start beyond
text column 65 536, two stores, a side stream, the verification rule and the pipeline from sketches to identity / coverage clusters.
Then against the anti-diagonal sweep of the same module, which shares nothing with the library, at full length: related pairs of up to
2048 x 2110 with gaps all along them, gaps planted where lanes 17, 40 and 63 begin, 2048 x 4500, two-letter rows of 2048 under gaps
that cost little or nothing, the ends of the scoring ranges, and the three pair-walk families against each other."""
import ctypes
import functools

import numpy as np
import pytest

import align_stats_twin as twin

pytestmark = pytest.mark.gpu

LETTERS = {"DNA4": "ACGT", "AMINO20": "ACDEFGHIKLMNPQRSTVWY"}
MODES = ("local", "global")
EDGES = {128: (1, 31, 32, 33, 63, 64, 65, 127, 128), 512: (129, 511, 512), 2048: (513,)}  # max_len (form 1, 2, 3): pattern lengths


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


@functools.lru_cache(maxsize=None)
def _scoring(key):
    from bioseq_amd import align
    tok = _tok(key)
    return (align.blosum62_matrix(tok), 11, 1) if key == "AMINO20" else (align.score_matrix(tok, 2, -3), 5, 2)


def _device(gpu, tok, ca, oa, row, col, cb=None, ob=None, **kw):
    """stats_pairs on uploaded copies, as numpy arrays (score, stats); int32 device tensors of the list's length."""
    import torch
    from bioseq_amd import align
    b = () if cb is None else (_dev(cb, gpu), _dev(ob, gpu))
    s, st = align.stats_pairs(tok, _dev(ca, gpu), _dev(oa, gpu), _dev(row, gpu), _dev(col, gpu), *b, **kw)
    assert s.dtype == torch.int32 and s.device == gpu and s.is_contiguous() and tuple(s.shape) == (len(row),)
    assert st.dtype == torch.int32 and st.device == gpu and st.is_contiguous() and tuple(st.shape) == (len(row), 6)
    return s.cpu().numpy(), st.cpu().numpy()


def _same(got, exp, meta=None):
    (gs, gt), (es, et) = got, exp
    bad = np.nonzero((gs != es) | (gt != et).any(axis=1))[0]
    assert bad.size == 0, [(meta[k] if meta else k, int(gs[k]), gt[k].tolist(), int(es[k]), et[k].tolist()) for k in bad[:6]]
    assert gs.tobytes() == es.tobytes() and gt.tobytes() == et.tobytes()


@functools.lru_cache(maxsize=None)
def _edge_pairs(key, max_len):
    """Every pattern length of EDGES[max_len] against texts of m, m + 1 and m + 37 characters, unrelated and related (mutated at 6 %), the
    shorter side in store B as often as in store A."""
    rng = np.random.default_rng(len(key) + max_len)
    pairs, meta = [], []
    for m in EDGES[max_len]:
        for n in (m, m + 1, m + 37):
            pairs.append((twin.random_row(rng, m, LETTERS[key]), twin.random_row(rng, n, LETTERS[key])))
            pairs.append(twin.related_pair(rng, m, n, LETTERS[key], rate=0.06))
            meta += [(m, n, False), (m, n, True)]
    for k in range(1, len(pairs), 4):
        pairs[k] = pairs[k][::-1]
    return pairs, meta


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ["DNA4", "AMINO20"])
def test_lane_and_form_edges(gpu, bsq, key, mode):
    """One lane, a last lane of 1, 31 and 32 rows, the first row of a second lane, the last lane of every form and the first pattern
    beyond it; patterns of up to 65 rows also against the Python programme."""
    from bioseq_amd import align
    tok = _tok(key)
    lut, nchars = _lut(tok)
    S, o, e = _scoring(key)
    kw = dict(matrix=S, gap_open=o, gap_extend=e, mode=mode)
    for max_len in EDGES:
        pairs, meta = _edge_pairs(key, max_len)
        ca, oa, cb, ob, row, col = twin.store_of(pairs)
        exp = align.stats_pairs_host(tok, ca, oa, row, col, cb, ob, max_len=max_len, **kw)
        if mode == "local":
            related = np.array([m[2] and m[0] >= 31 for m in meta])
            assert (exp[1][related, 4] > np.array([m[0] for m in meta])[related] // 2).all()  # (not vacuous: long alignments)
        assert align.stats_kernel_name(mode=mode, max_len=max_len) == "k_align_stats<%d, %s>" % ({128: 4, 512: 16, 2048: 64}[max_len], mode)
        _same(_device(gpu, tok, ca, oa, row, col, cb, ob, max_len=max_len, **kw), exp, meta)
        if max_len == 128:
            small = np.nonzero(np.array([m[0] for m in meta]) <= 65)[0]
            py = twin.stats_pairs(lut, nchars, ca, oa, cb, ob, row[small], col[small], S, o, e, mode)
            _same((exp[0][small], exp[1][small]), py, [meta[k] for k in small])


@pytest.mark.parametrize("form", [1, 2, 3])
def test_text_tile_edges_and_forced_forms(gpu, bsq, form):
    """Texts of G - 1, G, G + 1 and 2 G + 1 characters against patterns of 1 .. 3 (the text arrives G bytes at a time), and patterns of up to
    200 rows in the forms that are wider than they need: the result does not depend on the form."""
    from bioseq_amd import align
    rng = np.random.default_rng(40 + form)
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    S, o, e = _scoring("DNA4")
    G = 4 ** form
    pairs = []
    for n in (G - 1, G, G + 1, 2 * G + 1):
        for m in (1, 2, 3):
            x = twin.random_row(rng, n, "ACGT")
            pairs += [(x[n - m:].copy(), x), (x, x[:m].copy()), (twin.random_row(rng, m, "ACGT"), x)]
    longest = {1: 128, 2: 200, 3: 200}[form]
    for m in (31, 33, 64, 100, longest):
        pairs.append(twin.related_pair(rng, m, m + 30, "ACGT", rate=0.08))
        pairs.append(twin.related_pair(rng, m, m + 5, "ACGT", rate=0.2)[::-1])
    ca, oa, cb, ob, row, col = twin.store_of(pairs)
    for mode in MODES:
        kw = dict(matrix=S, gap_open=o, gap_extend=e, mode=mode)
        exp = align.stats_pairs_host(tok, ca, oa, row, col, cb, ob, max_len=longest, **kw)
        assert align.stats_kernel_name(mode=mode, max_len=longest, form=form) == "k_align_stats<%d, %s>" % (G, mode)
        _same(_device(gpu, tok, ca, oa, row, col, cb, ob, max_len=longest, form=form, **kw), exp)
        py = twin.stats_pairs(lut, nchars, ca, oa, cb, ob, row[:36], col[:36], S, o, e, mode)
        _same((exp[0][:36], exp[1][:36]), py)
    with pytest.raises(ValueError):
        align.stats_pairs(tok, _dev(ca, gpu), _dev(oa, gpu), _dev(row, gpu), _dev(col, gpu), matrix=S, gap_open=o, gap_extend=e, max_len=129, form=1)
    with pytest.raises(ValueError):
        align.stats_pairs(tok, _dev(ca, gpu), _dev(oa, gpu), _dev(row, gpu), _dev(col, gpu), matrix=S, gap_open=o, gap_extend=e, max_len=2049)


def test_mixed_waves_and_guards(gpu, bsq):
    """Form 1: sixteen pairs share a wave -- both orientations, empty rows, indices outside the stores and rows beyond max_len side by
    side, groups that finish at different steps; lists that fill a wave, leave one ragged and spread over many workgroups, through the
    C ABI with guard words around score and stats."""
    import torch
    from bioseq_amd import align, capi
    L = capi.load()
    rng = np.random.default_rng(3)
    tok = _tok("DNA4")
    S, o, e = _scoring("DNA4")
    lengths = [0, 1, 2, 31, 32, 33, 64, 127, 128, 129, 300, 0] + rng.integers(0, 129, size=8).tolist()
    rows = [twin.random_row(rng, n, "ACGT") for n in lengths]
    rows += [twin.fit(rng, twin.mutate(rng, rows[k], "ACGT", 0.05), len(rows[k]) + k % 3, "ACGT") for k in range(3, 9)]
    chars, offs = twin.pack(rows)
    B = len(rows)
    dc, do = _dev(chars, gpu), _dev(offs, gpu)
    desc, guard = capi.desc_of(tok), 16
    for mode in (0, 1):
        sc = capi.Score(128, 1, mode, o, e)
        np.ctypeslib.as_array(sc.matrix)[:5, :5] = S
        for n_pairs in (1, 15, 17, 65, 1000):
            row, col = rng.integers(-1, B + 1, size=n_pairs), rng.integers(-1, B + 1, size=n_pairs)
            row[::7] = col[::7]  # pairs (i, i)
            exp_s, exp_t = align.stats_pairs_host(tok, chars, offs, row, col, matrix=S, gap_open=o, gap_extend=e, mode=MODES[mode], max_len=128)
            if n_pairs == 1000:
                assert (exp_s == twin.TOO_LONG).any() and (exp_s == twin.BAD_INDEX).any() and len(set(exp_s.tolist())) > 30
            dr, dl = _dev(row, gpu), _dev(col, gpu)
            score = torch.full((n_pairs + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
            stats = torch.full((6 * n_pairs + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
            with capi.launching(gpu) as stream:
                capi.check(L.bsq_align_stats_device(ctypes.byref(desc), dc.data_ptr(), do.data_ptr(), B, dc.data_ptr(), do.data_ptr(), B, dr.data_ptr(),
                                                    dl.data_ptr(), n_pairs, ctypes.byref(sc), score.data_ptr() + 4 * guard,
                                                    stats.data_ptr() + 4 * guard, stream))
            raw, raw_t = score.cpu().numpy(), stats.cpu().numpy()
            assert (raw[:guard] == 0x5A5A5A5A).all() and (raw[-guard:] == 0x5A5A5A5A).all(), n_pairs
            assert (raw_t[:guard] == 0x5A5A5A5A).all() and (raw_t[-guard:] == 0x5A5A5A5A).all(), n_pairs
            _same((raw[guard:-guard], raw_t[guard:-guard].reshape(-1, 6)), (exp_s, exp_t))
    # a refusal writes nothing and launches nothing
    sc = capi.Score(2049, 0, 0, o, e)
    score = torch.full((4,), 7, dtype=torch.int32, device=gpu)
    stats = torch.full((24,), 7, dtype=torch.int32, device=gpu)
    with capi.launching(gpu) as stream:
        st = L.bsq_align_stats_device(ctypes.byref(desc), dc.data_ptr(), do.data_ptr(), B, dc.data_ptr(), do.data_ptr(), B, dr.data_ptr(), dl.data_ptr(), 4,
                                      ctypes.byref(sc), score.data_ptr(), stats.data_ptr(), stream)
    assert st == 2 and (score.cpu().numpy() == 7).all() and (stats.cpu().numpy() == 7).all()
    empty = torch.zeros(0, dtype=torch.int64, device=gpu)
    s, t = align.stats_pairs(tok, dc, do, empty, empty, matrix=S, gap_open=o, gap_extend=e)
    assert tuple(s.shape) == (0,) and tuple(t.shape) == (0, 6) and t.dtype == torch.int32


def test_alignments_across_a_lane_boundary(gpu, bsq):
    """A core planted in poly-P (pattern) and poly-W (text) so that it starts in one lane's rows and ends in another's, once whole and
    once with three characters of the text's copy cut out where the pattern crosses row 32: the planted start and end, the gap's columns."""
    from bioseq_amd import align
    rng = np.random.default_rng(8)
    tok = _tok("AMINO20")
    lut, nchars = _lut(tok)
    S, o, e = _scoring("AMINO20")
    core_letters = LETTERS["AMINO20"].replace("P", "").replace("W", "")
    pairs, want = [], []
    for before, n, after, lead in ((20, 24, 10, 50), (31, 2, 40, 0), (0, 70, 3, 7), (60, 40, 20, 100)):
        core = twin.random_row(rng, n, core_letters)
        pat = np.concatenate([np.full(before, ord("P"), np.uint8), core, np.full(after, ord("P"), np.uint8)])
        text = np.concatenate([np.full(lead, ord("W"), np.uint8), core, np.full(90, ord("W"), np.uint8)])
        pairs += [(pat, text), (text, pat)]
        want += [[before, lead, before + n, lead + n, n, n], [lead, before, lead + n, before + n, n, n]]
    core = twin.random_row(rng, 40, core_letters)  # rows 13 .. 52 of the pattern; the text lacks the characters of rows 31 .. 33
    pat = np.concatenate([np.full(12, ord("P"), np.uint8), core, np.full(5, ord("P"), np.uint8)])
    text = np.concatenate([np.full(30, ord("W"), np.uint8), core[:18], core[21:], np.full(60, ord("W"), np.uint8)])
    pairs += [(pat, text), (text, pat)]
    want += [[12, 30, 52, 67, 37, 40], [30, 12, 67, 52, 37, 40]]
    ca, oa, cb, ob, row, col = twin.store_of(pairs)
    kw = dict(matrix=S, gap_open=o, gap_extend=e)
    py = twin.stats_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, o, e, "local")
    assert py[1].tolist() == want
    for form in (1, 2, 3):
        _same(_device(gpu, tok, ca, oa, row, col, cb, ob, max_len=128, form=form, **kw), py)
    exp = align.stats_pairs_host(tok, ca, oa, row, col, cb, ob, mode="global", **kw)
    _same(_device(gpu, tok, ca, oa, row, col, cb, ob, mode="global", max_len=128, **kw), exp)


@functools.lru_cache(maxsize=None)
def _tie_case(mode, gaps):
    """250 pairs of up to 40 x 60 over two letters, +1 / -1: the stores, the list and the Python programme's answers."""
    from bioseq_amd import align
    rng = np.random.default_rng(17)
    pairs = []
    for k in range(250):
        m, n = int(rng.integers(0, 41)), int(rng.integers(0, 61))
        n = m if k % 10 == 0 else n
        x, y = twin.random_row(rng, m, "AC"), twin.random_row(rng, n, "AC")
        pairs.append((x, y) if k % 2 else (y, x))
    ca, oa, cb, ob, row, col = twin.store_of(pairs)
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    S = align.score_matrix(tok, 1, -1)
    return ca, oa, cb, ob, row, col, S, twin.stats_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, gaps[0], gaps[1], mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", [(0, 1), (1, 1), (3, 0), (0, 0)])
def test_ties_in_every_form(gpu, bsq, mode, gaps):
    """Most cells tie between the diagonal and a gap or between the two gaps, and the tie between the gaps is in A / B terms: a wave holds
    pairs of both orientations."""
    ca, oa, cb, ob, row, col, S, exp = _tie_case(mode, gaps)
    tok = _tok("DNA4")
    for form in (1, 2, 3):
        _same(_device(gpu, tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=gaps[0], gap_extend=gaps[1], mode=mode, max_len=64, form=form), exp)


def test_fields_at_the_top_of_their_range(gpu, bsq):
    """2048 x 2048, a row against itself: matches and diag reach 2048 (13 bits each).  40 x 70 000 with the core planted beyond text column
    65 536, in both store orders: the text-side start needs more than 16 bits, the pattern-side start sits above it."""
    from bioseq_amd import align
    rng = np.random.default_rng(12)
    tok = _tok("AMINO20")
    S, o, e = _scoring("AMINO20")
    kw = dict(matrix=S, gap_open=o, gap_extend=e)
    letters = LETTERS["AMINO20"].replace("P", "")
    whole = twin.random_row(rng, 2048, letters)
    core = twin.random_row(rng, 30, letters)
    pat = np.concatenate([np.full(7, ord("P"), np.uint8), core, np.full(3, ord("P"), np.uint8)])
    text = np.concatenate([np.full(66000, ord("W"), np.uint8), core, np.full(70000 - 66030, ord("W"), np.uint8)])
    chars, offs = twin.pack([whole, pat, text])
    row, col = np.array([0, 1, 2], np.int64), np.array([0, 2, 1], np.int64)
    for mode in MODES:
        exp = align.stats_pairs_host(tok, chars, offs, row, col, mode=mode, **kw)
        assert exp[1][0].tolist() == [0, 0, 2048, 2048, 2048, 2048]
        if mode == "local":
            assert exp[1][1:].tolist() == [[7, 66000, 37, 66030, 30, 30], [66000, 7, 66030, 37, 30, 30]]
        _same(_device(gpu, tok, chars, offs, row, col, mode=mode, **kw), exp)


def test_surface_on_a_side_stream(gpu, bsq):
    """verify_align_pairs == verify_align_pairs_host on a stream that is not the default one, with one store and with two, over the
    options; stats_identity and stats_coverage on device tensors; what the device call refuses."""
    import torch
    from bioseq_amd import align
    rng = np.random.default_rng(21)
    tok = _tok("AMINO20")
    S, o, e = _scoring("AMINO20")
    letters = LETTERS["AMINO20"]
    rows = [twin.random_row(rng, n, letters) for n in (150, 150, 0, 0, 90, 700)]
    rows += [twin.fit(rng, twin.mutate(rng, rows[0], letters, rate), n, letters) for rate, n in ((0.0, 150), (0.02, 150), (0.05, 140), (0.1, 160), (0.2, 150), (0.3, 150))]
    rows.append(rows[0][30:110].copy())
    chars, offs = twin.pack(rows)
    row = np.array([0, 0, 0, 0, 0, 0, 0, 2, 2, 4, 5, 5, -1, 0, 12, 0, 12], np.int64)
    col = np.array([6, 7, 8, 9, 10, 11, 1, 3, 0, 5, 5, 0, 0, 13, 0, 12, 12], np.int64)
    kw = dict(matrix=S, gap_open=o, gap_extend=e, max_len=600)
    keep_h, score_h, stats_h = align.verify_align_pairs_host(tok, chars, offs, row, col, min_identity=0.85, **kw)
    lengths = np.diff(offs)
    la, lb = lengths[np.clip(row, 0, 12)], lengths[np.clip(col, 0, 12)]
    assert keep_h.tolist() == twin.keeps(score_h, stats_h, la, lb, min_identity=0.85).tolist()
    assert keep_h[0] and 0 < keep_h[:6].sum() < 6 and not keep_h[14] and score_h[10] == twin.TOO_LONG and score_h[12:14].tolist() == [twin.BAD_INDEX] * 2
    dc, do, dr, dl = _dev(chars, gpu), _dev(offs, gpu), _dev(row, gpu), _dev(col, gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        keep, score, stats = align.verify_align_pairs(tok, dc, do, dr, dl, min_identity=0.85, **kw)
    side.synchronize()
    assert keep.dtype == torch.bool and score.dtype == torch.int32 and stats.dtype == torch.int32 and keep.device == gpu and tuple(stats.shape) == (17, 6)
    assert score.cpu().numpy().tobytes() == score_h.tobytes() and stats.cpu().numpy().tobytes() == stats_h.tobytes()
    assert keep.cpu().numpy().tobytes() == keep_h.tobytes()
    for opts in (dict(min_identity=0.5, min_coverage=0.5), dict(identity_over="shorter"), dict(coverage="shorter", min_coverage=0.9),
                 dict(coverage="longer", min_coverage=0.5), dict(coverage="a", min_coverage=0.5), dict(coverage="b", min_coverage=0.5),
                 dict(min_identity=0.0, min_coverage=0.0, min_score=300), dict(min_identity=1.0, min_coverage=1.0)):
        for mode in MODES:
            a = align.verify_align_pairs(tok, dc, do, dr, dl, mode=mode, **opts, **kw)[0].cpu().numpy()
            b = align.verify_align_pairs_host(tok, chars, offs, row, col, mode=mode, **opts, **kw)[0]
            assert a.tobytes() == b.tobytes(), (opts, mode)
    two = align.verify_align_pairs(tok, dc, do, dr[:12], dl[:12], dc, do, min_identity=0.85, **kw)
    assert two[0].cpu().numpy().tobytes() == keep_h[:12].tobytes() and two[2].cpu().numpy().tobytes() == stats_h[:12].tobytes(), "two stores"
    dla, dlb = _dev(la, gpu), _dev(lb, gpu)
    for over in ("columns", "shorter", "longer"):
        a, b = align.stats_identity(stats, over, dla, dlb), align.stats_identity(stats_h, over, la, lb)
        assert a.dtype == torch.float32 and a.device == gpu and np.array_equal(a.cpu().numpy(), b, equal_nan=True), over
    (ca_, cb_), (ha, hb) = align.stats_coverage(stats, dla, dlb), align.stats_coverage(stats_h, la, lb)
    assert np.array_equal(ca_.cpu().numpy(), ha, equal_nan=True) and np.array_equal(cb_.cpu().numpy(), hb, equal_nan=True) and ha[0] == 1 and np.isnan(ha[12])
    with pytest.raises(ValueError):
        align.stats_pairs(tok, chars, offs, row, col, **kw)  # numpy arrays are the host twin's
    with pytest.raises(ValueError):
        align.stats_pairs(tok, dc, do, dr.to(torch.int32), dl, **kw)
    for bad_row, bad_col in ((torch.stack([dr, dr], 1)[:, 0], dl), (dr, dl[:-1])):  # a row that is not contiguous; two lengths
        with pytest.raises(ValueError):
            align.stats_pairs(tok, dc, do, bad_row, bad_col, **kw)
    with pytest.raises(ValueError):
        align.stats_pairs(tok, dc, do, dr, dl, matrix=S, gap_open=128, gap_extend=1)
    with pytest.raises(ValueError):
        align.verify_align_pairs(tok, dc, do, dr, dl, min_coverage=1.1, **kw)


@functools.lru_cache(maxsize=None)
def _family_rows():
    """300 AMINO20 rows: 240 unrelated ones of 120 residues, then 20 families planted on rows 0, 7, 14, ...: a mutated whole copy (kept: high
    identity and coverage), a mutated copy of the middle third (high identity, low coverage of the longer row) and a heavily mutated copy."""
    rng = np.random.default_rng(6)
    letters = LETTERS["AMINO20"]
    rows = [twin.random_row(rng, 120, letters) for _ in range(240)]
    for k in range(20):
        head = rows[7 * k]
        rows.append(twin.fit(rng, twin.mutate(rng, head, letters, 0.05), 120, letters))
        rows.append(np.concatenate([twin.random_row(rng, 40, letters), twin.mutate(rng, head[40:80], letters, 0.03), twin.random_row(rng, 40, letters)]))
        rows.append(twin.fit(rng, twin.mutate(rng, head, letters, 0.3), 120, letters))
    return twin.pack(rows)


def test_sketches_to_identity_and_coverage_clusters(gpu, bsq):
    """minhash_packed -> sketch_pairs(low threshold) -> verify_align_pairs -> cluster_pairs gives the labels the host path gives over the
    same candidates, with candidates kept and candidates rejected -- by identity and by coverage."""
    from bioseq_amd import align, sketch
    tok = _tok("AMINO20")
    S, o, e = _scoring("AMINO20")
    chars, offs = _family_rows()
    dc, do = _dev(chars, gpu), _dev(offs, gpu)
    sk = sketch.minhash_packed(tok, dc, do, 3, 128)
    row, col, *_ = sketch.sketch_pairs(sk, min_jaccard=0.03)
    kw = dict(matrix=S, gap_open=o, gap_extend=e, min_identity=0.8, min_coverage=0.8, max_len=200)
    keep, score, stats = align.verify_align_pairs(tok, dc, do, row, col, **kw)
    labels = sketch.cluster_pairs(row[keep].contiguous(), col[keep].contiguous(), 300)
    r, c = row.cpu().numpy(), col.cpu().numpy()
    keep_h, score_h, stats_h = align.verify_align_pairs_host(tok, chars, offs, r, c, **kw)
    assert score.cpu().numpy().tobytes() == score_h.tobytes() and stats.cpu().numpy().tobytes() == stats_h.tobytes()
    assert keep.cpu().numpy().tobytes() == keep_h.tobytes()
    lengths = np.diff(offs)
    assert keep_h.tolist() == twin.keeps(score_h, stats_h, lengths[r], lengths[c], min_identity=0.8, min_coverage=0.8).tolist()
    by_identity = twin.keeps(score_h, stats_h, lengths[r], lengths[c], min_identity=0.8, min_coverage=0.0)
    assert keep_h.any() and (by_identity & ~keep_h).any() and (~by_identity).any(), "kept, rejected by coverage, rejected by identity"
    want = sketch.cluster_pairs_host(r[keep_h], c[keep_h], 300)
    assert labels.cpu().numpy().tobytes() == want.tobytes() and 10 <= (want != np.arange(300)).sum() <= 40


# ---- against the anti-diagonal sweep of tests/align_stats_twin.py (align_stats_diag), which shares nothing with the library: patterns of
# ---- full length, where lanes 17 .. 63 of k_align_stats<64, *> carry real alignments -- gaps, ties and tuples taken from E and F

FULL_SIZES = ((545, 600), (1300, 1301), (2047, 2110), (2048, 2048))


def _sweep(key_or_tok, stores, S, o, e, mode, counts=None, **kw):
    tok = _tok(key_or_tok) if isinstance(key_or_tok, str) else key_or_tok
    lut, nchars = _lut(tok)
    ca, oa, cb, ob, row, col = stores
    return twin.stats_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, o, e, mode, one=twin.align_stats_diag, counts=counts, **kw)


def _without_runs(x, lanes, length=3):
    """x without `length` characters from row 32 k - 1 on (1-based) for every k of `lanes`: aligned with x, the gap that bridges such a
    run opens in the last rows of lane k - 1 and is extended into the first row of lane k, so lane k continues an F state, and the
    tuple beside it, that it did not open."""
    keep = np.ones(x.size, bool)
    for k in lanes:
        keep[32 * k - 2:32 * k - 2 + length] = False
    return x[keep]


@functools.lru_cache(maxsize=None)
def _full_pairs(key):
    """Ten pairs, three workgroups of the widest form: related pairs (6 %) of every size of FULL_SIZES, one unrelated 2048 x 2048 pair, the
    three sizes with unequal sides once more, and two 2048 x 2110 pairs whose longer row is a mutated copy (6 %) of the shorter one
    without three characters at every fourth lane boundary; every second pair has the shorter side in store B.  meta: (m, n, related)."""
    rng = np.random.default_rng(len(key) + 70)
    letters = LETTERS[key]
    sizes = [s + (True,) for s in FULL_SIZES] + [(2048, 2048, False), (2047, 2110, True), (1300, 1301, True), (545, 600, True)]
    sizes += [(2048, 2110, "runs"), (2048, 2110, "runs")]
    pairs = []
    for k, (m, n, related) in enumerate(sizes):
        if related == "runs":
            x = twin.random_row(rng, m, letters)
            p = (x, twin.fit(rng, twin.mutate(rng, _without_runs(x, range(2 + k % 2, 64, 4)), letters, 0.06), n, letters))
        elif related:
            p = twin.related_pair(rng, m, n, letters, rate=0.06)
        else:
            p = (twin.random_row(rng, m, letters), twin.random_row(rng, n, letters))
        pairs.append(p[::-1] if k % 2 else p)
    return twin.store_of(pairs), sizes


@functools.lru_cache(maxsize=None)
def _full_case(key, mode):
    """The stores and list of _full_pairs, and the sweep's answers under the key's scoring (once per alphabet and mode)."""
    stores, meta = _full_pairs(key)
    return stores, meta, _sweep(key, stores, *_scoring(key), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ["DNA4", "AMINO20"])
def test_full_length_patterns_against_the_sweep(gpu, bsq, key, mode):
    """Patterns of 545 .. 2048 rows with insertions, deletions and substitutions all along them: every lane of the widest form carries H, F
    and tuples that came through gaps, and the best cell sits in the top lanes.  The 545-row pairs also with max_len = 545."""
    from bioseq_amd import align
    stores, meta, exp = _full_case(key, mode)
    ca, oa, cb, ob, row, col = stores
    tok = _tok(key)
    S, o, e = _scoring(key)
    kw = dict(matrix=S, gap_open=o, gap_extend=e, mode=mode)
    if mode == "local":  # not vacuous, from the reference alone: the alignment runs from the first lane to the last one and has gaps
        for k, (m, n, related) in enumerate(meta):
            if related:
                sa, sb, ea, eb, matches, columns = exp[1][k].tolist()
                start, end = (sb, eb) if k % 2 and m < n else (sa, ea)  # (on the pattern's side)
                assert start < 32 and end > m - 32 and columns - ((ea - sa) + (eb - sb) - columns) >= 20, (k, m, n, exp[1][k].tolist())
    assert align.stats_kernel_name(mode=mode, max_len=2048) == align.stats_kernel_name(mode=mode, max_len=545) == "k_align_stats<64, %s>" % mode
    _same(_device(gpu, tok, ca, oa, row, col, cb, ob, max_len=2048, **kw), exp, meta)
    small = np.array([k for k, s in enumerate(meta) if s[0] == 545], np.int64)
    _same(_device(gpu, tok, ca, oa, row[small], col[small], cb, ob, max_len=545, **kw), (exp[0][small], exp[1][small]), [meta[k] for k in small])


@pytest.mark.parametrize("key", ["DNA4", "AMINO20"])
def test_the_three_families_agree_at_full_length(gpu, bsq, key):
    """No reference, three kernels: over the full-length list the statistics' score and ends are those of k_score_pairs, and under unit
    costs in global mode columns - matches is the distance of k_edit_pairs and the score its negative."""
    import torch
    from bioseq_amd import align
    (ca, oa, cb, ob, row, col), meta = _full_pairs(key)
    tok = _tok(key)
    S, o, e = _scoring(key)
    d = [_dev(x, gpu) for x in (ca, oa, row, col, cb, ob)]
    for mode in MODES:
        kw = dict(matrix=S, gap_open=o, gap_extend=e, mode=mode, max_len=2048)
        s, st = align.stats_pairs(tok, *d, **kw)
        s2, ends = align.score_pairs(tok, *d, ends=True, **kw)
        assert torch.equal(s, s2) and torch.equal(st[:, 2:4], ends), mode
    s, st = align.stats_pairs(tok, *d, matrix=align.score_matrix(tok, 0, -1), gap_open=0, gap_extend=1, mode="global", max_len=2048)
    dist = align.edit_distance_pairs(tok, *d, max_len=2048)
    assert torch.equal(st[:, 5] - st[:, 4], dist) and torch.equal(-s, dist) and int(dist.min()) > 50 and int(dist.max()) > 500


def test_gaps_across_high_lane_boundaries(gpu, bsq):
    """The last case of test_alignments_across_a_lane_boundary in a pattern of 2048 rows: the core sits at rows 32 k - 18 .. 32 k + 21
    between poly-P, and the text's copy lacks the characters of rows 32 k - 1 .. 32 k + 1, so the alignment's gap opens where lane k - 1
    hands its bottom row to lane k -- for k = 17, 40 and 63, in both store orders."""
    rng = np.random.default_rng(18)
    tok = _tok("AMINO20")
    S, o, e = _scoring("AMINO20")
    core_letters = LETTERS["AMINO20"].replace("P", "").replace("W", "")
    pairs, want = [], []
    for k in (17, 40, 63):
        core = twin.random_row(rng, 40, core_letters)
        before = 32 * k - 19
        pat = np.concatenate([np.full(before, ord("P"), np.uint8), core, np.full(2048 - before - 40, ord("P"), np.uint8)])
        text = np.concatenate([np.full(30, ord("W"), np.uint8), core[:18], core[21:], np.full(2049 - 67, ord("W"), np.uint8)])
        pairs += [(pat, text), (text, pat)]
        want += [[before, 30, before + 40, 67, 37, 40], [30, before, 67, before + 40, 37, 40]]
    stores = twin.store_of(pairs)
    exp = _sweep(tok, stores, S, o, e, "local")
    assert exp[1].tolist() == want
    ca, oa, cb, ob, row, col = stores
    _same(_device(gpu, tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=o, gap_extend=e, max_len=2048), exp)


@pytest.mark.parametrize("mode", MODES)
def test_long_text_in_the_widest_form(gpu, bsq, mode):
    """2048 x 4500, the related part of the text from column 2100 on, in both store orders: 71 text tiles of 64 columns with every lane of
    the group at work; one of the two texts also bridges gaps of three rows across lane boundaries."""
    rng = np.random.default_rng(33)
    tok = _tok("AMINO20")
    S, o, e = _scoring("AMINO20")
    pairs = []
    for k in range(2):
        short, long_ = twin.related_pair(rng, 2048, 4500, LETTERS["AMINO20"], rate=0.06)
        if k:  # the second copy also lacks three characters at every fourth lane boundary
            long_ = twin.fit(rng, twin.mutate(rng, _without_runs(short, range(3, 64, 4)), LETTERS["AMINO20"], 0.06), 4500, LETTERS["AMINO20"])
        pairs.append((short, np.concatenate([long_[2400:], long_[:2400]])))
    pairs[1] = pairs[1][::-1]
    stores = twin.store_of(pairs)
    exp = _sweep(tok, stores, S, o, e, mode)
    if mode == "local":
        st = exp[1].tolist()
        assert 2050 < st[0][1] < 2150 and 2050 < st[1][0] < 2150 and min(st[0][4], st[1][4]) > 1500 and st[0][5] - st[0][4] > 100, st
    ca, oa, cb, ob, row, col = stores
    _same(_device(gpu, tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=o, gap_extend=e, mode=mode, max_len=2048), exp)


@functools.lru_cache(maxsize=None)
def _big_tie_stores():
    """Two-letter rows of 513, 1025 and 2048 characters against rows of m and m + 9, in both store orders."""
    rng = np.random.default_rng(19)
    pairs = []
    for m in (513, 1025, 2048):
        for n in (m, m + 9):
            x, y = twin.random_row(rng, m, "AC"), twin.random_row(rng, n, "AC")
            pairs += [(x, y), (y, x)]
    return twin.store_of(pairs)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", [(0, 1), (1, 1), (3, 0), (0, 0)])
def test_ties_at_scale(gpu, bsq, mode, gaps):
    """Two letters, +1 / -1, gaps that cost little or nothing: most cells of a 2048-row table tie between the diagonal and a gap or between
    the two gaps, in every lane, and (local mode, by the sweep's count) the best cell is one of several."""
    from bioseq_amd import align
    tok = _tok("DNA4")
    S = align.score_matrix(tok, 1, -1)
    stores = _big_tie_stores()
    counts = []
    exp = _sweep(tok, stores, S, gaps[0], gaps[1], mode, counts=counts)
    if mode == "local":
        assert max(counts) > 1, counts
    ca, oa, cb, ob, row, col = stores
    _same(_device(gpu, tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=gaps[0], gap_extend=gaps[1], mode=mode, max_len=2048), exp)


@functools.lru_cache(maxsize=None)
def _range_end_stores():
    """Patterns of 1 .. 300 rows, none a multiple of 32 (so rows of the pad class lie beside real rows that score -128), against texts of
    m, m + 3 and m + 40 characters, related (3 %) and unrelated, every second pair with the shorter side in store B."""
    rng = np.random.default_rng(27)
    pairs, meta = [], []
    for m in (1, 5, 31, 33, 65, 100, 127, 129, 200, 300):
        for n in (m, m + 3, m + 40):
            pairs.append(twin.related_pair(rng, m, n, "ACGT", rate=0.03))
            meta.append((m, n))
        pairs.append((twin.random_row(rng, m, "ACGT"), twin.random_row(rng, m + 7, "ACGT")))
        meta.append((m, m + 7))
    for k in range(1, len(pairs), 2):
        pairs[k] = pairs[k][::-1]
    return twin.store_of(pairs), meta


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", [(127, 127), (0, 127)])
def test_ends_of_the_scoring_ranges(gpu, bsq, mode, gaps):
    """A matrix of 127 on the diagonal and -128 off it with gap costs of 127: the largest and smallest entries a cell can add, in every
    form."""
    from bioseq_amd import align
    tok = _tok("DNA4")
    S = align.score_matrix(tok, 127, -128)
    stores, meta = _range_end_stores()
    ca, oa, cb, ob, row, col = stores
    exp = _sweep(tok, stores, S, gaps[0], gaps[1], mode)
    assert exp[0].max() > 127 * 200 and (mode == "local" or exp[0].min() < -128 * 30)
    kw = dict(matrix=S, gap_open=gaps[0], gap_extend=gaps[1], mode=mode)
    for form in (2, 3):
        _same(_device(gpu, tok, ca, oa, row, col, cb, ob, max_len=300, form=form, **kw), exp, meta)
    small = np.array([k for k, (m, n) in enumerate(meta) if min(m, n) <= 128], np.int64)
    _same(_device(gpu, tok, ca, oa, row[small], col[small], cb, ob, max_len=128, form=1, **kw), (exp[0][small], exp[1][small]), [meta[k] for k in small])
