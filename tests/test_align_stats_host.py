"""CPU: the alignment statistics of row pairs (include/bsq.h, "alignment statistics of row pairs") -- the declared symbols, the header's
known answers, the library's host twin bsq_align_stats_host against the cell-by-cell programme of tests/align_stats_twin.py on pairs
full of ties, related protein pairs, asymmetric matrices and both store orders, that programme's anti-diagonal sweep against it and the
host twin against the sweep on patterns of up to 2048 rows, the properties that tie the statistics to the score, the ends and the edit
distance, codes, every refusal, and the verification rule at its exact boundary.  No device is needed."""
import ctypes
import functools

import numpy as np
import pytest

import align_stats_twin as twin

LETTERS = {"DNA4": "ACGT", "AMINO20": "ACDEFGHIKLMNPQRSTVWY"}
BATCH = [b"ACGTAC", b"ACGNACGT", b"AC", b"", b"TTTTTTT"]
MODES = ("local", "global")


def _tok(key):
    import bioseq_amd
    return bioseq_amd.Tokenizer(key, False, False, False)


def _lut(tok):
    from bioseq_amd import capi
    d = capi.desc_of(tok)
    return np.array(list(d.lut), np.int64), d.nchars


def _rows(rows):
    return twin.pack([np.frombuffer(r, np.uint8) for r in rows])


def _grid(n):
    return [a.ravel().astype(np.int64) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]


def _same(got, exp, meta=None):
    (gs, gt), (es, et) = got, exp
    bad = np.nonzero((gs != es) | (gt != et).any(axis=1))[0]
    assert bad.size == 0, [(meta[k] if meta else k, int(gs[k]), gt[k].tolist(), int(es[k]), et[k].tolist()) for k in bad[:6]]
    assert gs.dtype == np.int32 and gt.dtype == np.int32 and gt.shape == (len(es), 6)
    assert gs.tobytes() == es.astype(np.int32).tobytes() and gt.tobytes() == et.astype(np.int32).tobytes()


def _properties(score, stats, la, lb, local):
    """What holds for every pair without a code: 0 <= matches <= diag <= min(spans), columns >= max(spans), starts <= ends <= lengths."""
    st = stats.astype(np.int64)
    ok = score > -2**30
    assert (st[~ok] == -1).all()
    st, la, lb = st[ok], np.asarray(la)[ok], np.asarray(lb)[ok]
    span_a, span_b = st[:, 2] - st[:, 0], st[:, 3] - st[:, 1]
    diag = span_a + span_b - st[:, 5]
    assert (st[:, 0] >= 0).all() and (st[:, 1] >= 0).all() and (span_a >= 0).all() and (span_b >= 0).all()
    assert (st[:, 2] <= la).all() and (st[:, 3] <= lb).all()
    assert (0 <= st[:, 4]).all() and (st[:, 4] <= diag).all() and (diag <= np.minimum(span_a, span_b)).all()
    assert (st[:, 5] >= np.maximum(span_a, span_b)).all()
    if local:
        zero = score[ok] == 0
        assert (st[zero] == 0).all() and (st[~zero][:, 5] > 0).all()
    else:
        assert (st[:, 0] == 0).all() and (st[:, 1] == 0).all() and (st[:, 2] == la).all() and (st[:, 3] == lb).all()


def test_new_symbols_are_declared_and_exported():
    import bioseq_amd.align as align
    from bioseq_amd import capi
    L = capi.load()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_align_stats_device", "bsq_align_stats_host", "bsq_align_stats_kernel_name"):
        assert n in names and hasattr(L, n), n
    assert L.bsq_abi_version() == 7 and ctypes.sizeof(capi.Score) == 20 + 32 * 32
    for n in ("stats_pairs", "stats_pairs_host", "stats_kernel_name", "stats_identity", "stats_coverage", "verify_align_pairs",
              "verify_align_pairs_host"):
        assert n in align.__all__ and callable(getattr(align, n))
    assert align.STATS_MAX_LEN == 2048 and "STATS_MAX_LEN" in align.__all__
    assert [align.stats_kernel_name(mode=m, max_len=n) for m, n in (("local", 128), ("local", 129), ("global", 512), ("global", 513), ("local", 2048))] == \
        ["k_align_stats<4, local>", "k_align_stats<16, local>", "k_align_stats<16, global>", "k_align_stats<64, global>", "k_align_stats<64, local>"]
    assert align.stats_kernel_name(max_len=100, form=3) == "k_align_stats<64, local>"
    assert align.stats_kernel_name(max_len=2049) == "" and align.stats_kernel_name(max_len=129, form=1) == "" and align.stats_kernel_name(gap_open=128) == ""


def test_known_answers_dna4():
    """The answers of include/bsq.h from the cell twin and the host twin."""
    from bioseq_amd import align
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    chars, offs = _rows(BATCH)
    row, col = _grid(5)
    S = align.score_matrix(tok, 2, -3)
    want_local = [(0, 0, 6, 6, 6, 6), (0, 4, 4, 8, 4, 4), (0, 0, 2, 2, 2, 2), (0,) * 6, (3, 0, 4, 1, 1, 1),
                  (4, 0, 8, 4, 4, 4), (0, 0, 8, 8, 8, 8), (0, 0, 2, 2, 2, 2), (0,) * 6, (7, 0, 8, 1, 1, 1),
                  (0, 0, 2, 2, 2, 2), (0, 0, 2, 2, 2, 2), (0, 0, 2, 2, 2, 2), (0,) * 6, (0,) * 6] + [(0,) * 6] * 5 + \
                 [(0, 3, 1, 4, 1, 1), (0, 7, 1, 8, 1, 1), (0,) * 6, (0,) * 6, (0, 0, 7, 7, 7, 7)]
    local_scores = [12, 8, 4, 0, 2, 8, 16, 4, 0, 2, 4, 4, 4, 0, 0, 0, 0, 0, 0, 0, 2, 2, 0, 0, 14]
    # global: starts (0, 0), ends (la, lb); (matches, columns) of every (i, j)
    want_global = [(6, 6), (5, 8), (2, 6), (0, 6), (1, 7), (5, 8), (8, 8), (2, 8), (0, 8), (1, 8), (2, 6), (2, 8), (2, 2), (0, 2), (0, 7),
                   (0, 6), (0, 8), (0, 2), (0, 0), (0, 7), (1, 7), (1, 8), (0, 7), (0, 7), (7, 7)]
    global_scores = [12, -2, -9, -17, -20, -2, 16, -13, -21, -23, -9, -13, 4, -9, -21, -17, -21, -9, 0, -19, -20, -23, -21, -19, 14]
    lengths = np.diff(offs)
    for stats_pairs in (lambda **kw: twin.stats_pairs(lut, nchars, chars, offs, chars, offs, row, col, S, 5, 2, kw["mode"]),
                        lambda **kw: align.stats_pairs_host(tok, chars, offs, row, col, matrix=S, gap_open=5, gap_extend=2, **kw)):
        s, st = stats_pairs(mode="local")
        assert s.tolist() == local_scores and [tuple(r) for r in st.tolist()] == want_local
        s, st = stats_pairs(mode="global")
        assert s.tolist() == global_scores and [tuple(r) for r in st[:, 4:].tolist()] == want_global
        assert (st[:, :2] == 0).all() and st[:, 2].tolist() == lengths[row].tolist() and st[:, 3].tolist() == lengths[col].tolist()
    # case folds and the unmapped class equals itself: acgtNN- against ACGTnxA aligns end to end with 6 identical columns of 7
    chars2, offs2 = _rows([b"acgtNN-", b"ACGTnxA"])
    s, st = align.stats_pairs_host(tok, chars2, offs2, np.array([0], np.int64), np.array([1], np.int64), matrix=S, gap_open=5, gap_extend=2, mode="global")
    assert s.tolist() == [9] and st.tolist() == [[0, 0, 7, 7, 6, 7]]


def test_known_answers_blosum62():
    from bioseq_amd import align
    tok = _tok("AMINO20")
    lut, nchars = _lut(tok)
    S = align.blosum62_matrix(tok)
    chars, offs = _rows([b"HEAGAWGHEE", b"PAWHEAE"])
    row, col = np.array([0, 1], np.int64), np.array([1, 0], np.int64)
    want = {(11, 1, "local"): ([17, 17], [[0, 3, 3, 6, 3, 3], [3, 0, 6, 3, 3, 3]]),
            (11, 1, "global"): ([1, 1], [[0, 0, 10, 7, 3, 10], [0, 0, 7, 10, 3, 10]]),
            (0, 8, "local"): ([20, 20], [[4, 1, 9, 5, 4, 5], [1, 4, 5, 9, 4, 5]]),
            (0, 8, "global"): ([-8, -8], [[0, 0, 10, 7, 3, 10], [0, 0, 7, 10, 3, 10]])}
    for (o, e, mode), (ws, wt) in want.items():
        for s, st in (twin.stats_pairs(lut, nchars, chars, offs, chars, offs, row, col, S, o, e, mode),
                      align.stats_pairs_host(tok, chars, offs, row, col, matrix=S, gap_open=o, gap_extend=e, mode=mode)):
            assert s.tolist() == ws and st.tolist() == wt, (o, e, mode)


@functools.lru_cache(maxsize=None)
def _tie_pairs():
    """300 pairs of up to 40 x 60 over two letters, the shorter row in A as often as in B, equal lengths and empty rows among them."""
    rng = np.random.default_rng(1)
    pairs = []
    for k in range(300):
        m, n = int(rng.integers(0, 41)), int(rng.integers(0, 61))
        n = m if k % 10 == 0 else n
        x, y = twin.random_row(rng, m, "AC"), twin.random_row(rng, n, "AC")
        pairs.append((x, y) if k % 2 else (y, x))
    return pairs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", [(0, 1), (1, 1)])
def test_pairs_full_of_ties(mode, gaps):
    """Two letters, +1 / -1: most cells tie between the diagonal and a gap or between the two gaps, and most best cells are one of many."""
    from bioseq_amd import align
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    S = align.score_matrix(tok, 1, -1)
    ca, oa, cb, ob, row, col = twin.store_of(_tie_pairs())
    exp = twin.stats_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, gaps[0], gaps[1], mode)
    got = align.stats_pairs_host(tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=gaps[0], gap_extend=gaps[1], mode=mode)
    _same(got, exp)
    _properties(got[0], got[1], np.diff(oa)[row], np.diff(ob)[col], mode == "local")
    s, en = align.score_pairs_host(tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=gaps[0], gap_extend=gaps[1], mode=mode, ends=True)
    assert got[0].tobytes() == s.tobytes() and np.ascontiguousarray(got[1][:, 2:4]).tobytes() == en.tobytes()
    assert len({tuple(r) for r in got[1].tolist()}) > 100  # (a check of something)


@functools.lru_cache(maxsize=None)
def _protein_pairs():
    """Related AMINO20 pairs around the 32-row edges, every second one with the shorter row in B, and a matrix that is not symmetric."""
    rng = np.random.default_rng(7)
    letters = LETTERS["AMINO20"]
    pairs = []
    for m, n in ((5, 9), (31, 31), (32, 40), (33, 33), (64, 70), (65, 65), (90, 140), (100, 100), (129, 160)):
        pairs.append(twin.related_pair(rng, m, n, letters, rate=0.1))
        pairs.append(twin.related_pair(rng, m, n, letters, rate=0.25)[::-1])
    asym = rng.integers(-5, 3, size=(21, 21)).astype(np.int8)
    asym[np.arange(21), np.arange(21)] = rng.integers(3, 9, size=21)
    assert (asym != asym.T).any()
    return pairs, asym


@pytest.mark.parametrize("mode", MODES)
def test_related_proteins_and_asymmetric_matrices(mode):
    """Related AMINO20 pairs around the 32-row edges under BLOSUM62 {11, 1}, both store orders; then an asymmetric matrix, where swapping
    the stores needs the transposed matrix and swaps the statistics wherever one cell alone is best."""
    from bioseq_amd import align
    tok = _tok("AMINO20")
    lut, nchars = _lut(tok)
    pairs, asym = _protein_pairs()
    ca, oa, cb, ob, row, col = twin.store_of(pairs)
    B62 = align.blosum62_matrix(tok)
    for S, o, e in ((B62, 11, 1), (asym, 4, 1), (asym, 0, 2)):
        exp = twin.stats_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, o, e, mode)
        got = align.stats_pairs_host(tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=o, gap_extend=e, mode=mode)
        _same(got, exp)
        _properties(got[0], got[1], np.diff(oa)[row], np.diff(ob)[col], mode == "local")
        assert got[1][:, 4].max() > 40  # (related rows: long alignments)
        s, en = align.score_pairs_host(tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=o, gap_extend=e, mode=mode, ends=True)
        assert got[0].tobytes() == s.tobytes() and np.ascontiguousarray(got[1][:, 2:4]).tobytes() == en.tobytes()
        St = np.ascontiguousarray(S.T)
        back = twin.stats_pairs(lut, nchars, cb, ob, ca, oa, col, row, St, o, e, mode)
        _same(align.stats_pairs_host(tok, cb, ob, col, row, ca, oa, matrix=St, gap_open=o, gap_extend=e, mode=mode), back)
        assert back[0].tobytes() == exp[0].tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_the_sweep_equals_the_cell_programme(mode):
    """align_stats_diag == align_stats, statistics and all: on the pairs full of ties under gaps that cost an opening, an extension, only
    one of them and nothing, and on the related proteins under BLOSUM62 {11, 1} and the matrix that is not symmetric.  The count of best
    cells is that of score_twin.gotoh_cells."""
    import score_twin
    from bioseq_amd import align
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    S = align.score_matrix(tok, 1, -1)
    ca, oa, cb, ob, row, col = twin.store_of(_tie_pairs())
    many = 0
    for o, e in ((0, 1), (1, 1), (3, 0), (0, 0)):
        counts = []
        swept = twin.stats_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, o, e, mode, one=twin.align_stats_diag, counts=counts)
        _same(swept, twin.stats_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, o, e, mode))
        for k in range(0, len(row), 7):
            x, y = (twin.classes(lut, nchars, c[f[k]:f[k + 1]]) for c, f in ((ca, oa), (cb, ob)))
            assert counts[k] == score_twin.gotoh_cells(x, y, S, o, e, mode)[3], (k, o, e)
        many += sum(c > 1 for c in counts)
    assert mode == "global" or many > 400  # (most best cells are one of many)
    tok = _tok("AMINO20")
    lut, nchars = _lut(tok)
    pairs, asym = _protein_pairs()
    ca, oa, cb, ob, row, col = twin.store_of(pairs)
    for S, o, e in ((align.blosum62_matrix(tok), 11, 1), (asym, 4, 1), (asym, 0, 2)):
        swept = twin.stats_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, o, e, mode, one=twin.align_stats_diag)
        _same(swept, twin.stats_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, o, e, mode))


FULL_SIZES = ((129, 160), (511, 600), (513, 513), (1000, 1500), (2047, 2048), (2048, 2048), (2048, 3000), (700, 5000))


@functools.lru_cache(maxsize=None)
def _full_length_pairs():
    """Every size of FULL_SIZES three times: a DNA4 pair related at 8 %, a two-letter related pair with the shorter row in B, and two
    unrelated two-letter rows.  The stores and the list, shared by every scoring and mode."""
    rng = np.random.default_rng(29)
    pairs, meta = [], []
    for m, n in FULL_SIZES:
        pairs.append(twin.related_pair(rng, m, n, "ACGT", rate=0.08))
        pairs.append(twin.related_pair(rng, m, n, "AC", rate=0.08)[::-1])
        pairs.append((twin.random_row(rng, m, "AC"), twin.random_row(rng, n, "AC")))
        meta += [(m, n, "related"), (n, m, "two letters, related"), (m, n, "two letters")]
    return twin.store_of(pairs), meta


@pytest.mark.parametrize("scoring", [(2, -3, 5, 2, "local"), (2, -3, 5, 2, "global"), (1, -1, 0, 1, "local"), (1, -1, 3, 0, "local"), (1, -1, 0, 0, "local")])
def test_host_twin_against_the_sweep_at_full_length(scoring):
    """bsq_align_stats_host == align_stats_diag on patterns of up to 2048 rows -- every lane of the widest form's pattern, texts of up to
    5000 columns: the two share no cell, no packing and no orientation, so a mistake in what the host twin and the kernels compile
    together shows here."""
    from bioseq_amd import align
    match, mismatch, o, e, mode = scoring
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    S = align.score_matrix(tok, match, mismatch)
    (ca, oa, cb, ob, row, col), meta = _full_length_pairs()
    counts = []
    exp = twin.stats_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, o, e, mode, one=twin.align_stats_diag, counts=counts)
    got = align.stats_pairs_host(tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=o, gap_extend=e, mode=mode)
    _same(got, exp, meta)
    _properties(got[0], got[1], np.diff(oa)[row], np.diff(ob)[col], mode == "local")
    if mode == "local":
        if (o, e) == (5, 2):  # (not vacuous: the related pairs align over most of the shorter row)
            assert all(st[4] > min(m, n) // 2 for st, (m, n, kind) in zip(exp[1].tolist(), meta) if kind == "related")
        else:
            assert sum(c > 1 for c in counts) >= 8  # (best cells that are one of many)


def test_unit_costs_give_the_edit_distance():
    """score_matrix(0, -1), {0, 1}, global: every column is a match or costs 1, so columns - matches is the edit distance."""
    from bioseq_amd import align
    rng = np.random.default_rng(3)
    tok = _tok("DNA4")
    pairs = [twin.related_pair(rng, int(m), int(m + d), "ACGT", rate=0.15) for m, d in zip(rng.integers(0, 80, size=60), rng.integers(0, 30, size=60))]
    pairs += [p[::-1] for p in pairs[:20]]
    ca, oa, cb, ob, row, col = twin.store_of(pairs)
    s, st = align.stats_pairs_host(tok, ca, oa, row, col, cb, ob, matrix=align.score_matrix(tok, 0, -1), gap_open=0, gap_extend=1, mode="global")
    dist = align.edit_distance_host(tok, ca, oa, row, col, cb, ob)
    assert (st[:, 5] - st[:, 4]).tolist() == dist.tolist() == (-s).tolist() and dist.max() > 10


def test_self_alignment_and_planted_cores():
    """A row against itself: (0, 0, L, L, L, L) in both modes.  junk + core + junk against the core: the planted start and end, in both
    store orders, the core across the 32-row edge of the pattern included."""
    from bioseq_amd import align
    rng = np.random.default_rng(5)
    tok = _tok("AMINO20")
    S = align.blosum62_matrix(tok)
    letters = LETTERS["AMINO20"]
    rows = [twin.random_row(rng, n, letters) for n in (1, 31, 32, 33, 100, 700)]
    chars, offs = twin.pack(rows)
    idx = np.arange(len(rows), dtype=np.int64)
    for mode in MODES:
        s, st = align.stats_pairs_host(tok, chars, offs, idx, idx, matrix=S, gap_open=11, gap_extend=1, mode=mode)
        L = np.diff(offs)
        assert st.tolist() == [[0, 0, n, n, n, n] for n in L.tolist()]
        assert s.tolist() == twin.stats_pairs(*_lut(tok), chars, offs, chars, offs, idx, idx, S, 11, 1, mode)[0].tolist()
    # the junk is poly-P against a core without P: nothing outside the core scores
    core_letters = letters.replace("P", "")
    pairs, want = [], []
    for before, n, after in ((0, 40, 0), (7, 40, 13), (20, 30, 100), (3, 64, 5), (50, 10, 0), (0, 10, 50)):
        core = twin.random_row(rng, n, core_letters)
        whole = np.concatenate([np.full(before, ord("P"), np.uint8), core, np.full(after, ord("P"), np.uint8)])
        pairs += [(whole, core), (core, whole)]
        want += [[before, 0, before + n, n, n, n], [0, before, n, before + n, n, n]]
    ca, oa, cb, ob, row, col = twin.store_of(pairs)
    s, st = align.stats_pairs_host(tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=11, gap_extend=1)
    assert st.tolist() == want and (s > 0).all()


def test_codes_and_refusals():
    """max_len + 1 on the shorter side, indices outside the stores, a longer side beyond 2^20; what the library refuses writes nothing."""
    from bioseq_amd import align, capi
    L = capi.load()
    rng = np.random.default_rng(9)
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    S = align.score_matrix(tok, 2, -3)
    kw = dict(matrix=S, gap_open=5, gap_extend=2)
    rows = [twin.random_row(rng, n, "ACGT") for n in (99, 100, 101, 300)]
    chars, offs = twin.pack(rows)
    row = np.array([0, 1, 2, 1, 2, 2, -1, 0, 4, 1 << 40, 0, 0], np.int64)
    col = np.array([3, 3, 3, 1, 2, 0, 0, 4, 4, 0, -(1 << 40), 1], np.int64)
    for mode in MODES:
        exp = twin.stats_pairs(lut, nchars, chars, offs, chars, offs, row, col, S, 5, 2, mode, max_len=100)
        assert exp[0][[2, 4]].tolist() == [twin.TOO_LONG] * 2 and exp[0][6:11].tolist() == [twin.BAD_INDEX] * 5
        assert (exp[1][[2, 4, 6, 7, 8, 9, 10]] == -1).all() and (exp[1][[0, 1, 3, 5, 11]] >= 0).all()
        _same(align.stats_pairs_host(tok, chars, offs, row, col, mode=mode, max_len=100, **kw), exp)
    big = [np.frombuffer(b"G", np.uint8), twin.random_row(rng, (1 << 20) + 1, "ACGT")]
    chars2, offs2 = twin.pack(big)
    s, st = align.stats_pairs_host(tok, chars2, offs2, np.array([0, 1], np.int64), np.array([1, 0], np.int64), **kw)
    assert s.tolist() == [twin.TOO_LONG] * 2 and (st == -1).all()
    # refusals of the Python layer
    idx = np.array([0], np.int64)
    for bad in (dict(max_len=2049), dict(max_len=0), dict(max_len=129, form=1), dict(max_len=513, form=2), dict(form=4), dict(mode="semi")):
        with pytest.raises(ValueError):
            align.stats_pairs_host(tok, chars, offs, idx, idx, **{**kw, **bad})
    with pytest.raises(ValueError):
        align.stats_pairs_host(tok, chars, offs, idx, idx, matrix=S, gap_open=128, gap_extend=1)
    with pytest.raises(ValueError):
        align.stats_pairs_host(_tok("BYTES"), chars, offs, idx, idx, matrix=np.zeros((257, 257), np.int8), gap_open=1, gap_extend=1)
    # refusals of the library: the status, and nothing written
    desc = capi.desc_of(tok)
    score, stats = np.full(2, 7, np.int32), np.full(12, 7, np.int32)
    r2, c2 = np.array([0, 1], np.int64), np.array([1, 0], np.int64)

    def call(d=desc, ch=chars.ctypes.data, of=offs.ctypes.data, B=4, rw=r2.ctypes.data, cl=c2.ctypes.data, n=2, sc=None, out=score.ctypes.data,
             st=stats.ctypes.data, rules=(100, 0, 0, 1, 1)):
        s = capi.Score(*rules)
        return L.bsq_align_stats_host(ctypes.byref(d) if d is not None else None, ch, of, B, ch, of, B, rw, cl, n, None if sc == "null" else ctypes.byref(s), out, st)

    for rules in ((0, 0, 0, 1, 1), (2049, 0, 0, 1, 1), (4096, 0, 0, 1, 1), (129, 1, 0, 1, 1), (513, 2, 0, 1, 1), (100, 4, 0, 1, 1), (100, -1, 0, 1, 1),
                  (100, 0, 2, 1, 1), (100, 0, -1, 1, 1), (100, 0, 0, 128, 1), (100, 0, 0, -1, 1), (100, 0, 1, 1, 128)):
        assert call(rules=rules) == 2, rules  # (BSQ_ERR_INVALID_ARG)
        assert L.bsq_align_stats_kernel_name(ctypes.byref(capi.Score(*rules))) == b"", rules
    wide = capi.desc_of(_tok("BYTES"))
    for kwargs in (dict(d=None), dict(d=wide), dict(ch=None), dict(of=None), dict(B=-1), dict(rw=None), dict(cl=None), dict(n=-1), dict(sc="null"),
                   dict(out=None), dict(st=None)):
        assert call(**kwargs) == 2, kwargs
    assert L.bsq_align_stats_kernel_name(None) == b""
    assert (score == 7).all() and (stats == 7).all()
    assert call(rw=None, cl=None, n=0, out=None, st=None) == 0 and (score == 7).all()  # n_pairs == 0: nothing to do
    assert call(ch=None, of=None, B=0) == 0  # stores without rows: every index is bad
    assert score.tolist() == [twin.BAD_INDEX] * 2 and (stats == -1).all()
    s, st = align.stats_pairs_host(tok, chars, offs, np.zeros(0, np.int64), np.zeros(0, np.int64), **kw)
    assert s.shape == (0,) and st.shape == (0, 6)


def test_identity_and_coverage():
    from bioseq_amd import align
    stats = np.array([[2, 0, 10, 8, 6, 9], [0, 0, 0, 0, 0, 0], [-1] * 6, [0, 0, 4, 4, 4, 4]], np.int32)
    la, lb = np.array([10, 5, 3, 4], np.int64), np.array([16, 0, 3, 4], np.int64)
    ident = align.stats_identity(stats)
    assert ident.dtype == np.float32 and ident[0] == np.float32(6 / 9) and np.isnan(ident[1]) and np.isnan(ident[2]) and ident[3] == 1
    assert align.stats_identity(stats, "shorter", la, lb)[[0, 3]].tolist() == [np.float32(0.6), 1.0] and np.isnan(align.stats_identity(stats, "shorter", la, lb)[1])
    assert align.stats_identity(stats, "longer", la, lb)[0] == np.float32(6 / 16)
    ca, cb = align.stats_coverage(stats, la, lb)
    assert ca.dtype == np.float32 and ca[0] == np.float32(0.8) and cb[0] == np.float32(0.5) and ca[1] == 0 and np.isnan(cb[1]) and np.isnan(ca[2]) and cb[3] == 1
    with pytest.raises(ValueError):
        align.stats_identity(stats, "shorter")
    with pytest.raises(ValueError):
        align.stats_identity(stats, "all")


def test_verification_rule():
    """verify_align_pairs_host against `keeps` on Python integers over every option, and a threshold met with equality."""
    from bioseq_amd import align
    rng = np.random.default_rng(11)
    tok = _tok("AMINO20")
    S = align.blosum62_matrix(tok)
    letters = LETTERS["AMINO20"]
    base = twin.random_row(rng, 120, letters)
    rows = [base] + [twin.fit(rng, twin.mutate(rng, base, letters, rate), n, letters) for rate, n in
                     ((0.0, 120), (0.03, 120), (0.08, 110), (0.15, 130), (0.3, 120), (0.05, 60), (0.05, 200))]
    rows += [base[20:80], np.concatenate([twin.random_row(rng, 100, letters), base[:50]]), np.zeros(0, np.uint8), twin.random_row(rng, 300, letters)]
    chars, offs = twin.pack(rows)
    row, col = _grid(len(rows))
    row, col = np.concatenate([row, [-1, 0]]).astype(np.int64), np.concatenate([col, [0, 99]]).astype(np.int64)
    kw = dict(matrix=S, gap_open=11, gap_extend=1, max_len=250)
    lengths = np.diff(offs)
    la, lb = lengths[np.clip(row, 0, len(rows) - 1)], lengths[np.clip(col, 0, len(rows) - 1)]
    seen = set()
    for mode in MODES:
        score, stats = align.stats_pairs_host(tok, chars, offs, row, col, mode=mode, **kw)
        assert (score == twin.TOO_LONG).any() and (score == twin.BAD_INDEX).sum() == 2
        for opts in (dict(), dict(min_identity=0.5, min_coverage=0.5), dict(identity_over="shorter"), dict(coverage="shorter", min_identity=0.8),
                     dict(coverage="longer", min_coverage=0.4), dict(coverage="a", min_coverage=0.45), dict(coverage="b", min_coverage=0.45),
                     dict(min_identity=0.0, min_coverage=0.0, min_score=200), dict(min_identity=1.0, min_coverage=1.0), dict(min_score=-10**6, min_identity=0.0)):
            keep, s2, st2 = align.verify_align_pairs_host(tok, chars, offs, row, col, mode=mode, **opts, **kw)
            assert keep.dtype == np.bool_ and s2.tobytes() == score.tobytes() and st2.tobytes() == stats.tobytes()
            want = twin.keeps(score, stats, la, lb, **opts)
            assert keep.tolist() == want.tolist(), (mode, opts)
            assert not keep[score <= -2**30].any()
            seen.add((bool(keep.any()), bool(keep.all())))
    assert (True, False) in seen
    # equality: AAAAAAAA against AAAACCAA under +1 / -1 {3, 1}, global: 6 identical columns of 8, identity 0.75 exactly
    t4 = _tok("DNA4")
    chars, offs = _rows([b"AAAAAAAA", b"AAAACCAA", b"AAAAAAAAA", b"AAAAAAAAAAAA"])
    S4 = align.score_matrix(t4, 1, -1)
    k4 = dict(matrix=S4, gap_open=3, gap_extend=1, mode="global", min_coverage=0.0)
    one = np.array([0], np.int64)
    keep, s, st = align.verify_align_pairs_host(t4, chars, offs, one, one + 1, min_identity=0.75, **k4)
    assert st.tolist() == [[0, 0, 8, 8, 6, 8]] and keep.tolist() == [True] and 6 * 65536 == 49152 * 8
    assert align.verify_align_pairs_host(t4, chars, offs, one, one + 1, min_identity=49153 / 65536, **k4)[0].tolist() == [False]
    # coverage with equality: the 9-character row covers 9 of the 12-character one in local mode, 0.75 exactly
    k5 = dict(matrix=S4, gap_open=3, gap_extend=1, min_identity=0.0, coverage="b")
    keep, s, st = align.verify_align_pairs_host(t4, chars, offs, one + 2, one + 3, min_coverage=0.75, **k5)
    assert st.tolist() == [[0, 0, 9, 9, 9, 9]] and keep.tolist() == [True] and 9 * 65536 == 49152 * 12
    assert align.verify_align_pairs_host(t4, chars, offs, one + 2, one + 3, min_coverage=49153 / 65536, **k5)[0].tolist() == [False]
    assert align.verify_align_pairs_host(t4, chars, offs, one + 2, one + 3, min_coverage=1.0, **{**k5, "coverage": "a"})[0].tolist() == [True]
    with pytest.raises(ValueError):
        align.verify_align_pairs_host(t4, chars, offs, one, one, min_coverage=1.5, **k5)
    with pytest.raises(ValueError):
        align.verify_align_pairs_host(t4, chars, offs, one, one, identity_over="longer", **k4)
