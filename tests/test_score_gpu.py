"""GPU: the scored alignment of row pairs (bioseq_amd.align, bsq_score_pairs_device) against the plain Gotoh programme of
tests/score_twin.py and the library's host twin, byte for byte, scores and ends: shorter sides at every lane and group edge with four
longer sides each in both modes, a long deletion that tells affine gaps from linear ones, every form on the pairs it holds, rows full
of ties, an asymmetric matrix, the ends of the scoring ranges, waves whose groups finish at different steps with guards around both outputs, the codes, long texts,
unmapped bytes, the Python surface on a side stream, and the pipeline from sketches to score-verified clusters."""
import ctypes
import functools

import numpy as np
import pytest

import score_twin as twin

pytestmark = pytest.mark.gpu

LETTERS = {"DNA4": "ACGT", "AMINO20": "ACDEFGHIKLMNPQRSTVWY"}
EDGES = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096)
MODES = ("local", "global")


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
    """The issue's two scorings: BLOSUM62 {11, 1} for AMINO20, +2 / -3 {5, 2} for DNA4."""
    from bioseq_amd import align
    tok = _tok(key)
    return (align.blosum62_matrix(tok), 11, 1) if key == "AMINO20" else (align.score_matrix(tok, 2, -3), 5, 2)


def _device(gpu, tok, ca, oa, row, col, cb=None, ob=None, *, ends=True, **kw):
    """score_pairs on uploaded copies, as numpy arrays (score, ends); int32 device tensors of the list's length."""
    import torch
    from bioseq_amd import align
    b = () if cb is None else (_dev(cb, gpu), _dev(ob, gpu))
    got = align.score_pairs(tok, _dev(ca, gpu), _dev(oa, gpu), _dev(row, gpu), _dev(col, gpu), *b, ends=ends, **kw)
    s, e = got if ends else (got, None)
    assert s.dtype == torch.int32 and s.device == gpu and s.is_contiguous() and tuple(s.shape) == (len(row),)
    if not ends:
        return s.cpu().numpy()
    assert e.dtype == torch.int32 and e.device == gpu and e.is_contiguous() and tuple(e.shape) == (len(row), 2)
    return s.cpu().numpy(), e.cpu().numpy()


def _same(got, exp, meta=None):
    (gs, ge), (es, ee) = got, exp
    bad = np.nonzero((gs != es) | (ge != ee).any(axis=1))[0]
    assert bad.size == 0, [(meta[k] if meta else k, int(gs[k]), ge[k].tolist(), int(es[k]), ee[k].tolist()) for k in bad[:6]]
    assert gs.tobytes() == es.tobytes() and ge.tobytes() == ee.tobytes()


@functools.lru_cache(maxsize=None)
def _edge_pairs(key):
    """Every shorter side of EDGES against longer sides m, m + 1, m + 70 and 2 m + 3, unrelated and related (mutated at 4 %), the shorter
    side in store B as often as in store A; last, a 60-character row against itself with four characters deleted in one run."""
    rng = np.random.default_rng(len(key) + 40)
    pairs, meta = [], []
    for m in EDGES:
        for n in (m, m + 1, m + 70, 2 * m + 3):
            pairs.append((twin.random_row(rng, m, LETTERS[key]), twin.random_row(rng, n, LETTERS[key])))
            pairs.append(twin.related_pair(rng, m, n, LETTERS[key], rate=0.04))
            meta += [(m, n, False), (m, n, True)]
    for k in range(1, len(pairs), 4):
        pairs[k] = pairs[k][::-1]
    whole = twin.random_row(rng, 60, LETTERS[key])
    pairs.append((twin.delete_run(whole, 27, 4), whole))
    meta.append((56, 60, True))
    return pairs, meta


@functools.lru_cache(maxsize=None)
def _edges(key, mode):
    """The stores, the list and the twin's answers under the key's scoring (computed once per alphabet and mode)."""
    pairs, meta = _edge_pairs(key)
    ca, oa, cb, ob, row, col = twin.store_of(pairs)
    lut, nchars = _lut(_tok(key))
    S, o, e = _scoring(key)
    return ca, oa, cb, ob, row, col, twin.score_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, o, e, mode), meta


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ["DNA4", "AMINO20"])
def test_lane_and_group_edges(gpu, bsq, key, mode):
    """One lane, a last lane of 1, 63 and 64 rows, the first row of a second lane, the last lane of every form and one past it."""
    from bioseq_amd import align
    ca, oa, cb, ob, row, col, exp, meta = _edges(key, mode)
    tok = _tok(key)
    S, o, e = _scoring(key)
    if mode == "local":
        lut, nchars = _lut(tok)
        sa, sb = twin.self_scores(lut, nchars, ca, oa, S), twin.self_scores(lut, nchars, cb, ob, S)
        for k, (m, n, related) in enumerate(meta):
            if related and m >= 63:
                assert 0 < exp[0][k] < min(sa[k], sb[k]), (m, n)  # (not vacuous: neither equal rows nor nothing in common)
    else:
        assert (exp[1][:, 0] == np.diff(oa)).all() and (exp[1][:, 1] == np.diff(ob)).all()
    kw = dict(matrix=S, gap_open=o, gap_extend=e, mode=mode)
    _same(align.score_pairs_host(tok, ca, oa, row, col, cb, ob, ends=True, **kw), exp, meta)
    _same(_device(gpu, tok, ca, oa, row, col, cb, ob, **kw), exp, meta)
    assert _device(gpu, tok, ca, oa, row, col, cb, ob, ends=False, **kw).tobytes() == exp[0].tobytes(), "without ends"


@pytest.mark.parametrize("key", ["DNA4", "AMINO20"])
def test_a_long_deletion_tells_affine_from_linear(gpu, bsq, key):
    """The last pair of the list lost four characters in one run: {11, 1} charges it once, {0, 12} four times."""
    pairs, _ = _edge_pairs(key)
    tok = _tok(key)
    lut, nchars = _lut(tok)
    S = _scoring(key)[0]
    ca, oa, cb, ob, row, col = twin.store_of(pairs[-1:] + pairs[-1:][::-1])
    row, col = np.array([0, 1, 1], np.int64), np.array([0, 1, 0], np.int64)
    scores = []
    for o, e in ((11, 1), (0, 12)):
        for mode in MODES:
            exp = twin.score_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, o, e, mode)
            _same(_device(gpu, tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=o, gap_extend=e, mode=mode, max_len=64), exp)
            scores.append(int(exp[0][0]))
    assert scores[0] != scores[2] and scores[1] != scores[3], scores


@pytest.mark.parametrize("key", ["DNA4", "AMINO20"])
def test_every_form_gives_one_result(gpu, bsq, key):
    from bioseq_amd import align
    tok = _tok(key)
    S, o, e = _scoring(key)
    for mode in MODES:
        ca, oa, cb, ob, row, col, exp, meta = _edges(key, mode)
        m = np.array([x[0] for x in meta])
        for max_len, forms in ((256, (None, 1, 2, 3)), (1024, (None, 2, 3))):
            sel = np.nonzero(m <= max_len)[0]
            for form in forms:
                got = _device(gpu, tok, ca, oa, row[sel], col[sel], cb, ob, matrix=S, gap_open=o, gap_extend=e, mode=mode, max_len=max_len, form=form)
                _same(got, (exp[0][sel], exp[1][sel]), [meta[k] + (form,) for k in sel])
    d = [_dev(x, gpu) for x in (ca, oa, row, col)]
    for max_len, form in ((257, 1), (1025, 2)):
        with pytest.raises(ValueError):
            align.score_pairs(tok, *d, matrix=S, gap_open=o, gap_extend=e, max_len=max_len, form=form)


def test_ties_take_the_smallest_ends(gpu, bsq):
    """Poly-A rows, ACAC... rows and a row against itself doubled, in both store orders, every form, lengths around 64 and 256: many
    cells reach the maximum (the twin counts them), and the ends are the smallest end_a, then the smallest end_b."""
    rng = np.random.default_rng(31)
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    S, o, e = _scoring("DNA4")
    pairs = []
    for m in (63, 64, 65, 255, 256):
        a, ac, x = np.full(m, ord("A"), np.uint8), np.frombuffer(b"AC" * 200, np.uint8)[:m], twin.random_row(rng, m, "ACGT")
        pairs += [(a, np.full(m + 9, ord("A"), np.uint8)), (ac, np.frombuffer(b"AC" * 300, np.uint8)[:2 * m + 1]), (x, np.concatenate([x, x])),
                  (np.concatenate([x[:m // 2], x[:m // 2]]), x[:m // 2])]
    pairs += [p[::-1] for p in pairs]
    counts = [twin.gotoh(twin.classes(lut, nchars, x), twin.classes(lut, nchars, y), S, o, e, "local")[3] for x, y in pairs]
    assert min(counts) > 1, counts
    ca, oa, cb, ob, row, col = twin.store_of(pairs)
    exp = twin.score_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, o, e, "local")
    for form in (1, 2, 3):
        _same(_device(gpu, tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=o, gap_extend=e, max_len=256, form=form), exp)
    # gaps that cost nothing to extend, or nothing at all: ties along whole rows and columns
    for o2, e2 in ((3, 0), (0, 0)):
        exp = twin.score_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, o2, e2, "local")
        _same(_device(gpu, tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=o2, gap_extend=e2, max_len=256), exp)


def test_asymmetric_matrix(gpu, bsq):
    """A matrix that is not symmetric, the shorter side in A and in B: the kernel reads S for one and S transposed for the other."""
    rng = np.random.default_rng(23)
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    S = rng.integers(-6, 7, size=(5, 5)).astype(np.int8)
    S[np.arange(5), np.arange(5)] = rng.integers(1, 7, size=5)
    assert (S != S.T).any()
    pairs = []
    for m, n in ((5, 9), (9, 5), (64, 70), (70, 64), (65, 65), (130, 40), (300, 257), (257, 300), (0, 4), (4, 0)):
        x = twin.random_row(rng, m, "ACGTN")
        pairs.append((x, twin.fit(rng, twin.mutate(rng, x, "ACGTN", 0.1), n, "ACGTN")))
    ca, oa, cb, ob, row, col = twin.store_of(pairs)
    for mode in MODES:
        exp = twin.score_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, 4, 1, mode)
        _same(_device(gpu, tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=4, gap_extend=1, mode=mode), exp)
        back = twin.score_pairs(lut, nchars, cb, ob, ca, oa, col, row, S.T, 4, 1, mode)
        assert back[0].tobytes() == exp[0].tobytes()
        _same(_device(gpu, tok, cb, ob, col, row, ca, oa, matrix=np.ascontiguousarray(S.T), gap_open=4, gap_extend=1, mode=mode), back)
        wrong = _device(gpu, tok, cb, ob, col, row, ca, oa, matrix=S, gap_open=4, gap_extend=1, mode=mode, ends=False)
        assert (wrong != exp[0]).any(), "the matrix matters"


@functools.lru_cache(maxsize=None)
def _range_end_stores():
    """Shorter sides of 1 .. 300 characters, none a multiple of 32 or 64 (so rows of the pad class lie beside real rows that score -128),
    against longer sides of m, m + 3 and m + 40, related (3 %) and unrelated, every second pair with the shorter side in store B."""
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
    lut, nchars = _lut(tok)
    S = align.score_matrix(tok, 127, -128)
    (ca, oa, cb, ob, row, col), meta = _range_end_stores()
    exp = twin.score_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, gaps[0], gaps[1], mode)
    assert exp[0].max() > 127 * 200 and (mode == "local" or exp[0].min() < -128 * 30)
    kw = dict(matrix=S, gap_open=gaps[0], gap_extend=gaps[1], mode=mode)
    _same(align.score_pairs_host(tok, ca, oa, row, col, cb, ob, ends=True, **kw), exp, meta)
    for form in (2, 3):
        _same(_device(gpu, tok, ca, oa, row, col, cb, ob, max_len=300, form=form, **kw), exp, meta)
    small = np.array([k for k, (m, n) in enumerate(meta) if min(m, n) <= 256], np.int64)
    _same(_device(gpu, tok, ca, oa, row[small], col[small], cb, ob, max_len=256, form=1, **kw), (exp[0][small], exp[1][small]), [meta[k] for k in small])


def test_ragged_waves_and_guards(gpu, bsq):
    """Form 1: sixteen pairs share a wave, lengths 0 .. 256 mixed, so the groups of a wave finish at different steps; lists that fill a
    wave, leave one ragged and spread over many workgroups, with repeated indices and pairs (i, i), through the C ABI; the guard words
    around score and ends stay, and with ends = NULL nothing but score is written."""
    import torch
    from bioseq_amd import capi
    L = capi.load()
    rng = np.random.default_rng(3)
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    S, o, e = _scoring("DNA4")
    lengths = [0, 1, 2, 63, 64, 65, 128, 255, 256] + rng.integers(0, 257, size=7).tolist()
    rows = [twin.random_row(rng, n, "ACGT") for n in lengths]
    rows += [twin.fit(rng, twin.mutate(rng, rows[k], "ACGT", 0.03), len(rows[k]) + k % 3, "ACGT") for k in range(3, 16, 2)]
    chars, offs = twin.pack(rows)
    B = len(rows)
    known = {}

    def reference(row, col):
        for i, j in zip(row.tolist(), col.tolist()):
            if (i, j) not in known:
                s, en = twin.score_pairs(lut, nchars, chars, offs, chars, offs, [i], [j], S, o, e, "local", max_len=256)
                known[(i, j)] = (int(s[0]), int(en[0, 0]), int(en[0, 1]))
        both = np.array([known[p] for p in zip(row.tolist(), col.tolist())], np.int32)
        return np.ascontiguousarray(both[:, 0]), np.ascontiguousarray(both[:, 1:])

    dc, do = _dev(chars, gpu), _dev(offs, gpu)
    desc, guard = capi.desc_of(tok), 16
    sc = capi.Score(256, 1, 0, o, e)
    np.ctypeslib.as_array(sc.matrix)[:5, :5] = S
    for n_pairs in (1, 15, 17, 65, 1000):
        row, col = rng.integers(0, B, size=n_pairs), rng.integers(0, 10, size=n_pairs)  # (few columns: indices repeat)
        row[::7] = col[::7]  # pairs (i, i)
        exp_s, exp_e = reference(row, col)
        assert n_pairs < 17 or len(set(exp_s.tolist())) > 8
        dr, dl = _dev(row, gpu), _dev(col, gpu)
        for with_ends in (True, False):
            score = torch.full((n_pairs + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
            ends = torch.full((2 * n_pairs + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
            with capi.launching(gpu) as stream:
                capi.check(L.bsq_score_pairs_device(ctypes.byref(desc), dc.data_ptr(), do.data_ptr(), B, dc.data_ptr(), do.data_ptr(), B, dr.data_ptr(),
                                                    dl.data_ptr(), n_pairs, ctypes.byref(sc), score.data_ptr() + 4 * guard,
                                                    ends.data_ptr() + 4 * guard if with_ends else None, stream))
            raw, raw_e = score.cpu().numpy(), ends.cpu().numpy()
            assert (raw[:guard] == 0x5A5A5A5A).all() and (raw[-guard:] == 0x5A5A5A5A).all(), n_pairs
            assert raw[guard:-guard].tobytes() == exp_s.tobytes(), (n_pairs, with_ends)
            if with_ends:
                assert (raw_e[:guard] == 0x5A5A5A5A).all() and (raw_e[-guard:] == 0x5A5A5A5A).all(), n_pairs
                assert raw_e[guard:-guard].tobytes() == exp_e.tobytes(), n_pairs
            else:
                assert (raw_e == 0x5A5A5A5A).all()


def test_codes(gpu, bsq):
    """A shorter side of max_len + 1 gets TOO_LONG between neighbours that stay correct; indices -1, Ba and 2^40 get BAD_INDEX and are
    not followed; a longer side of 2^20 + 1 against one character is TOO_LONG while 2^20 is scored; ends of codes are (-1, -1); an empty
    list and a store without rows."""
    import torch
    from bioseq_amd import align
    rng = np.random.default_rng(5)
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    S, o, e = _scoring("DNA4")
    kw = dict(matrix=S, gap_open=o, gap_extend=e)
    rows = [twin.random_row(rng, n, "ACGT") for n in (99, 100, 101, 300)]
    chars, offs = twin.pack(rows)
    row = np.array([0, 1, 2, 1, 2, 2, -1, 0, 4, 1 << 40, 0, 0], np.int64)
    col = np.array([3, 3, 3, 1, 2, 0, 0, 4, 4, 0, -(1 << 40), 1], np.int64)
    for mode in MODES:
        exp = twin.score_pairs(lut, nchars, chars, offs, chars, offs, row, col, S, o, e, mode, max_len=100)
        assert exp[0][[2, 4]].tolist() == [twin.TOO_LONG] * 2 and exp[0][6:11].tolist() == [twin.BAD_INDEX] * 5 and (exp[0][[0, 1, 3, 5, 11]] > -2**30).all()
        assert (exp[1][[2, 4, 6, 7, 8, 9, 10]] == -1).all() and (exp[1][[0, 1, 3, 5, 11]] >= 0).all()
        _same(align.score_pairs_host(tok, chars, offs, row, col, mode=mode, ends=True, max_len=100, **kw), exp)
        _same(_device(gpu, tok, chars, offs, row, col, mode=mode, max_len=100, **kw), exp)
    big = [np.frombuffer(b"G", np.uint8), twin.random_row(rng, (1 << 20) + 1, "ACGT"), twin.random_row(rng, 1 << 20, "ACGT"), rows[0]]
    chars, offs = twin.pack(big)
    row, col = np.array([0, 1, 3, 0, 3], np.int64), np.array([1, 0, 0, 2, 3], np.int64)
    exp = twin.score_pairs(lut, nchars, chars, offs, chars, offs, row, col, S, o, e, "local", max_len=100)
    assert exp[0].tolist() == [twin.TOO_LONG, twin.TOO_LONG, 2, 2, 198] and exp[1][3].tolist()[0] == 1
    _same(_device(gpu, tok, chars, offs, row, col, max_len=100, **kw), exp)
    empty = torch.zeros(0, dtype=torch.int64, device=gpu)
    s, en = align.score_pairs(tok, _dev(chars, gpu), _dev(offs, gpu), empty, empty, ends=True, **kw)
    assert s.dtype == torch.int32 and s.device == gpu and tuple(s.shape) == (0,) and tuple(en.shape) == (0, 2)
    s, en = align.score_pairs(tok, torch.zeros(0, dtype=torch.uint8, device=gpu), torch.zeros(1, dtype=torch.int64, device=gpu),
                              _dev(np.array([0, 1], np.int64), gpu), _dev(np.array([0, 0], np.int64), gpu), _dev(chars, gpu), _dev(offs, gpu), ends=True, **kw)
    assert s.tolist() == [twin.BAD_INDEX] * 2 and en.tolist() == [[-1, -1]] * 2  # a store without rows


def test_long_text(gpu, bsq):
    """1024 x 20 001 in form 2: 1251 text tiles of 16 columns; 1 x 20 001 and 0 x 20 001 in every form; both modes."""
    rng = np.random.default_rng(11)
    tok = _tok("AMINO20")
    lut, nchars = _lut(tok)
    S, o, e = _scoring("AMINO20")
    letters = LETTERS["AMINO20"]
    short, long_ = twin.related_pair(rng, 1024, 20001, letters, rate=0.04)
    long_ = np.concatenate([long_[12000:], long_[:12000]])  # the related part far into the text
    chars, offs = twin.pack([short, long_, np.frombuffer(b"W", np.uint8), np.zeros(0, np.uint8)])
    row, col = np.array([0, 1, 2, 1, 3, 1], np.int64), np.array([1, 0, 1, 2, 1, 3], np.int64)
    for mode in MODES:
        exp = twin.score_pairs(lut, nchars, chars, offs, chars, offs, row, col, S, o, e, mode)
        if mode == "local":
            assert exp[0][0] > 2000 and exp[1][0, 1] > 8000 and exp[0][2] == 11 and exp[0][4] == 0
        _same(_device(gpu, tok, chars, offs, row, col, matrix=S, gap_open=o, gap_extend=e, mode=mode, max_len=1024, form=2), exp)
        for form in (1, 2, 3):
            got = _device(gpu, tok, chars, offs, row[2:], col[2:], matrix=S, gap_open=o, gap_extend=e, mode=mode, max_len=16, form=form)
            _same(got, (exp[0][2:], exp[1][2:]))


def test_unmapped_bytes(gpu, bsq):
    """N, '-', lower case and bytes >= 0x80 in DNA4: one unmapped class, scored by its own row and column of the matrix."""
    from bioseq_amd import align
    rng = np.random.default_rng(13)
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    S = np.array(_scoring("DNA4")[0])
    S[4, :4], S[:4, 4], S[4, 4] = -1, -2, 1  # (the unmapped class told apart from the letters, and A's side from B's)
    pool = np.frombuffer(b"ACGTacgtNNn--\x80\xc3\xff", np.uint8)
    rows = [pool[rng.integers(0, pool.size, size=n)] for n in (5, 64, 65, 130, 200, 257, 300)]
    rows += [np.frombuffer(b"ACNNGT", np.uint8), np.frombuffer(b"ac-\xffgt", np.uint8), np.frombuffer(b"ACANGT", np.uint8)]
    chars, offs = twin.pack(rows)
    row, col = [a.ravel().astype(np.int64) for a in np.meshgrid(np.arange(10), np.arange(10), indexing="ij")]
    for mode in MODES:
        exp = twin.score_pairs(lut, nchars, chars, offs, chars, offs, row, col, S, 5, 2, mode)
        assert exp[0][7 * 10 + 8] == exp[0][7 * 10 + 7] == 10
        _same(align.score_pairs_host(tok, chars, offs, row, col, matrix=S, gap_open=5, gap_extend=2, mode=mode, ends=True), exp)
        _same(_device(gpu, tok, chars, offs, row, col, matrix=S, gap_open=5, gap_extend=2, mode=mode), exp)
        _same(_device(gpu, tok, chars, offs, row, col, matrix=S, gap_open=5, gap_extend=2, mode=mode, max_len=300, form=2), exp)


def test_surface_on_a_side_stream(gpu, bsq):
    """verify_score_pairs == verify_score_pairs_host on a stream that is not the default one, self_scores against the numpy sum, the
    kernel names, and what the device call refuses."""
    import torch
    from bioseq_amd import align
    rng = np.random.default_rng(21)
    tok = _tok("AMINO20")
    lut, nchars = _lut(tok)
    S, o, e = _scoring("AMINO20")
    letters = LETTERS["AMINO20"]
    rows = [twin.random_row(rng, n, letters) for n in (150, 150, 0, 0, 90, 700)]
    rows += [twin.fit(rng, twin.mutate(rng, rows[0], letters, rate), 150, letters) for rate in (0.0, 0.02, 0.05, 0.1, 0.2, 0.3)]
    rows.append(np.frombuffer(b"XXXXXX--", np.uint8))  # a negative self-score
    chars, offs = twin.pack(rows)
    row = np.array([0, 0, 0, 0, 0, 0, 0, 2, 2, 4, 5, 5, -1, 0, 12, 12], np.int64)
    col = np.array([6, 7, 8, 9, 10, 11, 1, 3, 0, 5, 5, 0, 0, 13, 12, 0], np.int64)
    kw = dict(matrix=S, gap_open=o, gap_extend=e, max_len=600)
    keep_h, score_h = align.verify_score_pairs_host(tok, chars, offs, row, col, min_ratio=0.5, **kw)
    assert keep_h[0] and not keep_h[6] and not keep_h[7] and score_h[10] == twin.TOO_LONG and score_h[12:14].tolist() == [twin.BAD_INDEX] * 2
    assert 0 < keep_h[:6].sum() < 6 and not keep_h[14]
    selfs = twin.self_scores(lut, nchars, chars, offs, S)
    assert selfs[12] < 0 and selfs[2] == 0
    exp = twin.score_pairs(lut, nchars, chars, offs, chars, offs, row, col, S, o, e, "local", max_len=600)[0]
    sa, sb = selfs[np.clip(row, 0, 12)], selfs[np.clip(col, 0, 12)]
    ok = exp > -2**30
    assert score_h.tobytes() == exp.tobytes() and keep_h[ok].tolist() == twin.keeps(exp[ok], sa[ok], sb[ok], 0.5).tolist() and not keep_h[~ok].any()
    dc, do, dr, dl = _dev(chars, gpu), _dev(offs, gpu), _dev(row, gpu), _dev(col, gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        keep, score = align.verify_score_pairs(tok, dc, do, dr, dl, min_ratio=0.5, **kw)
        mine = align.self_scores(tok, dc, do, S)
    side.synchronize()
    assert keep.dtype == torch.bool and score.dtype == torch.int32 and keep.device == gpu and mine.dtype == torch.int64 and mine.device == gpu
    assert score.cpu().numpy().tobytes() == score_h.tobytes() and keep.cpu().numpy().tobytes() == keep_h.tobytes()
    assert mine.cpu().numpy().tolist() == selfs.tolist() == align.self_scores(tok, chars, offs, S).tolist()
    for T, least in ((0.0, 1), (0.3, 1), (0.9, 1), (1.0, 1), (0.0, 400), (0.0, 0)):
        for mode in MODES:
            a = align.verify_score_pairs(tok, dc, do, dr, dl, min_ratio=T, min_score=least, mode=mode, **kw)[0].cpu().numpy()
            b = align.verify_score_pairs_host(tok, chars, offs, row, col, min_ratio=T, min_score=least, mode=mode, **kw)[0]
            assert a.tobytes() == b.tobytes(), (T, least, mode)
    two = align.verify_score_pairs(tok, dc, do, dr[:12], dl[:12], dc, do, min_ratio=0.5, **kw)[0].cpu().numpy()
    assert two.tobytes() == keep_h[:12].tobytes(), "two stores"
    assert [align.score_kernel_name(mode=m, ends=en, max_len=n) for m, en, n in (("local", False, 100), ("local", True, 600), ("global", True, 4096))] == \
        ["k_score_pairs<4, local>", "k_score_pairs<16, local+ends>", "k_score_pairs<64, global>"]
    assert align.score_kernel_name(max_len=100, form=3) == "k_score_pairs<64, local>" and align.score_kernel_name(max_len=257, form=1) == ""
    with pytest.raises(ValueError):
        align.score_pairs(tok, chars, offs, row, col, **kw)  # numpy arrays are the host twin's
    with pytest.raises(ValueError):
        align.score_pairs(tok, dc, do, dr.to(torch.int32), dl, **kw)
    for bad_row, bad_col in ((torch.stack([dr, dr], 1)[:, 0], dl), (dr, dl[:-1])):  # a row that is not contiguous; two lengths
        with pytest.raises(ValueError):
            align.score_pairs(tok, dc, do, bad_row, bad_col, **kw)
    with pytest.raises(ValueError):
        align.score_pairs(tok, dc, do, dr, dl, matrix=S, gap_open=128, gap_extend=1)
    with pytest.raises(ValueError):
        align.verify_score_pairs(tok, dc, do, dr, dl, min_ratio=1.1, **kw)


@functools.lru_cache(maxsize=None)
def _pipeline_rows():
    """300 AMINO20 rows of 120 residues, the last 20 mutated copies (substitution, insertion and deletion at 8 % each) of earlier ones."""
    rng = np.random.default_rng(6)
    letters = LETTERS["AMINO20"]
    rows = [twin.random_row(rng, 120, letters) for _ in range(280)]
    rows += [twin.fit(rng, twin.mutate(rng, rows[7 * k], letters, 0.08), 120, letters) for k in range(20)]
    return twin.pack(rows)


def test_sketches_to_score_verified_clusters(gpu, bsq):
    """minhash_packed -> sketch_pairs(low threshold) -> verify_score_pairs -> cluster_pairs gives the labels the twin gives over the same
    candidates; the seed is one at which candidates are both kept and rejected (chosen on the CPU with the twin)."""
    from bioseq_amd import align, sketch
    tok = _tok("AMINO20")
    lut, nchars = _lut(tok)
    S, o, e = _scoring("AMINO20")
    chars, offs = _pipeline_rows()
    dc, do = _dev(chars, gpu), _dev(offs, gpu)
    sk = sketch.minhash_packed(tok, dc, do, 3, 128)
    row, col, *_ = sketch.sketch_pairs(sk, min_jaccard=0.04)
    keep, score = align.verify_score_pairs(tok, dc, do, row, col, matrix=S, gap_open=o, gap_extend=e, min_ratio=0.5, max_len=120)
    labels = sketch.cluster_pairs(row[keep].contiguous(), col[keep].contiguous(), 300)
    r, c = row.cpu().numpy(), col.cpu().numpy()
    exp = twin.score_pairs(lut, nchars, chars, offs, chars, offs, r, c, S, o, e, "local", max_len=120)[0]
    selfs = twin.self_scores(lut, nchars, chars, offs, S)
    passed = twin.keeps(exp, selfs[r], selfs[c], 0.5)
    assert score.cpu().numpy().tobytes() == exp.tobytes() and keep.cpu().numpy().tobytes() == passed.tobytes()
    assert passed.any() and not passed.all(), "a candidate kept and a candidate rejected"
    want = sketch.cluster_pairs_host(r[passed], c[passed], 300)
    assert labels.cpu().numpy().tobytes() == want.tobytes() and 0 < (want != np.arange(300)).sum() <= 20
