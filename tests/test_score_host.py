"""CPU: the scored alignment of row pairs (include/bsq.h, "scored alignment of row pairs") -- the declared symbols, the header's known
answers, the row-vectorised numpy twin of tests/score_twin.py against its cell-by-cell version, the library's host twin
bsq_score_pairs_host against the twin on generated pairs, the equivalence with the edit distance, the symmetry under an asymmetric
matrix, BLOSUM62 over AMINO20, codes, every refusal and the verification rule at its exact boundary.  No device is needed."""
import ctypes

import numpy as np
import pytest

import edit_twin
import score_twin as twin

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


def test_new_symbols_are_declared_and_exported():
    import bioseq_amd.align as align
    from bioseq_amd import capi
    L = capi.load()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_score_pairs_device", "bsq_score_pairs_host", "bsq_score_pairs_kernel_name", "bsq_blosum62_scores"):
        assert n in names and hasattr(L, n), n
    assert L.bsq_abi_version() == 7 and ctypes.sizeof(capi.Score) == 20 + 32 * 32
    for n in ("score_matrix", "blosum62_matrix", "score_pairs", "score_pairs_host", "score_kernel_name", "self_scores", "verify_score_pairs",
              "verify_score_pairs_host"):
        assert n in align.__all__ and callable(getattr(align, n))
    assert (align.SCORE_TOO_LONG, align.SCORE_BAD_INDEX, align.CODE_BELOW) == (-2**31 + 1, -2**31 + 2, -2**30)


def test_known_answers_dna4():
    """The answers of include/bsq.h from the cell twin, the row twin and the host twin."""
    from bioseq_amd import align
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    chars, offs = _rows(BATCH)
    row, col = _grid(5)
    S = align.score_matrix(tok, 2, -3)
    assert S.shape == (5, 5) and S.dtype == np.int8 and S[4, 4] == 2 and S[0, 4] == -3
    want_global = [12, -2, -9, -17, -20, -2, 16, -13, -21, -23, -9, -13, 4, -9, -21, -17, -21, -9, 0, -19, -20, -23, -21, -19, 14]
    want_local = [(12, 6, 6), (8, 4, 8), (4, 2, 2), (0, 0, 0), (2, 4, 1), (8, 8, 4), (16, 8, 8), (4, 2, 2), (0, 0, 0), (2, 8, 1),
                  (4, 2, 2), (4, 2, 2), (4, 2, 2), (0, 0, 0), (0, 0, 0)] + [(0, 0, 0)] * 5 + [(2, 1, 4), (2, 1, 8), (0, 0, 0), (0, 0, 0), (14, 7, 7)]
    lengths = np.diff(offs)
    for one in (twin.gotoh_cells, twin.gotoh):
        s, e = twin.score_pairs(lut, nchars, chars, offs, chars, offs, row, col, S, 5, 2, "global", one=one)
        assert s.tolist() == want_global and e[:, 0].tolist() == lengths[row].tolist() and e[:, 1].tolist() == lengths[col].tolist()
        s, e = twin.score_pairs(lut, nchars, chars, offs, chars, offs, row, col, S, 5, 2, "local", one=one)
        assert [(int(a), int(b), int(c)) for a, (b, c) in zip(s, e)] == want_local
    s, e = align.score_pairs_host(tok, chars, offs, row, col, matrix=S, gap_open=5, gap_extend=2, mode="global", ends=True)
    assert s.dtype == np.int32 and e.dtype == np.int32 and e.shape == (25, 2)
    assert s.tolist() == want_global and e[:, 0].tolist() == lengths[row].tolist() and e[:, 1].tolist() == lengths[col].tolist()
    s, e = align.score_pairs_host(tok, chars, offs, row, col, matrix=S, gap_open=5, gap_extend=2, ends=True)
    assert [(int(a), int(b), int(c)) for a, (b, c) in zip(s, e)] == want_local
    assert align.score_pairs_host(tok, chars, offs, row, col, matrix=S, gap_open=5, gap_extend=2).tolist() == [w[0] for w in want_local]
    # the unit-cost edit distance: 0 / -1, {0, 1}, global
    unit = align.score_matrix(tok, 0, -1)
    dist = [0, 3, 4, 6, 6, 3, 0, 6, 8, 7, 4, 6, 0, 2, 7, 6, 8, 2, 0, 7, 6, 7, 7, 7, 0]
    assert (-align.score_pairs_host(tok, chars, offs, row, col, matrix=unit, gap_open=0, gap_extend=1, mode="global")).tolist() == dist
    assert align.edit_distance_host(tok, chars, offs, row, col).tolist() == dist


def test_known_answers_blosum62():
    from bioseq_amd import align
    tok = _tok("AMINO20")
    lut, nchars = _lut(tok)
    ca, oa = _rows([b"HEAGAWGHEE"])
    cb, ob = _rows([b"PAWHEAE"])
    z = np.zeros(1, np.int64)
    S = align.blosum62_matrix(tok)
    for (o, e), local, ends, glob in (((11, 1), 17, (3, 6), 1), ((0, 8), 20, (9, 5), -8)):
        for one in (twin.gotoh_cells, twin.gotoh):
            s, en = twin.score_pairs(lut, nchars, ca, oa, cb, ob, z, z, S, o, e, "local", one=one)
            assert (int(s[0]), tuple(en[0])) == (local, ends)
            assert twin.score_pairs(lut, nchars, ca, oa, cb, ob, z, z, S, o, e, "global", one=one)[0].tolist() == [glob]
        s, en = align.score_pairs_host(tok, ca, oa, z, z, cb, ob, matrix=S, gap_open=o, gap_extend=e, ends=True)
        assert (int(s[0]), tuple(en[0])) == (local, ends)
        s, en = align.score_pairs_host(tok, cb, ob, z, z, ca, oa, matrix=S, gap_open=o, gap_extend=e, ends=True)
        assert (int(s[0]), tuple(en[0])) == (local, ends[::-1]), "swapping the stores swaps the ends"
        assert align.score_pairs_host(tok, ca, oa, z, z, cb, ob, matrix=S, gap_open=o, gap_extend=e, mode="global").tolist() == [glob]
    assert align.self_scores(tok, ca, oa, S).tolist() == [62] and align.self_scores(tok, cb, ob, S).tolist() == [44]
    assert twin.self_scores(lut, nchars, ca, oa, S).tolist() == [62]


def test_row_twin_equals_cell_twin():
    """Small random cases over three classes (many ties), gap costs with e = 0 and o = 0 among them, asymmetric matrices, both modes."""
    rng = np.random.default_rng(17)
    n = 0
    for _ in range(150):
        la, lb = rng.integers(0, 14, size=2)
        x, y = rng.integers(0, 3, size=la), rng.integers(0, 3, size=lb)
        S = rng.integers(-4, 5, size=(3, 3))
        o, e = [(0, 0), (0, 1), (3, 0), (5, 2), (11, 1)][rng.integers(0, 5)]
        for mode in MODES:
            a, b = twin.gotoh(x, y, S, o, e, mode), twin.gotoh_cells(x, y, S, o, e, mode)
            assert a == b, (x, y, S, o, e, mode)
            n += a[3] > 1
    assert n > 20, "cases where several cells reach the maximum"


@pytest.mark.parametrize("key", ["DNA4", "AMINO20"])
def test_host_twin_equals_the_twin(key):
    """Generated pairs around the block edges, the shorter side in either store; score and ends byte for byte, every form."""
    from bioseq_amd import align
    tok = _tok(key)
    lut, nchars = _lut(tok)
    pairs = edit_twin.cases(len(key) * 5 + 2, LETTERS[key], lengths=(0, 1, 2, 7, 63, 64, 65, 129))
    for k in range(1, len(pairs), 3):
        pairs[k] = pairs[k][::-1]
    ca, oa, cb, ob, row, col = twin.store_of(pairs)
    S, o, e = (align.blosum62_matrix(tok), 11, 1) if key == "AMINO20" else (align.score_matrix(tok, 2, -3), 5, 2)
    for mode in MODES:
        exp_s, exp_e = twin.score_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, o, e, mode)
        got_s, got_e = align.score_pairs_host(tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=o, gap_extend=e, mode=mode, ends=True)
        assert got_s.tobytes() == exp_s.tobytes() and got_e.tobytes() == exp_e.tobytes(), mode
        assert len(set(exp_s.tolist())) > len(pairs) // 4
        for form in (1, 2, 3):  # (checked, and changes nothing on the host)
            assert align.score_pairs_host(tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=o, gap_extend=e, mode=mode, max_len=256,
                                          form=form).tobytes() == exp_s.tobytes()
    unit = align.score_matrix(tok, 0, -1)
    glob = align.score_pairs_host(tok, ca, oa, row, col, cb, ob, matrix=unit, gap_open=0, gap_extend=1, mode="global")
    assert (-glob).tobytes() == align.edit_distance_host(tok, ca, oa, row, col, cb, ob).tobytes()


def test_asymmetric_matrix_and_swapped_stores():
    """score(A, B; S) == score(B, A; S transposed) for a matrix that is not symmetric; the ends are swapped wherever one cell alone
    reaches the maximum (among several, each call takes the smallest end of ITS store A first)."""
    from bioseq_amd import align
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    rng = np.random.default_rng(23)
    S = rng.integers(-6, 7, size=(5, 5)).astype(np.int8)
    S[np.arange(5), np.arange(5)] = rng.integers(1, 7, size=5)
    assert (S != S.T).any()
    pool = "ACGTN"
    pairs = []
    for m, n in ((5, 9), (9, 5), (64, 70), (70, 64), (65, 65), (130, 40), (0, 4), (4, 0)):
        x = twin.random_row(rng, m, pool)
        pairs.append((x, twin.fit(rng, twin.mutate(rng, x, pool, 0.1), n, pool)))
    ca, oa, cb, ob, row, col = twin.store_of(pairs)
    for mode in MODES:
        exp_s, exp_e = twin.score_pairs(lut, nchars, ca, oa, cb, ob, row, col, S, 4, 1, mode)
        s1, e1 = align.score_pairs_host(tok, ca, oa, row, col, cb, ob, matrix=S, gap_open=4, gap_extend=1, mode=mode, ends=True)
        s2, e2 = align.score_pairs_host(tok, cb, ob, col, row, ca, oa, matrix=np.ascontiguousarray(S.T), gap_open=4, gap_extend=1, mode=mode, ends=True)
        assert s1.tobytes() == exp_s.tobytes() and e1.tobytes() == exp_e.tobytes()
        back_s, back_e = twin.score_pairs(lut, nchars, cb, ob, ca, oa, col, row, S.T, 4, 1, mode)
        assert s2.tobytes() == exp_s.tobytes() == back_s.tobytes() and e2.tobytes() == back_e.tobytes()
        single = np.array([twin.gotoh(twin.classes(lut, nchars, x), twin.classes(lut, nchars, y), S, 4, 1, mode)[3] == 1 for x, y in pairs])
        assert single.sum() >= 3 and (e2[single][:, ::-1] == exp_e[single]).all(), "one best cell: swapping the stores swaps the ends"
        wrong = align.score_pairs_host(tok, cb, ob, col, row, ca, oa, matrix=S, gap_open=4, gap_extend=1, mode=mode)
        assert (wrong != exp_s).any(), "the matrix matters: not transposing it changes a score"


def test_blosum62_matrix():
    from bioseq_amd import align, capi
    tok = _tok("AMINO20")
    lut, nchars = _lut(tok)
    S = align.blosum62_matrix(tok)
    assert S.shape == (21, 21) and S.dtype == np.int8 and (S == S.T).all()
    raw = np.zeros((21, 21), np.int8)
    capi.check(capi.load().bsq_blosum62_scores(raw.ctypes.data))
    order = "ARNDCQEGHILKMFPSTWYV"
    assert (raw == raw.T).all() and raw[20, 20] == -1 and raw[0, 0] == 4 and raw[17, 17] == 11 and raw[4, 20] == -2 and raw[17, 4] == -2

    def at(a, b):
        return int(S[lut[ord(a)], lut[ord(b)]])

    assert (at("W", "W"), at("I", "V"), at("W", "P"), at("A", "A"), at("C", "C"), at("H", "Y")) == (11, 3, -4, 4, 9, 2)
    for a in order:
        for b in order:
            assert at(a, b) == raw[order.index(a), order.index(b)]
        assert int(S[lut[ord(a)], 20]) == raw[order.index(a), 20] == int(S[20, lut[ord(a)]])
    assert S[20, 20] == -1
    assert capi.load().bsq_blosum62_scores(None) == capi.ERR_INVALID_ARG
    for key in ("DNA4", "BYTES"):
        with pytest.raises(ValueError):
            align.blosum62_matrix(_tok(key))


def test_codes_and_refusals():
    from bioseq_amd import align, capi
    tok = _tok("DNA4")
    rng = np.random.default_rng(5)
    rows = [twin.random_row(rng, n, "ACGT") for n in (100, 101, 102, 300)]
    chars, offs = twin.pack(rows)
    lut, nchars = _lut(tok)
    S = align.score_matrix(tok, 2, -3)
    kw = dict(matrix=S, gap_open=5, gap_extend=2)
    row = np.array([0, 1, 2, 1, 3, 2, -1, 0, 4, 1 << 40, 0], np.int64)
    col = np.array([3, 3, 3, 1, 3, 0, 0, 4, 4, 0, -(1 << 40)], np.int64)
    for mode in MODES:
        exp_s, exp_e = twin.score_pairs(lut, nchars, chars, offs, chars, offs, row, col, S, 5, 2, mode, max_len=100)
        assert exp_s[1:5].tolist() == [twin.TOO_LONG] * 4 and exp_s[6:].tolist() == [twin.BAD_INDEX] * 5 and (exp_e[1:5] == -1).all() and (exp_e[6:] == -1).all()
        assert exp_s[0] > -2**30 and exp_s[5] > -2**30 and (exp_e[[0, 5]] >= 0).all()
        got_s, got_e = align.score_pairs_host(tok, chars, offs, row, col, mode=mode, ends=True, max_len=100, **kw)
        assert got_s.tobytes() == exp_s.tobytes() and got_e.tobytes() == exp_e.tobytes()
    assert (twin.TOO_LONG, twin.BAD_INDEX) == (align.SCORE_TOO_LONG, align.SCORE_BAD_INDEX)
    empty = np.zeros(0, np.int64)
    s, e = align.score_pairs_host(tok, chars, offs, empty, empty, ends=True, **kw)
    assert s.shape == (0,) and e.shape == (0, 2)
    assert align.score_pairs_host(tok, np.zeros(0, np.uint8), np.zeros(1, np.int64), row[:2], col[:2], **kw).tolist() == [twin.BAD_INDEX] * 2
    row, col = np.array([0, 1, 2], np.int64), np.array([1, 2, 3], np.int64)
    for bad in ({"max_len": 0}, {"max_len": 4097}, {"max_len": 2.5}, {"max_len": 257, "form": 1}, {"max_len": 1025, "form": 2}, {"form": 4},
                {"form": -1}, {"form": True}, {"mode": "semi"}, {"mode": 0}, {"gap_open": -1}, {"gap_open": 128}, {"gap_extend": -1},
                {"gap_extend": 128}, {"gap_open": 1.5}, {"gap_extend": True}, {"matrix": S[:4, :4]}, {"matrix": S.astype(np.float32)},
                {"matrix": S.astype(np.int32) * 100}, {"matrix": np.zeros((21, 21), np.int8)}):
        with pytest.raises(ValueError):
            align.score_pairs_host(tok, chars, offs, row, col, **{**kw, **bad})
    with pytest.raises(ValueError):
        align.score_pairs_host(_tok("BYTES"), chars, offs, row, col, matrix=np.zeros((257, 257), np.int8), gap_open=1, gap_extend=1)
    with pytest.raises(ValueError):
        align.score_pairs_host(tok, chars, offs, row.astype(np.int32), col, **kw)
    with pytest.raises(ValueError):
        align.score_pairs_host(tok, chars, offs, row, col[:2], **kw)
    with pytest.raises(ValueError):
        align.score_pairs_host(tok, chars, offs, row, col, chars_b=chars, **kw)
    with pytest.raises(ValueError):
        align.score_matrix(tok, 200, 0)
    with pytest.raises(ValueError):
        align.self_scores(tok, chars, offs, S[:4, :4])
    for bad in ({"min_ratio": -0.1}, {"min_ratio": 1.5}, {"min_ratio": float("nan")}, {"min_score": 1.5}):
        with pytest.raises(ValueError):
            align.verify_score_pairs_host(tok, chars, offs, row, col, **kw, **bad)
    names = [align.score_kernel_name(mode=m, ends=e, max_len=n) for m, e, n in (("local", False, 256), ("local", True, 257), ("global", False, 4096),
                                                                                   ("global", True, 1024))]
    assert names == ["k_score_pairs<4, local>", "k_score_pairs<16, local+ends>", "k_score_pairs<64, global>", "k_score_pairs<16, global>"]
    assert align.score_kernel_name(max_len=100, form=3) == "k_score_pairs<64, local>"
    assert align.score_kernel_name(max_len=257, form=1) == "" and align.score_kernel_name(mode="semi") == "" and align.score_kernel_name(gap_open=128) == ""
    # the C ABI itself: a refusal writes nothing and leaves a reason
    L = capi.load()
    desc = capi.desc_of(tok)
    score, ends = np.full(3, 7, np.int32), np.full(6, 7, np.int32)

    def call(s, chars_p=chars.ctypes.data, Ba=4, row_p=row.ctypes.data, n=3, d=desc, score_p=score.ctypes.data):
        return L.bsq_score_pairs_host(ctypes.byref(d) if d is not None else None, chars_p, offs.ctypes.data, Ba, chars.ctypes.data, offs.ctypes.data, 4, row_p,
                                      col.ctypes.data, n, ctypes.byref(s) if s is not None else None, score_p, ends.ctypes.data)

    good = capi.Score(4096, 0, 0, 5, 2)
    np.ctypeslib.as_array(good.matrix)[:5, :5] = S
    for field, value in (("max_len", 0), ("max_len", 4097), ("form", 4), ("form", -1), ("mode", 2), ("mode", -1), ("gap_open", 128), ("gap_open", -1),
                         ("gap_extend", 128), ("gap_extend", -1)):
        s = capi.Score.from_buffer_copy(good)
        setattr(s, field, value)
        assert call(s) == capi.ERR_INVALID_ARG and L.bsq_last_error() and (score == 7).all() and (ends == 7).all(), (field, value)
        assert L.bsq_score_pairs_kernel_name(ctypes.byref(s), 1) == b""
    s = capi.Score.from_buffer_copy(good)
    s.max_len, s.form = 257, 1
    assert call(s) == capi.ERR_INVALID_ARG
    assert call(None) == capi.ERR_INVALID_ARG and L.bsq_score_pairs_kernel_name(None, 0) == b""
    assert call(good, d=capi.desc_of(_tok("BYTES"))) == capi.ERR_INVALID_ARG
    for bad in ({"chars_p": None}, {"Ba": -1}, {"row_p": None}, {"n": -1}, {"score_p": None}, {"d": None}):
        assert call(good, **bad) == capi.ERR_INVALID_ARG and (score == 7).all() and (ends == 7).all(), bad
    assert L.bsq_score_pairs_host(ctypes.byref(desc), None, None, 0, None, None, 0, None, None, 0, ctypes.byref(good), None, None) == capi.OK
    assert call(good) == capi.OK and score.tolist() == align.score_pairs_host(tok, chars, offs, row, col, **kw).tolist() and (ends >= 0).all()
    # entries of the matrix at an index > nchars are not read
    np.ctypeslib.as_array(good.matrix)[5:, :] = 99
    np.ctypeslib.as_array(good.matrix)[:, 5:] = 99
    again = score.copy()
    assert call(good) == capi.OK and score.tolist() == again.tolist()


def test_verification_rule_at_its_exact_boundary():
    """+2 / -3, {5, 2}: a 128-character row against a copy with k substitutions spread out scores 2 (128 - k) - 3 k locally... not
    exactly (an alignment may stop short), so the thresholds are taken from the pair's own score: T chosen so that score * 65536 ==
    T * least passes, and one step beyond fails."""
    from bioseq_amd import align
    tok = _tok("DNA4")
    lut, nchars = _lut(tok)
    S = align.score_matrix(tok, 2, -3)
    base = np.frombuffer(b"ACGT" * 32, np.uint8)
    x = base.copy()
    x[8:8 + 4 * 16:4] = ord("T")  # 16 substitutions of A by T
    rows = [base, x, base[:64], np.zeros(0, np.uint8), np.frombuffer(b"NNNN", np.uint8)]
    chars, offs = twin.pack(rows)
    row, col = np.array([0, 0, 0, 3, 0, 9, 4], np.int64), np.array([1, 2, 3, 3, 0, 0, 4], np.int64)
    kw = dict(matrix=S, gap_open=5, gap_extend=2)
    score, _ = twin.score_pairs(lut, nchars, chars, offs, chars, offs, row, col, S, 5, 2, "local")
    selfs = twin.self_scores(lut, nchars, chars, offs, S)
    assert selfs.tolist() == [256, 256, 128, 0, 8] and align.self_scores(tok, chars, offs, S).tolist() == selfs.tolist()
    assert score.tolist() == [176, 128, 0, 0, 256, twin.BAD_INDEX, 8]  # 2 * 112 - 3 * 16 = 176
    assert 176 * 65536 == 45056 * 256  # the ratio 0.6875 is a 16-bit fraction: T = 45056 sits exactly on it
    keep, got = align.verify_score_pairs_host(tok, chars, offs, row, col, min_ratio=0.6875, **kw)
    assert got.tobytes() == score.tobytes() and keep.dtype == np.bool_
    assert keep.tolist() == [True, True, False, False, True, False, True]
    sa, sb = selfs[np.clip(row, 0, 4)], selfs[col]
    assert keep[:5].tolist() == twin.keeps(score[:5], sa[:5], sb[:5], 0.6875).tolist()
    one_beyond = 45057 / 65536
    assert align.verify_score_pairs_host(tok, chars, offs, row, col, min_ratio=one_beyond, **kw)[0].tolist() == [False, True, False, False, True, False, True]
    assert align.verify_score_pairs_host(tok, chars, offs, row, col, min_ratio=0.0, **kw)[0].tolist() == [True, True, False, False, True, False, True]
    assert align.verify_score_pairs_host(tok, chars, offs, row, col, min_ratio=0.0, min_score=0, **kw)[0].tolist() == [True, True, False, False, True, False, True]  # (an empty row: least = 0)
    assert align.verify_score_pairs_host(tok, chars, offs, row, col, min_ratio=0.0, min_score=177, **kw)[0].tolist() == [False] * 4 + [True, False, False]
    assert align.verify_score_pairs_host(tok, chars, offs, row, col, min_ratio=1.0, **kw)[0].tolist() == [False, True, False, False, True, False, True]
    assert align.verify_score_pairs_host(tok, chars, offs, row, col, min_ratio=0.5, max_len=100, **kw)[0].tolist() == [False, True, False, False, False, False, True]
