"""CPU: sequence packing (include/bsq.h, "sequence packing") -- the library's host twins bsq_pack_plan_host / bsq_pack_tokenize_host
against the numpy twin (tests/pack_twin.py) byte for byte, known answers typed out here, the properties of the specification, the
device plan's parallel arithmetic (csrc/bsq_pack_dev.h, run on the host) against the sequential loop, the rows = N rule, the argument
rules and the dataset keyword.  No device is needed."""
import ctypes
import itertools

import numpy as np
import pytest

import pack_twin as twin

SEQS = [b"ACG", b"", b"AC", b"ACGTAC", b"T"]
FLAGS = list(itertools.product((0, 1), repeat=3))  # (bos, eos, padchar)
PADLENS = (1, 15, 16, 17, 100, 1000)
MODES = ("nextfit", "stream")
GUARD = 64
DESTCHARS = "bhiqfd"


def _lib():
    from bioseq_amd import capi
    return capi, capi.load()


def _tok(key, flags):
    import bioseq_amd
    bos, eos, pad = flags
    return bioseq_amd.Tokenizer(key, bool(eos), bool(bos), bool(pad))


def _pack(seqs, lead=b"", tail=b""):
    chars = np.frombuffer(lead + b"".join(seqs) + tail, dtype=np.uint8).copy()
    offs = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=offs[1:])
    return chars, offs + len(lead)


def _guarded(nbytes, fill):
    raw = np.full(nbytes + 2 * GUARD, fill, dtype=np.uint8)
    return raw, raw[GUARD:GUARD + nbytes]


def _intact(raw, nbytes, fill):
    return bool((raw[:GUARD] == fill).all() and (raw[GUARD + nbytes:] == fill).all())


def _host(key, flags, chars, offs, P, mode, dt, rows=None, seg=True, pos=True, fill=0xAB):
    """bsq_pack_plan_host + bsq_pack_tokenize_host into buffers pre-filled with `fill` bytes (a sentinel no output holds), guard
    bytes on both sides of every output: (tokens, seg, pos, starts, n_rows, n_placed, guards intact)."""
    capi, L = _lib()
    bos, eos, pad = flags
    d = capi.make_desc(key, eos=eos, bos=bos, padchar=pad)
    B = len(offs) - 1
    code = capi.PACK_NEXTFIT if mode == "nextfit" else capi.PACK_STREAM
    sraw, sbuf = _guarded((B + 1) * 8, fill)
    n_rows, n_placed = ctypes.c_int64(-7), ctypes.c_int64(-7)
    assert L.bsq_pack_plan_host(offs.ctypes.data, B, P, bos, eos, code, rows or 0, sbuf.ctypes.data, ctypes.addressof(n_rows),
                                ctypes.addressof(n_placed)) == capi.OK
    starts = sbuf.view(np.int64)
    R = n_rows.value if rows is None else rows
    np_t = twin.NP_DTYPES[dt]
    nt = R * P * np.dtype(np_t).itemsize
    traw, tbuf = _guarded(nt, fill)
    graw, gbuf = _guarded(R * P * 4, fill)
    praw, pbuf = _guarded(R * P * 4, fill)
    keep = chars if chars.size else np.zeros(16, np.uint8)
    st = L.bsq_pack_tokenize_host(ctypes.byref(d), keep.ctypes.data, offs.ctypes.data, B, starts.ctypes.data, R, P, dt, tbuf.ctypes.data,
                                  gbuf.ctypes.data if seg else None, pbuf.ctypes.data if pos else None)
    assert st == capi.OK, L.bsq_last_error()
    intact = _intact(sraw, (B + 1) * 8, fill) and _intact(traw, nt, fill) and _intact(graw, R * P * 4, fill) and _intact(praw, R * P * 4, fill)
    return (tbuf.view(np_t).reshape(R, P), gbuf.view(np.int32).reshape(R, P), pbuf.view(np.int32).reshape(R, P), starts.copy(),
            n_rows.value, n_placed.value, intact)


def test_new_symbols_are_declared_and_exported():
    capi, L = _lib()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_pack_plan_device", "bsq_pack_plan_host", "bsq_pack_plan_parallel_host", "bsq_pack_tokenize_device",
              "bsq_pack_tokenize_host", "bsq_pack_kernel_name"):
        assert n in names and hasattr(L, n), n
    assert L.bsq_abi_version() == 7
    import bioseq_amd
    assert bioseq_amd.packing.pack_tokenize_packed and "packing" in bioseq_amd.__all__


# DNA4: A C G T = 0 1 2 3; with all three flags BOS = 4, EOS = 5, PAD = 6.  Worked out by hand from the rules of the header, P = 8.
def _known(flags, mode):
    bos, eos, pad = flags
    ids = {"A": 0, "C": 1, "G": 2, "T": 3}
    nxt = 4
    BOS = EOS = None
    if bos:
        BOS, nxt = nxt, nxt + 1
    if eos:
        EOS, nxt = nxt, nxt + 1
    PAD = nxt if pad else 0
    P = 8
    runs = [([BOS] if bos else []) + [ids[c] for c in s.decode()] + ([EOS] if eos else []) for s in SEQS]
    rows, seg, pos = [[]], [[]], [[]]
    first = 0
    starts = []
    if mode == "nextfit":
        for i, r in enumerate(runs):
            if i > 0 and len(rows[-1]) + len(r) > P:
                rows.append([]), seg.append([]), pos.append([])
                first = i
            starts.append((len(rows) - 1) * P + len(rows[-1]))
            rows[-1] += r
            seg[-1] += [1 + i - first] * len(r)
            pos[-1] += list(range(len(r)))
    else:
        for i, r in enumerate(runs):
            starts.append((len(rows) - 1) * P + len(rows[-1]))
            for k, t in enumerate(r):
                if len(rows[-1]) == P:
                    rows.append([]), seg.append([]), pos.append([])
                    first = i
                rows[-1].append(t), seg[-1].append(1 + i - first), pos[-1].append(k)
    starts.append((len(rows) - 1) * P + len(rows[-1]))
    for a, fill in ((rows, PAD), (seg, 0), (pos, 0)):
        for r in a:
            r += [fill] * (P - len(r))
    return np.array(rows), np.array(seg), np.array(pos), starts


TYPED = {  # (flags, mode) -> starts | tokens / segment_ids / position_ids, typed out
    ((0, 0, 0), "nextfit"): ([0, 3, 3, 8, 14, 15], ["0 1 2 0 1 0 0 0", "0 1 2 3 0 1 3 0"], ["1 1 1 3 3 0 0 0", "1 1 1 1 1 1 2 0"],
                             ["0 1 2 0 1 0 0 0", "0 1 2 3 4 5 0 0"]),
    ((0, 0, 0), "stream"): ([0, 3, 3, 5, 11, 12], ["0 1 2 0 1 0 1 2", "3 0 1 3 0 0 0 0"], ["1 1 1 3 3 4 4 4", "1 1 1 2 0 0 0 0"],
                            ["0 1 2 0 1 0 1 2", "3 4 5 0 0 0 0 0"]),
    ((1, 1, 1), "nextfit"): ([0, 5, 8, 16, 24, 27], ["4 0 1 2 5 4 5 6", "4 0 1 5 6 6 6 6", "4 0 1 2 3 0 1 5", "4 3 5 6 6 6 6 6"],
                             ["1 1 1 1 1 2 2 0", "1 1 1 1 0 0 0 0", "1 1 1 1 1 1 1 1", "1 1 1 0 0 0 0 0"],
                             ["0 1 2 3 4 0 1 0", "0 1 2 3 0 0 0 0", "0 1 2 3 4 5 6 7", "0 1 2 0 0 0 0 0"]),
    ((1, 1, 1), "stream"): ([0, 5, 7, 11, 19, 22], ["4 0 1 2 5 4 5 4", "0 1 5 4 0 1 2 3", "0 1 5 4 3 5 6 6"],
                            ["1 1 1 1 1 2 2 3", "1 1 1 2 2 2 2 2", "1 1 1 2 2 2 0 0"], ["0 1 2 3 4 0 1 0", "1 2 3 0 1 2 3 4", "5 6 7 0 1 2 0 0"]),
    ((1, 0, 0), "nextfit"): ([0, 4, 5, 8, 16, 18], ["4 0 1 2 4 4 0 1", "4 0 1 2 3 0 1 0", "4 3 0 0 0 0 0 0"],
                             ["1 1 1 1 2 3 3 3", "1 1 1 1 1 1 1 0", "1 1 0 0 0 0 0 0"], ["0 1 2 3 0 0 1 2", "0 1 2 3 4 5 6 0", "0 1 0 0 0 0 0 0"]),
    ((0, 1, 1), "nextfit"): ([0, 4, 5, 8, 16, 18], ["0 1 2 4 4 0 1 4", "0 1 2 3 0 1 4 5", "3 4 5 5 5 5 5 5"],
                             ["1 1 1 1 2 3 3 3", "1 1 1 1 1 1 1 0", "1 1 0 0 0 0 0 0"], ["0 1 2 3 0 0 1 2", "0 1 2 3 4 5 6 0", "0 1 0 0 0 0 0 0"]),
}


def _mat(rows):
    return np.array([[int(x) for x in r.split()] for r in rows], dtype=np.int64)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("mode", MODES)
def test_known_answers_of_the_specification(flags, mode):
    capi, _ = _lib()
    chars, offs = _pack(SEQS)
    tok, seg, pos, starts, n_rows, n_placed, intact = _host("DNA4", flags, chars, offs, 8, mode, capi.U64)
    w_tok, w_seg, w_pos, w_starts = _known(flags, mode)
    assert intact and n_placed == 5 and n_rows == len(w_tok)
    assert starts.tolist() == w_starts
    assert np.array_equal(tok.astype(np.int64), w_tok) and np.array_equal(seg, w_seg) and np.array_equal(pos, w_pos)
    if (flags, mode) in TYPED:
        t_starts, t_tok, t_seg, t_pos = TYPED[(flags, mode)]
        assert starts.tolist() == t_starts
        assert np.array_equal(tok.astype(np.int64), _mat(t_tok)) and np.array_equal(seg, _mat(t_seg)) and np.array_equal(pos, _mat(t_pos))
    t = twin.pack("DNA4", flags, chars, offs, 8, mode)
    assert np.array_equal(t[0], w_tok) and np.array_equal(t[1], w_seg) and np.array_equal(t[2], w_pos) and t[3].tolist() == w_starts


def _batches(rng, P, be):
    """Batches that hit the edges at width P: random lengths, runs exactly P wide and one token wider, empty sequences, all-empty, B = 0."""
    pool = np.frombuffer(b"ACGTACGTACGTNacgt*\xff", dtype=np.uint8)
    full = max(P - be, 0)

    def seqs(lens):
        return [bytes(rng.choice(pool, int(n))) for n in lens]

    yield "random", seqs(rng.integers(0, max(2, min(P, 70)) + 1, 23))
    yield "exact", seqs([full, 3, 0, full, full, 1, max(full - 1, 0), 1])
    yield "wider", seqs([2, full + 1, 0, 1, full + 1, full + 5, 0])
    yield "empty", seqs([0] * 9)
    yield "none", []


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", PADLENS)
def test_host_twins_equal_the_numpy_twin(mode, P):
    capi, _ = _lib()
    rng = np.random.default_rng(17 * P + len(mode))
    n = 0
    for flags in FLAGS:
        be = flags[0] + flags[1]
        for name, seqs in _batches(rng, P, be):
            chars, offs = _pack(seqs, lead=b"\xffGGGG", tail=b"TTTT\xff")  # offsets[0] = 5, junk either side
            for key in (("DNA4", "AMINO20") if name == "random" else ("DNA4",)):
                want = twin.pack(key, flags, chars, offs, P, mode)
                for dt in range(6):
                    tok, seg, pos, starts, n_rows, n_placed, intact = _host(key, flags, chars, offs, P, mode, dt, fill=0xAB if dt < 4 else 0xFF)
                    assert intact, (name, flags, dt)
                    assert starts.tolist() == want[3].tolist() and n_rows == want[4] and n_placed == len(seqs), (name, flags)
                    assert tok.tobytes() == want[0].astype(twin.NP_DTYPES[dt]).tobytes(), (name, flags, dt)
                    assert seg.tobytes() == want[1].tobytes() and pos.tobytes() == want[2].tobytes(), (name, flags, dt)
                    n += 1
    assert n > 0


@pytest.mark.parametrize("mode", MODES)
def test_properties_of_the_specification(mode):
    """The unpack identity, no split in next-fit, the flat concatenation in stream mode, the segment and position rules and every
    element written once (the outputs are pre-filled with 0xAB bytes: no id, segment or position of these batches is 0xABAB...)."""
    capi, _ = _lib()
    rng = np.random.default_rng(5)
    for flags, P in itertools.product(FLAGS, (16, 33, 100)):
        be = flags[0] + flags[1]
        seqs = [bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), int(n))) for n in rng.integers(0, P - be + 1, 60)]
        chars, offs = _pack(seqs)
        tok, seg, pos, starts, n_rows, _, intact = _host("DNA4", flags, chars, offs, P, mode, capi.I32)
        assert intact
        for a in (tok, seg, pos):
            assert not (a.view(np.uint8).reshape(-1, 4) == 0xAB).all(axis=1).any()  # every element was written
        runs = twin.runs("DNA4", flags, chars, offs)
        flat, fseg, fpos = tok.reshape(-1), seg.reshape(-1), pos.reshape(-1)
        covered = np.zeros(flat.size, dtype=bool)
        for i, run in enumerate(runs):
            s, w = int(starts[i]), len(run)
            assert np.array_equal(flat[s:s + w], run)  # the unpack identity
            assert np.array_equal(fpos[s:s + w], np.arange(w))
            assert not covered[s:s + w].any()
            covered[s:s + w] = True
            if mode == "nextfit" and w:
                assert s // P == (s + w - 1) // P
                assert (fseg[s:s + w] == fseg[s]).all() and fseg[s] >= 1
        assert int(starts[-1]) == (int(starts[len(seqs) - 1]) + len(runs[-1]))
        assert (flat[~covered] == twin.pad_value("DNA4", flags)).all() and (fseg[~covered] == 0).all() and (fpos[~covered] == 0).all()
        assert (fseg[covered] >= 1).all()
        if mode == "stream":
            cat = np.concatenate(runs) if runs else np.zeros(0, np.int64)
            assert np.array_equal(flat[:cat.size], cat) and not covered[cat.size:].any() and n_rows == max(1, -(-cat.size // P))
            assert (seg[:, 0][covered.reshape(-1, P)[:, 0]] == 1).all()  # whatever covers column 0 is segment 1 of its row
        # segments count sequences: inside a row the ids of consecutive covered positions differ by the difference of their sequences
        cover = np.full(flat.size, -1)
        for i, run in enumerate(runs):
            cover[int(starts[i]):int(starts[i]) + len(run)] = i
        c2, s2 = cover.reshape(-1, P), seg
        for r in range(c2.shape[0]):
            m = c2[r] >= 0
            if m.any():
                assert np.array_equal(s2[r][m] - s2[r][m][0], c2[r][m] - c2[r][m][0]) and s2[r][m][0] == 1 + c2[r][m][0] - c2[r][0]


@pytest.mark.parametrize("seed, n, lo, hi, P, flags", [(1, 262144, 0, 1022, 1024, (1, 1, 1)), (2, 100000, 140, 160, 1024, (1, 1, 0)),
                                                       (3, 65536, 50, 1022, 2048, (0, 0, 0)), (4, 5000, 0, 3, 1, (0, 0, 0)),
                                                       (5, 4097, 0, 14, 16, (1, 0, 0)), (6, 1, 5, 5, 16, (1, 1, 1)), (7, 70000, 0, 0, 7, (0, 0, 0))])
def test_parallel_plan_arithmetic_equals_the_sequential_loop(seed, n, lo, hi, P, flags):
    from bioseq_amd import packing, synth
    lens = synth.synth_lengths(seed, n, lo, hi)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    offs += 11
    tok = _tok("DNA4", flags)
    for mode in MODES:
        for rows in (None, 3, 1000):
            a = packing.pack_plan_host(tok, offs, P, mode, rows)
            b = packing.pack_plan_host(tok, offs, P, mode, rows, parallel=True)
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], (mode, rows)
    if n <= 5000:  # and both equal the twin's loop
        for mode in MODES:
            t = twin.plan(offs, P, flags[0], flags[1], mode)
            a = packing.pack_plan_host(tok, offs, P, mode)
            assert np.array_equal(a[0], t[0]) and a[1:] == t[1:]


def test_a_run_wider_than_the_row_without_validation():
    """Next-fit: it has its row to itself and is cut at P positions; the parallel plan agrees."""
    from bioseq_amd import packing
    tok = _tok("DNA4", (1, 1, 1))
    chars, offs = _pack([b"AC", b"ACGTACGTACGT", b"", b"A", b"ACGTACGTAC"])
    r = packing.pack_tokenize_host(tok, chars, offs, 8, "i")
    assert r.starts.tolist() == [0, 8, 16, 18, 24, 32] and r.n_rows == 4
    assert r.tokens.tolist() == [[4, 0, 1, 5, 6, 6, 6, 6], [4, 0, 1, 2, 3, 0, 1, 2], [4, 5, 4, 0, 5, 6, 6, 6], [4, 0, 1, 2, 3, 0, 1, 2]]
    assert r.position_ids[1].tolist() == list(range(8)) and r.segment_ids[2].tolist() == [1, 1, 2, 2, 2, 0, 0, 0]
    assert np.array_equal(packing.pack_plan_host(tok, offs, 8, "nextfit", parallel=True)[0], r.starts)
    t = twin.pack("DNA4", (1, 1, 1), chars, offs, 8, "nextfit", dtype=np.int32)
    assert np.array_equal(t[0], r.tokens) and np.array_equal(t[1], r.segment_ids) and np.array_equal(t[2], r.position_ids)


@pytest.mark.parametrize("mode", MODES)
def test_rows_n_places_a_prefix(mode):
    from bioseq_amd import packing
    rng = np.random.default_rng(3)
    flags = (1, 1, 1)
    tok = _tok("DNA4", flags)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(n))) for n in rng.integers(0, 30, 40)]
    chars, offs = _pack(seqs)
    P = 32
    whole = packing.pack_tokenize_host(tok, chars, offs, P, "h", mode=mode)
    need = whole.n_rows
    assert need > 4
    for N in (1, 2, need - 1, need, need + 3):
        r = packing.pack_tokenize_host(tok, chars, offs, P, "h", mode=mode, rows=N)
        t = twin.pack("DNA4", flags, chars, offs, P, mode, rows=N, dtype=np.int16)
        assert r.tokens.shape == (N, P) and r.n_rows == need and r.n_placed == t[5]
        assert np.array_equal(r.starts, t[3]) and np.array_equal(r.tokens, t[0]) and np.array_equal(r.segment_ids, t[1])
        assert np.array_equal(r.position_ids, t[2])
        k = r.n_placed
        assert (r.starts[:k] >= 0).all() and (r.starts[k:-1] == -1).all()
        if N >= need:
            assert k == len(seqs) and np.array_equal(r.tokens[:need], whole.tokens) and (r.tokens[need:] == 6).all()
            assert (r.segment_ids[need:] == 0).all()
        else:
            assert 0 < k < len(seqs)
            # the placed runs are where the whole plan has them, they end inside the matrix, the next one would not
            assert np.array_equal(r.starts[:k], whole.starts[:k])
            w = np.diff(offs) + 2
            assert whole.starts[k - 1] + w[k - 1] <= N * P < whole.starts[k] + w[k]
            flat = r.tokens.reshape(-1)
            assert (flat[int(r.starts[-1]):] == 6).all() and np.array_equal(flat[:int(r.starts[-1])], whole.tokens.reshape(-1)[:int(r.starts[-1])])
            # resuming at n_placed packs the rest
            rest = packing.pack_tokenize_host(tok, chars, offs[k:], P, "h", mode=mode)
            assert rest.starts[0] == 0 and rest.tokens[0, 0] == 4
    assert packing.pack_rows_bound(int(offs[-1] - offs[0]), len(seqs), P, tok, mode) >= need


def test_rows_bound_is_safe():
    from bioseq_amd import packing, synth
    for seed, (lo, hi), flags, P in itertools.product((1, 2, 3), ((0, 5), (20, 62), (62, 62), (1, 1)), ((0, 0, 0), (1, 1, 1)), (64, 100)):
        tok = _tok("DNA4", flags)
        lens = synth.synth_lengths(seed, 500, lo, hi)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        for mode in MODES:
            assert packing.pack_rows_bound(int(offs[-1]), 500, P, tok, mode) >= packing.pack_plan_host(tok, offs, P, mode)[1]
    assert packing.pack_rows_bound(0, 0, 64, _tok("DNA4", (0, 0, 0))) == 0


def test_argument_rules_nothing_written():
    capi, L = _lib()
    from bioseq_amd import packing
    chars, offs = _pack(SEQS)
    d = capi.make_desc("DNA4", 1, 1, 1)
    starts = np.full(6, 0x5A5A, dtype=np.int64)
    n_rows = ctypes.c_int64(-7)
    base = dict(offs=offs.ctypes.data, B=5, P=8, bos=1, eos=1, mode=1, max_rows=0, starts=starts.ctypes.data, n_rows=ctypes.addressof(n_rows))

    def plan(fn, **kw):
        a = dict(base, **kw)
        args = [a["offs"], a["B"], a["P"], a["bos"], a["eos"], a["mode"], a["max_rows"], a["starts"], a["n_rows"], None]
        return fn(*args, None) if fn is L.bsq_pack_plan_device else fn(*args)

    for fn in (L.bsq_pack_plan_host, L.bsq_pack_plan_parallel_host, L.bsq_pack_plan_device):
        for kw in ({"offs": None}, {"B": -1}, {"P": 0}, {"P": -3}, {"P": 2 ** 30 + 1}, {"bos": 2}, {"eos": -1}, {"mode": 2}, {"mode": -1},
                   {"max_rows": -1}, {"starts": None}, {"n_rows": None}, {"B": 2 ** 31}):
            assert plan(fn, **kw) == capi.ERR_INVALID_ARG, kw
        assert (starts == 0x5A5A).all() and n_rows.value == -7 and L.bsq_last_error() != b""
    tokens = np.full(64, 0xAB, dtype=np.uint8)
    ok_starts = packing.pack_plan_host(_tok("DNA4", (1, 1, 1)), offs, 8)[0]
    tb = dict(d=ctypes.byref(d), chars=chars.ctypes.data, offs=offs.ctypes.data, B=5, starts=ok_starts.ctypes.data, rows=1, P=8, dt=capi.I8,
              tokens=tokens.ctypes.data)

    def enc(dev, **kw):
        a = dict(tb, **kw)
        args = [a["d"], a["chars"], a["offs"], a["B"], a["starts"], a["rows"], a["P"], a["dt"], a["tokens"], None, None]
        return L.bsq_pack_tokenize_device(*args, None) if dev else L.bsq_pack_tokenize_host(*args)

    for dev in (False, True):
        for kw in ({"d": None}, {"chars": None}, {"offs": None}, {"starts": None}, {"tokens": None}, {"B": -1}, {"rows": -1}, {"P": 0},
                   {"rows": 2 ** 31 + 1}, {"rows": 2 ** 31, "P": 2 ** 10}):
            assert enc(dev, **kw) == capi.ERR_INVALID_ARG, (dev, kw)
        for dt in (-1, 6):
            assert enc(dev, dt=dt) == capi.ERR_DTYPE
        assert enc(dev, rows=0) == capi.OK  # nothing to write, nothing launched
        assert (tokens == 0xAB).all()
    if L.bsq_device_count() == 0:
        assert enc(True) == capi.ERR_NO_DEVICE or enc(True) == capi.ERR_HIP
    assert L.bsq_pack_kernel_name(ctypes.byref(d), 5, 4, 8, capi.I8) == b"k_pack_flat<perm>"
    assert L.bsq_pack_kernel_name(ctypes.byref(capi.make_desc("BYTES")), 5, 4, 8, capi.U64) == b"k_pack_flat<lut>"
    assert L.bsq_pack_kernel_name(ctypes.byref(d), 5, 4, 0, capi.I8) == b"" and L.bsq_pack_kernel_name(None, 5, 4, 8, capi.I8) == b""
    # the Python layer: ValueError before any device work
    tok = _tok("DNA4", (1, 1, 1))
    for kw in (dict(mode="bestfit"), dict(padlen=0), dict(padlen=-4), dict(rows=0), dict(rows=-2), dict(padlen=2 ** 30 + 1)):
        a = dict(dict(padlen=8, mode="nextfit", rows=None), **kw)
        with pytest.raises(ValueError):
            packing.pack_tokenize_host(tok, chars, offs, a["padlen"], mode=a["mode"], rows=a["rows"])
        with pytest.raises(ValueError):
            packing.pack_tokenize_packed(tok, chars, offs, a["padlen"], mode=a["mode"], rows=a["rows"])
        with pytest.raises(ValueError):
            packing.pack_plan(tok, chars, offs, a["padlen"], mode=a["mode"], rows=a["rows"])
    with pytest.raises(ValueError):
        packing.pack_tokenize_packed(tok, chars, offs, 8)  # host arrays: the device call takes resident batches
    with pytest.raises(ValueError):
        packing.pack_rows_bound(-1, 5, 8, tok)
    assert packing.pack_cu_seqlens(np.array([0, 3, 9], dtype=np.int64)).dtype == np.int32
    assert packing.pack_kernel_name(tok, 100, 10, 1024, "q") == "k_pack_flat<perm>"


def test_dataset_keyword_without_a_device(tmp_path):
    import bioseq_amd
    from bioseq_amd.flatfile import FlatFile, write_flatfile
    from bioseq_amd.loaders import FlatFileDataset
    ff = FlatFile(write_flatfile([b"ACGTACGTACGT", b"ACG", b""], str(tmp_path / "p.ff")))
    tok = bioseq_amd.Tokenizer("DNA4", True, True, True)
    for mode in MODES:
        for kw in ({"cnn": True}, {"augment": 1}, {"masked": True}, {"kmer": 3}):
            with pytest.raises(ValueError):
                FlatFileDataset(ff, tok, device="cpu", pack=mode, **kw)
        ds = FlatFileDataset(ff, tok, device="cpu", pack=mode)
        assert ds.max_seq_len == 14 and ds.pack == mode
        with pytest.raises(ValueError):
            next(iter(ds.batches(2, shuffle=False, group=2)))
        assert FlatFileDataset(ff, tok, device="cpu", pack=mode, crop=8, revcomp_frac=0.5).max_seq_len == 10
    with pytest.raises(ValueError):
        FlatFileDataset(ff, tok, device="cpu", pack="bestfit")
    assert FlatFileDataset(ff, tok, device="cpu").pack is None  # (off by default)
