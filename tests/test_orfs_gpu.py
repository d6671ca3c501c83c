"""GPU: ORF extraction (bioseq_amd.orfs, bsq_orf_count_device / bsq_orf_emit_device) bit for bit against the numpy twin
(tests/orf_twin.py) -- the row edges around the walk's pieces, the start mode, every launch class, a six-frame batch whose filter both
keeps and drops, max_orfs cuts behind poisoned entries and guards, a side stream --, and the whole pipeline on a DNA store against
translate_twin + orf_twin + row slicing, with the tokens of the ORF batch."""
import ctypes

import numpy as np
import pytest

import orf_twin as twin
import translate_twin

pytestmark = pytest.mark.gpu

GUARD = 256
POISON = -7777


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _store(chars, offs, gpu):
    """(device chars, device offsets, n_rows) of a host batch; an empty batch gets the 16-byte stand-in the wrappers use."""
    ch = chars if chars.size else np.zeros(16, np.uint8)
    return _dev(ch, gpu), _dev(offs, gpu), offs.size - 1


def _raw(gpu, store, stop, start, min_len, max_orfs=None, stream=None, want_residues=True):
    """bsq_orf_count_device + bsq_orf_emit_device into arrays that sit between GUARD poisoned entries, with the entries past max_orfs
    poisoned too: (row, start, length, orf_offsets, residues) on the host, the arrays whole up to max_orfs.  Checks the guards and
    that nothing at or past max_orfs was written.  max_orfs None: the count, read back."""
    import torch
    from bioseq_amd import capi
    L = capi.load()
    dch, dof, n = store
    rule = capi.Orf(stop, start, min_len)
    s = ctypes.c_void_p(stream.cuda_stream if stream is not None else capi.raw_stream(gpu))
    offs_buf = torch.full((n + 1 + 2 * GUARD,), POISON, dtype=torch.int64, device=gpu)
    res = torch.full((1 + 2 * GUARD,), POISON, dtype=torch.int64, device=gpu)
    orf_offs = offs_buf[GUARD:GUARD + n + 1]
    capi.check(L.bsq_orf_count_device(dch.data_ptr(), dof.data_ptr(), n, ctypes.byref(rule), orf_offs.data_ptr(),
                                      res[GUARD:].data_ptr() if want_residues else None, s))
    if max_orfs is None:
        torch.cuda.synchronize()
        max_orfs = int(orf_offs[-1].item())
    tail = 64
    out = [torch.full((max_orfs + tail + 2 * GUARD,), POISON, dtype=torch.int64, device=gpu) for _ in range(3)]
    capi.check(L.bsq_orf_emit_device(dch.data_ptr(), dof.data_ptr(), n, ctypes.byref(rule), orf_offs.data_ptr(), max_orfs,
                                     out[0][GUARD:].data_ptr(), out[1][GUARD:].data_ptr(), out[2][GUARD:].data_ptr(), s))
    torch.cuda.synchronize()
    host = [a.cpu().numpy() for a in out]
    for a in host:
        assert (a[:GUARD] == POISON).all() and (a[GUARD + max_orfs:] == POISON).all(), "an entry outside [0, max_orfs) was written"
    ob, rb = offs_buf.cpu().numpy(), res.cpu().numpy()
    assert (ob[:GUARD] == POISON).all() and (ob[GUARD + n + 1:] == POISON).all(), "a guard entry of orf_offsets was overwritten"
    assert (rb[:GUARD] == POISON).all() and (rb[GUARD + 1:] == POISON).all() and (want_residues or rb[GUARD] == POISON)
    return [a[GUARD:GUARD + max_orfs] for a in host] + [ob[GUARD:GUARD + n + 1], int(rb[GUARD])]


def _same(got, exp, cut=None):
    """got = (row, start, length, orf_offsets, residues) against the twin's; cut: the arrays hold max_orfs = cut entries."""
    k = exp[0].size if cut is None else min(cut, exp[0].size)
    assert np.array_equal(got[3], exp[3]) and got[4] == exp[4]
    for a, b in zip(got[:3], exp[:3]):
        assert a.size == (exp[0].size if cut is None else cut)
        assert np.array_equal(a[:k], b[:k]) and (a[k:] == POISON).all()


@pytest.fixture(scope="module")
def hand(gpu):
    """The hand-made rows per min_len, on the host and the device."""
    out = {}
    for ml in (1, 5, 30):
        chars, offs = twin.hand_rows(ml)
        out[ml] = (chars, offs, _store(chars, offs, gpu))
    return out


@pytest.mark.parametrize("start", [-1, ord("M")])
@pytest.mark.parametrize("min_len", [1, 5, 30])
def test_row_edges_and_start_mode_on_hand_rows(gpu, hand, min_len, start):
    """Rows of 0 .. 5000 residues around the piece (64) and the round (256), stops at 0, at the end, in runs, at both sides of a piece
    edge, segments of min_len and min_len - 1, M first / last / carried / deciding from the piece before (orf_twin.hand_rows)."""
    chars, offs, store = hand[min_len]
    exp = twin.find(chars, offs, ord("*"), start, min_len)
    assert exp[0].size > 20 and (np.diff(exp[3]) == 0).any() and (np.diff(exp[3]) > 1).any()
    _same(_raw(gpu, store, ord("*"), start, min_len), exp)


def test_every_length_around_the_pieces_every_alignment(gpu):
    """Every row length 0 .. 330 twice (rows back to back: every alignment of a row's first byte modulo 16), noise with a stop every
    ~20 residues, and stop / start bytes that a register nobody loaded would hold (NUL) or that fill a byte (0xFF)."""
    rng = np.random.default_rng(7)
    lens = np.concatenate([np.arange(331), np.arange(331)[::-1]])
    offs = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = rng.choice(np.frombuffer(b"AAAAAAAAAAAAAAACDEFGHIKLMX*\x00\xff", np.uint8), int(offs[-1])).astype(np.uint8)
    store = _store(chars, offs, gpu)
    for stop, start, ml in ((ord("*"), -1, 1), (ord("*"), ord("M"), 5), (0, 0xFF, 1), (0xFF, 0, 3), (0, -1, 30)):
        _same(_raw(gpu, store, stop, start, ml), twin.find(chars, offs, stop, start, ml))


def _short_rows(n, seed):
    """n rows of 0 .. 3 residues (row i: i % 4), one residue in four a stop."""
    rng = np.random.default_rng(seed)
    lens = np.arange(n, dtype=np.int64) % 4
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = rng.choice(np.frombuffer(b"AM**KKLV", np.uint8), int(offs[-1])).astype(np.uint8)
    return chars, offs


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_launch_classes_few_rows(gpu, n):
    """No rows, one row, a partial / whole / second workgroup of 64 rows, and more rows than any loader batch."""
    from bioseq_amd import orfs
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 200, n)
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = rng.choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY*", np.uint8), int(offs[-1])).astype(np.uint8)
    assert orfs.kernel_name(n) == ("hipMemsetAsync" if n == 0 else "k_orf_count+k_orf_offsets;k_orf_emit")
    store = _store(chars, offs, gpu)
    for start, ml in ((-1, 5), (ord("M"), 1)):
        _same(_raw(gpu, store, ord("*"), start, ml), twin.find(chars, offs, ord("*"), start, ml))
    if n == 0:
        got = _raw(gpu, store, ord("*"), -1, 1, want_residues=False)
        assert got[3].tolist() == [0]


@pytest.mark.parametrize("n", [2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1])
def test_launch_class_boundary_at_2_pow_20_rows(gpu, n):
    """The two sides of the scanned class: rows of 0 .. 3 residues, min_len 1, so that ORFs are many and every prefix matters."""
    from bioseq_amd import orfs
    chars, offs = _short_rows(n, n)
    assert orfs.kernel_name(n) == ("k_orf_count+k_orf_offsets;k_orf_emit" if n <= 2 ** 20 else "k_orf_count+k_orf_scan+k_orf_offsets;k_orf_emit")
    exp = twin.find(chars, offs, ord("*"), -1, 1)
    assert exp[0].size > n // 2
    _same(_raw(gpu, _store(chars, offs, gpu), ord("*"), -1, 1), exp)


def test_scanned_class_beyond_2_pow_20_rows(gpu):
    """The class beyond 2^20 rows (k_orf_count + k_orf_scan + k_orf_offsets<true>): 2^20 + 65 rows of 0 .. 3 residues with min_len 1,
    so the last workgroup is partial and the last entry of the scanned sums is the sum of one row -- against the library's host twin
    (the form of test_scanned_place_beyond_2_pow_20_rows), and the host twin against the numpy twin."""
    from bioseq_amd import orfs
    n = 2 ** 20 + 65
    chars, offs = _short_rows(n, 20)
    assert orfs.kernel_name(n) == "k_orf_count+k_orf_scan+k_orf_offsets;k_orf_emit"
    dch, dof, _ = _store(chars, offs, gpu)
    for start in (None, "M"):
        e_row, e_start, e_len, e_offs = orfs.find_orfs_host(chars, offs, min_len=1, start=start)
        t = twin.find(chars, offs, ord("*"), -1 if start is None else ord("M"), 1)
        assert np.array_equal(e_offs, t[3]) and np.array_equal(e_row, t[0]) and np.array_equal(e_start, t[1]) and np.array_equal(e_len, t[2])
        assert e_offs.size == n + 1 and e_row.size == int(e_offs[-1]) > (n // 4 if start is None else 1000)
        row, o_start, o_len, orf_offs = orfs.find_orfs_packed(dch, dof, min_len=1, start=start)
        assert np.array_equal(orf_offs.cpu().numpy(), e_offs)
        assert np.array_equal(row.cpu().numpy(), e_row) and np.array_equal(o_start.cpu().numpy(), e_start) and np.array_equal(o_len.cpu().numpy(), e_len)


@pytest.fixture(scope="module")
def mix(gpu):
    p_chars, p_offs = twin.batch_mix()
    return p_chars, p_offs, _store(p_chars, p_offs, gpu), twin.find(p_chars, p_offs, ord("*"), -1, 30)


def test_batch_mix_six_frames_min_len_30(gpu, mix):
    """Uniform ACGT in six frames: the twin keeps and drops at least 100 segments each, so neither side of the filter is vacuous."""
    p_chars, p_offs, store, exp = mix
    accepted, rejected = twin.segments(p_chars, p_offs, ord("*"), -1, 30)
    assert accepted >= 100 and rejected >= 100 and exp[0].size == accepted
    _same(_raw(gpu, store, ord("*"), -1, 30), exp)
    e = twin.find(p_chars, p_offs, ord("*"), ord("M"), 30)
    assert e[0].size >= 100
    _same(_raw(gpu, store, ord("*"), ord("M"), 30), e)


def test_max_orfs_cuts(gpu, mix):
    """max_orfs equal to the count, one less, a value in the middle of a row's ORFs, and 0: ranks < max_orfs are written, nothing else."""
    p_chars, p_offs, store, exp = mix
    total = exp[0].size
    several = np.nonzero(np.diff(exp[3]) >= 3)[0]
    assert several.size
    mid = int(exp[3][several[several.size // 2]]) + 1  # behind the first ORF of a row that has three
    assert exp[0][mid - 1] == exp[0][mid] == exp[0][mid + 1]
    for cap in (total, total - 1, mid, 0, total + 50):
        _same(_raw(gpu, store, ord("*"), -1, 30, max_orfs=cap), exp, cut=cap)


def test_side_stream_and_python_api(gpu, mix, hand):
    import torch
    from bioseq_amd import orfs
    p_chars, p_offs, store, exp = mix
    side = torch.cuda.Stream(device=gpu)
    _same(_raw(gpu, store, ord("*"), -1, 30, stream=side), exp)
    _same(_raw(gpu, store, ord("*"), -1, 30, max_orfs=exp[0].size + 7, stream=side), exp, cut=exp[0].size + 7)
    # find_orfs_packed: exact (one read-back) and bounded (none; zeros behind the last ORF, the count tells of a cut)
    dch, dof, _ = store
    got = [a.cpu().numpy() for a in orfs.find_orfs_packed(dch, dof)]
    assert all(np.array_equal(a, b) for a, b in zip(got, exp[:4]))
    total = exp[0].size
    for cap in (total + 9, total // 2, 0):
        got = [a.cpu().numpy() for a in orfs.find_orfs_packed(dch, dof, max_orfs=cap)]
        k = min(cap, total)
        assert np.array_equal(got[3], exp[3]) and all(a.size == cap and np.array_equal(a[:k], b[:k]) and not a[k:].any() for a, b in zip(got, exp[:3]))
    chars, offs, (hch, hof, _) = hand[5]
    with torch.cuda.stream(side):
        got = [a.cpu().numpy() for a in orfs.find_orfs_packed(hch, hof, min_len=5, start="M")]
    e = twin.find(chars, offs, ord("*"), ord("M"), 5)
    assert all(np.array_equal(a, b) for a, b in zip(got, e[:4]))
    got = orfs.find_orfs_packed(hch[:0], hof[:1])
    assert got[3].cpu().tolist() == [0] and got[0].numel() == 0


# ---- end to end on a DNA store ----

PLANTED = b"MKVLAAGIVRESTWYHDEQNCFPMMKLAVGSTRAW"  # 35 residues, no stop


def _back_translate(protein):
    """A DNA sequence that the standard code reads as `protein`: the first codon of each letter in the table's order."""
    tab = translate_twin.table(1)
    return b"".join("".join(translate_twin.NCBI[(int(np.nonzero(tab == c)[0][0]) >> s) & 3] for s in (4, 2, 0)).encode() for c in protein)


@pytest.fixture(scope="module")
def dna(gpu):
    """120 rows of 0 .. 2000 characters drawn like tests/test_translate_gpu.py::_store (unknown codons everywhere); row 17 carries
    TAA + the reverse complement of a planted gene + TTA at nucleotides [100, 100 + 3 * 35 + 6): the ORF lies on its reverse strand."""
    rng = np.random.default_rng(18)
    lens = rng.integers(0, 2001, 120)
    lens[17] = 900
    chars, offs = twin.dna_store(rng, lens)
    gene = b"TAA" + _back_translate(PLANTED) + b"TAA"  # stop, ORF, stop -- on the reverse strand
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    planted = gene.translate(comp)[::-1]
    at = int(offs[17]) + 100
    chars[at:at + len(planted)] = np.frombuffer(planted, np.uint8)
    return chars, offs, lens, (_dev(chars, gpu), _dev(offs, gpu))


def _expected(chars, offs, index, code, frames, tab, stop, start, min_len):
    p_chars, p_offs, _ = translate_twin.translate(chars, offs, index, frame=code, frames=frames, tab=tab)
    e = twin.find(p_chars, p_offs, stop, start, min_len)
    e_chars, e_offs = twin.slices(p_chars, p_offs, e[0], e[1], e[2])
    return e, e_chars, e_offs


@pytest.mark.parametrize("table", [1, 2])
def test_pipeline_frames_and_tables(gpu, dna, table):
    from bioseq_amd import orfs
    chars, offs, lens, (dch, dof) = dna
    rng = np.random.default_rng(table)
    per_row = rng.integers(0, 6, 120).astype(np.uint8)
    tab = translate_twin.table(table)
    for frame, code, frames, start in ((0, 0, None, None), ("six", translate_twin.SIX, None, None), ("six", translate_twin.SIX, None, "M"),
                                       (per_row, 0, per_row, None), (_dev(per_row, gpu), 0, per_row, None)):
        e, e_chars, e_offs = _expected(chars, offs, None, code, frames, tab, ord("*"), -1 if start is None else ord(start), 30)
        assert e[0].size >= 8
        c, o, (src, fc, s, n) = orfs.orfs_packed(dch, dof, frame=frame, table=table, start=start)
        assert np.array_equal(o.cpu().numpy(), e_offs) and c[:int(e_offs[-1])].cpu().numpy().tobytes() == e_chars.tobytes()
        assert np.array_equal(s.cpu().numpy(), e[1]) and np.array_equal(n.cpu().numpy(), e[2])
        if code == translate_twin.SIX:
            assert np.array_equal(src.cpu().numpy(), e[0] // 6) and np.array_equal(fc.cpu().numpy(), e[0] % 6)
        else:
            assert np.array_equal(src.cpu().numpy(), e[0])
            assert np.array_equal(fc.cpu().numpy(), frames[e[0]] if frames is not None else np.full(e[0].size, frame))
    # an index list with repeats, another stop letter
    index = rng.integers(0, 120, 70).astype(np.int64)
    tab2 = tab.copy()
    tab2[tab2 == ord("*")] = ord("$")
    e, e_chars, e_offs = _expected(chars, offs, index, translate_twin.SIX, None, tab2, ord("$"), -1, 20)
    for idx in (list(index), _dev(index, gpu)):
        c, o, origin = orfs.orfs_packed(dch, dof, index=idx, table=table, stop="$", min_len=20)
        assert np.array_equal(o.cpu().numpy(), e_offs) and c[:int(e_offs[-1])].cpu().numpy().tobytes() == e_chars.tobytes()
        assert np.array_equal(origin[0].cpu().numpy(), e[0] // 6)


def test_pipeline_finds_the_planted_reverse_strand_orf(gpu, dna):
    from bioseq_amd import orfs
    chars, offs, lens, (dch, dof) = dna
    c, o, (src, fc, s, n) = orfs.orfs_packed(dch, dof)
    src, fc, s, n, o = (x.cpu().numpy() for x in (src, fc, s, n, o))
    a, b = orfs.orf_spans(lens[src], fc, s, n)
    hit = np.nonzero((src == 17) & (a == 103) & (b == 103 + 3 * len(PLANTED)))[0]
    assert hit.size == 1
    k = int(hit[0])
    assert fc[k] >= 3 and n[k] == len(PLANTED) and c[o[k]:o[k + 1]].cpu().numpy().tobytes() == PLANTED
    assert (900 - 103 - 3 * len(PLANTED)) % 3 == fc[k] - 3
    ta, tb = orfs.orf_spans(_dev(lens[src], gpu), _dev(fc, gpu), _dev(s, gpu), _dev(n, gpu))  # tensors as they come back
    assert np.array_equal(ta.cpu().numpy(), a) and np.array_equal(tb.cpu().numpy(), b)


def test_pipeline_without_read_back_gives_the_same_rows(gpu, dna):
    from bioseq_amd import orfs
    chars, offs, lens, (dch, dof) = dna
    e, e_chars, e_offs = _expected(chars, offs, None, translate_twin.SIX, None, translate_twin.table(1), ord("*"), -1, 30)
    total, nbytes = e[0].size, int(e_offs[-1])
    c, o, (src, fc, s, n) = orfs.orfs_packed(dch, dof, max_orfs=total + 11, capacity=nbytes + 100)
    o = o.cpu().numpy()
    assert o.size == total + 12 and np.array_equal(o[:total + 1], e_offs) and (o[total:] == nbytes).all()  # the rows behind the last ORF are empty
    assert c[:nbytes].cpu().numpy().tobytes() == e_chars.tobytes()
    assert np.array_equal(s.cpu().numpy()[:total], e[1]) and np.array_equal(n.cpu().numpy()[:total], e[2]) and not n.cpu().numpy()[total:].any()
    assert np.array_equal(src.cpu().numpy()[:total], e[0] // 6) and np.array_equal(fc.cpu().numpy()[:total], e[0] % 6)
    # a bound below the count: the first max_orfs ORFs
    c, o, origin = orfs.orfs_packed(dch, dof, max_orfs=total // 2, capacity=nbytes)
    assert np.array_equal(o.cpu().numpy(), e_offs[:total // 2 + 1])
    assert c[:int(e_offs[total // 2])].cpu().numpy().tobytes() == e_chars[:int(e_offs[total // 2])].tobytes()


def test_tokens_of_the_orf_batch(gpu, bsq, dna):
    from bioseq_amd import orfs
    chars, offs, lens, (dch, dof) = dna
    e, e_chars, e_offs = _expected(chars, offs, None, translate_twin.SIX, None, translate_twin.table(1), ord("*"), ord("M"), 30)
    c, o, _ = orfs.orfs_packed(dch, dof, start="M")
    tok = bsq.pbeos_tokenizers["AMINO20"]
    P = int(np.diff(e_offs).max()) + 2
    got = tok.tokenize_packed(c, o, P, "b", True)
    exp = tok.tokenize_packed(_dev(e_chars, gpu), _dev(e_offs, gpu), P, "b", True)
    assert got.shape == (e[0].size, P) and got.cpu().numpy().tobytes() == exp.cpu().numpy().tobytes()
    rows = [bytes(e_chars[e_offs[i]:e_offs[i + 1]]) for i in range(e[0].size)]
    assert got.cpu().numpy().tobytes() == np.ascontiguousarray(tok.batch_tokenize(rows, padlen=P, batch_first=True)).tobytes()
