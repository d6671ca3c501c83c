"""GPU: BPE ids of packed batches (bioseq_amd.bpe, bsq_bpe_tokenize_device) against the library's CPU twin, byte for byte -- tokens and
lengths: row lengths at every lane, 64-position and form edge, both forms on the rows both hold, one to five rows (four per workgroup),
poly-A rows of every length (the run parity across 64-position boundaries), N barriers at those boundaries, a chain table whose every
step fuses one pair, cut rows and P = 1, the (P, B) layout, all six element types, a table whose hash collides, no merges at all, the
outputs of refused calls, and a store that ends at the last byte of its allocation.  tests/test_bpe_host.py holds the twin to the
one-merge-at-a-time rule."""
import ctypes
import functools

import numpy as np
import pytest

import bpe_twin as twin

pytestmark = pytest.mark.gpu

EDGES = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024)
PARITY_MERGES = [("A", "A"), ("AA", "AA"), ("AA", "A")]


def _tok(key="DNA4", eos=False, bos=False, padchar=False):
    import bioseq_amd
    return bioseq_amd.Tokenizer(key, eos, bos, padchar)


@functools.lru_cache(maxsize=None)
def _trained(flags=(False, False, False), key="DNA4", letters="ACGT", n_merges=200):
    from bioseq_amd import bpe
    rng = np.random.default_rng(n_merges)
    rows = [twin.random_row(rng, 300, letters) for _ in range(40)] + [twin.low_complexity_row(rng, 300, letters) for _ in range(20)]
    return bpe.bpe_train_host(_tok(key, *flags), *twin.pack(rows), n_merges)


def _check(gpu, v, rows, P, destchar="i", batch_first=True, **kw):
    """bpe_tokenize_packed on uploaded copies against bpe_tokenize_host; returns the twin's (tokens, lengths)."""
    import torch
    from bioseq_amd import bpe, capi
    chars, offs = twin.pack(rows)
    host_kw = dict(kw)
    if host_kw.get("max_chars") is None:
        host_kw["max_chars"] = 8192 if max(len(r) for r in rows) > 1024 or kw.get("form") == 2 else 1024
    exp_t, exp_l = bpe.bpe_tokenize_host(v, chars, offs, P, destchar, batch_first, **host_kw)
    got_t, got_l = bpe.bpe_tokenize_packed(v, torch.from_numpy(chars).to(gpu), torch.from_numpy(offs).to(gpu), P, destchar, batch_first, **kw)
    assert got_t.device == gpu and got_t.is_contiguous() and got_t.dtype == capi.dtype_of(destchar)[1] and tuple(got_t.shape) == exp_t.shape
    assert got_l.dtype == torch.int32 and tuple(got_l.shape) == (len(rows),)
    assert got_l.cpu().numpy().tobytes() == exp_l.tobytes(), (got_l.cpu().numpy().tolist(), exp_l.tolist())
    assert got_t.cpu().numpy().tobytes() == exp_t.tobytes()
    return exp_t, exp_l


@functools.lru_cache(maxsize=None)
def _edge_rows():
    rng = np.random.default_rng(42)
    rows = []
    for n in EDGES:
        rows += [twin.random_row(rng, n, "ACGT"), twin.random_row(rng, n, "ACGT", 0.02), twin.low_complexity_row(rng, n, "ACGT")]
    return rows


@pytest.mark.parametrize("form", [None, 1, 2])
def test_row_lengths_at_every_edge_in_both_forms(gpu, bsq, form):
    """0 .. 1024 characters: one lane, one row of 64, a second one, sixteen; None and 1 take the wave form, 2 the block form."""
    from bioseq_amd import bpe
    v = _trained()
    exp_t, exp_l = _check(gpu, v, _edge_rows(), 1030, form=form)
    assert bpe.bpe_kernel_name(v, max_chars=1024, form=form) == ("k_bpe_block" if form == 2 else "k_bpe_wave")
    lens = np.array([len(r) for r in _edge_rows()])
    assert (exp_l[lens > 2] < lens[lens > 2]).all() and exp_l[:3].tolist() == [0, 0, 0], "merges fire in every row of three characters or more"


def test_block_form_lengths_and_the_too_long_code(gpu, bsq):
    """1025 and 8192 characters take the block form; 8193 gets -1 and an empty token row, with and without a read-back of the bound."""
    rng = np.random.default_rng(7)
    v = _trained((True, True, True))
    rows = [twin.random_row(rng, n, "ACGT", 0.01) for n in (1025, 8192, 8193, 100, 0, 4097)] + [twin.low_complexity_row(rng, 8192, "ACGT")]
    for kw in (dict(), dict(max_chars=8192)):
        exp_t, exp_l = _check(gpu, v, rows, 3000, "h", **kw)
        assert exp_l[2] == -1 and exp_t[2, :3].tolist() == [v.M + 5, v.M + 6, v.M + 7] and (exp_l[[0, 1, 3, 5, 6]] > 0).all()
    exp_t, exp_l = _check(gpu, v, rows, 16, "h", max_chars=1024)  # the same batch under a smaller bound: four rows are too long
    assert exp_l.tolist()[:3] == [-1, -1, -1] and exp_l[3] > 0 and exp_l[5] == exp_l[6] == -1


def test_max_chars_1024_and_1025_on_one_batch(gpu, bsq):
    from bioseq_amd import bpe
    v = _trained()
    rows = _edge_rows()
    a = _check(gpu, v, rows, 600, max_chars=1024)
    b = _check(gpu, v, rows, 600, max_chars=1025)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert (bpe.bpe_kernel_name(v, max_chars=1024), bpe.bpe_kernel_name(v, max_chars=1025)) == ("k_bpe_wave", "k_bpe_block")


@pytest.mark.parametrize("B", [1, 3, 4, 5])
def test_one_to_five_rows(gpu, bsq, B):
    """Four rows share a workgroup of the wave form: a last workgroup with one, three and four of its waves at work."""
    rng = np.random.default_rng(B)
    rows = [twin.random_row(rng, int(n), "ACGT", 0.02) for n in rng.integers(100, 700, B)]
    for form in (1, 2):
        _check(gpu, _trained(), rows, 400, form=form)


def test_poly_a_rows_of_every_length(gpu, bsq):
    """(A,A), (AA,AA), (AA,A): every candidate mask is one run, so the parity carry crosses every 64-position boundary."""
    from bioseq_amd import bpe
    v = bpe.BPEVocab.from_merges(_tok(), PARITY_MERGES)
    rows = [np.full(n, ord("A"), np.uint8) for n in range(1, 201)]
    for form in (1, 2):
        exp_t, exp_l = _check(gpu, v, rows, 64, "b", form=form)
    assert exp_l[:8].tolist() == [1, 1, 1, 1, 2, 2, 2, 2] and exp_t[6, :2].tolist() == [5, 6]
    long_rows = [np.full(n, ord("A"), np.uint8) for n in (1024, 1023, 8192, 8191, 4097)]
    _check(gpu, v, long_rows[:2], 300, "b", form=1)
    exp_t, exp_l = _check(gpu, v, long_rows, 2100, "b")
    assert exp_l.tolist() == [256, 256, 2048, 2048, 1025]


def test_unmapped_bytes_are_barriers_at_the_boundaries(gpu, bsq):
    """N at positions 15, 16, 63, 64 and at a row's first and last character, in poly-A rows and in random ones."""
    from bioseq_amd import bpe
    rng = np.random.default_rng(5)
    rows = []
    for at in ([15], [16], [63], [64], [0], [-1], [0, -1], [15, 16], [63, 64], [62, 64], [0, 15, 16, 63, 64, -1]):
        for base in (np.full(130, ord("A"), np.uint8), twin.low_complexity_row(rng, 130, "ACGT")):
            row = base.copy()
            row[at] = ord("N")
            rows.append(row)
    rows += [np.full(n, ord("N"), np.uint8) for n in (1, 2, 64, 65)]
    for v in (bpe.BPEVocab.from_merges(_tok(), PARITY_MERGES), _trained()):
        for form in (1, 2):
            exp_t, exp_l = _check(gpu, v, rows, 140, form=form)
        assert exp_l[-4:].tolist() == [1, 2, 64, 65] and (exp_t[-1, :65] == v.M + 4).all(), "an UNK is never fused"


def test_a_chain_table_fuses_one_pair_per_step(gpu, bsq):
    """(C,A), (CA,A), (CAA,A) ...: a row C A A A ... loses one symbol per step, so the step loop runs the row's length."""
    from bioseq_amd import bpe
    M = 3000
    merges = np.zeros((M, 2), np.int64)
    merges[0] = (1, 0)
    merges[1:, 0] = 4 + np.arange(M - 1)
    v = bpe.BPEVocab(_tok(), merges)
    row = lambda n: np.concatenate([[ord("C")], np.full(n - 1, ord("A"), np.uint8)]).astype(np.uint8)
    exp_t, exp_l = _check(gpu, v, [row(1024), row(700), row(2)], 8, form=1)
    assert exp_l.tolist() == [1, 1, 1] and exp_t[:, 0].tolist() == [4 + 1022, 4 + 698, 4]
    exp_t, exp_l = _check(gpu, v, [row(8192), row(3001), row(1025)], 5200, "h")
    assert exp_l.tolist() == [8192 - 3000, 1, 1] and exp_t[0, :2].tolist() == [4 + 2999, 0]


@pytest.mark.parametrize("flags", [(False, False, False), (True, True, True), (True, False, False), (False, True, False)])
def test_cut_rows_keep_their_count_in_lengths(gpu, bsq, flags):
    """P below, at and above n + bos + eos, and P = 1: lengths holds n before the cut."""
    v = _trained(flags)
    rng = np.random.default_rng(3)
    rows = [twin.random_row(rng, 300, "ACGT"), twin.random_row(rng, 40, "ACGT", 0.05), np.zeros(0, np.uint8)]
    eos, bos, _ = flags
    n = int(_check(gpu, v, rows, 400)[1][0])
    for P in (1, 2, n + bos + eos - 1, n + bos + eos, n + bos + eos + 1, n - 7):
        for form in (1, 2):
            exp_t, exp_l = _check(gpu, v, rows, P, form=form)
            assert exp_l[0] == n and exp_l[2] == 0
    if bos and eos:
        assert _check(gpu, v, rows, 1)[0].ravel().tolist() == [v.M + 5] * 3  # BOS alone


@pytest.mark.parametrize("destchar", ["b", "h", "i", "q", "f", "d"])
@pytest.mark.parametrize("batch_first", [True, False])
def test_every_element_type_in_both_layouts(gpu, bsq, destchar, batch_first):
    v = _trained((True, True, True), n_merges=100)  # vocab 108: int8 holds it
    rng = np.random.default_rng(8)
    rows = [twin.random_row(rng, int(n), "ACGT", 0.02) for n in rng.integers(0, 500, 37)]
    for form in (1, 2):
        _check(gpu, v, rows, 131, destchar, batch_first, form=form)


def test_a_table_whose_hash_collides_and_no_table_at_all(gpu, bsq):
    from bioseq_amd import bpe
    rng = np.random.default_rng(12)
    tok = _tok("AMINO20", True, False, True)
    letters = "ACDEFGHIKLMNPQRSTVWY"
    v = bpe.BPEVocab(tok, twin.random_table(rng, 20, 3000, small=0.9))
    slots = v.table.view(np.uint32).reshape(-1, 2)
    used = np.flatnonzero(slots[:, 0] != 0xFFFFFFFF)
    lg = int(np.log2(len(slots)))
    home = ((slots[used, 0].astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - lg)
    assert len(slots) == 8192 and len(used) == 3000 and (home != used).sum() > 100, "the table has no displaced entries: nothing probes"
    rows = [twin.random_row(rng, int(n), letters, 0.01) for n in rng.integers(0, 1025, 40)] + [twin.low_complexity_row(rng, 900, letters) for _ in range(8)]
    for form in (1, 2):
        exp_t, exp_l = _check(gpu, v, rows, 700, "h", form=form)
    assert (exp_l[1:] < np.array([len(r) for r in rows])[1:]).sum() > 30
    v0 = bpe.BPEVocab(tok, np.zeros((0, 2), np.int64))
    exp_t, exp_l = _check(gpu, v0, rows, 1100, "b")
    assert exp_l.tolist() == [len(r) for r in rows] and v0.table.nbytes == 128


def test_refused_calls_leave_the_outputs_untouched(gpu, bsq):
    import torch
    from bioseq_amd import bpe, capi
    L = capi.load()
    v = _trained()  # vocab 205
    chars, offs = twin.pack(_edge_rows()[:12])
    dch, dof = torch.from_numpy(chars).to(gpu), torch.from_numpy(offs).to(gpu)
    B, P = len(offs) - 1, 16
    table = v.device_table(gpu)

    def call(dt, max_chars=1024, form=0, reserved=0, M=v.M, tab=table.data_ptr(), padlen=P, rows=B):
        tokens = torch.full((B * P * 2,), 0x5A, dtype=torch.uint8, device=gpu)
        lengths = torch.full((B * 4,), 0x5A, dtype=torch.uint8, device=gpu)
        st = L.bsq_bpe_tokenize_device(ctypes.byref(v.desc), dch.data_ptr(), dof.data_ptr(), rows, padlen, 1, tab, M,
                                       ctypes.byref(capi.Bpe(max_chars, form, reserved)), dt, tokens.data_ptr(), lengths.data_ptr(), None)
        torch.cuda.synchronize()
        return st, bool((tokens == 0x5A).all()), bool((lengths == 0x5A).all())

    assert call(capi.I16) == (capi.OK, False, False)
    assert call(capi.I8) == (capi.ERR_DTYPE, True, True) and L.bsq_last_error()
    for kw in (dict(max_chars=0), dict(max_chars=8193), dict(max_chars=1025, form=1), dict(form=3), dict(reserved=1), dict(M=70000), dict(tab=None),
               dict(padlen=0), dict(rows=-1)):
        assert call(capi.I16, **kw) == (capi.ERR_INVALID_ARG, True, True), kw
    assert call(capi.I16, rows=0) == (capi.OK, True, True)  # B == 0: nothing launched
    t, n = bpe.bpe_tokenize_packed(v, dch[:0], dof[:1], 5)
    assert tuple(t.shape) == (0, 5) and tuple(n.shape) == (0,)
    with pytest.raises(ValueError):
        bpe.bpe_tokenize_packed(v, dch, dof, P, "b")
    with pytest.raises(ValueError):
        bpe.bpe_tokenize_packed(v, dch, dof, P, max_chars=1025, form=1)
    with pytest.raises(ValueError):
        bpe.bpe_tokenize_packed(v, chars, offs, P)  # host arrays


def test_a_store_that_ends_with_its_allocation(gpu, bsq):
    """The last row ends exactly at offsets[B] and the character tensor holds not one byte more: no read goes past it (the kernels bound
    every character load by offsets[B]).  Lengths 1 .. 17 and 1024 as the last row, on a side stream."""
    import torch
    from bioseq_amd import bpe
    v = _trained()
    rng = np.random.default_rng(21)
    side = torch.cuda.Stream(device=gpu)
    for last in (1, 15, 16, 17, 1024):
        rows = [twin.random_row(rng, 33, "ACGT"), twin.random_row(rng, last, "ACGT")]
        chars, offs = twin.pack(rows)
        dch = torch.empty(int(offs[-1]), dtype=torch.uint8, device=gpu)
        dch.copy_(torch.from_numpy(chars))
        dof = torch.from_numpy(offs).to(gpu)
        assert dch.numel() == offs[-1]
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got_t, got_l = bpe.bpe_tokenize_packed(v, dch, dof, 600, "i", max_chars=1024)
        side.synchronize()
        exp_t, exp_l = bpe.bpe_tokenize_host(v, chars, offs, 600, "i")
        assert got_t.cpu().numpy().tobytes() == exp_t.tobytes() and got_l.cpu().numpy().tobytes() == exp_l.tobytes()
