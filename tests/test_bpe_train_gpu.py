"""GPU: BPE training on the device (bioseq_amd.bpe.bpe_train_packed, bsq_bpe_train_*_device) against the numpy rule `bpe_train_host`
where that is fast enough, else against the library's CPU twin, which tests/test_bpe_train_host.py pins to it -- merges and winning
counts: the header's known answers, row lengths at every lane, 64-position and form edge in both forms, one batch and one row at a
time, the block form's lengths, barriers at 64-position edges, a many-ties sample whose stop comes early, several workgroups, the spill
of the per-workgroup LDS hash to the global table, the overflow of a small pair table, the cut of the steps into calls, rows above
max_chars, untouched inputs, a store that ends at the last byte of its allocation, and the vocabulary's way into the tokenizer."""
import functools

import numpy as np
import pytest

import bpe_twin as twin

pytestmark = pytest.mark.gpu

EDGES = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024)
BLOCK_EDGES = (1025, 4095, 4096, 4097, 8191, 8192)
KNOWN = [([b"AAAAAAA"], [(0, 0)], [3]),
         ([b"ACGACGACG", b"CGCG"], [(1, 2), (0, 4)], [5, 3]),
         ([b"ACAC", b"GTGT"], [(0, 1), (2, 3)], [2, 2]),
         ([b"ACACAC", b"ACACAC"], [(0, 1), (4, 4), (5, 4)], [6, 2, 2]),
         ([b"AAAAANAAAA"], [(0, 0), (4, 4)], [4, 2]),
         ([b"ACGTNACGT"], [(0, 1), (2, 3), (4, 5)], [2, 2, 2]),
         ([b"AC", b"AC"], [(0, 1)], [2]),
         ([b"A" * 8192], [(0, 0)] + [(k, k) for k in range(4, 15)], [4096 >> k for k in range(12)])]


def _tok(key="DNA4", eos=False, bos=False, padchar=False):
    import bioseq_amd
    return bioseq_amd.Tokenizer(key, eos, bos, padchar)


def _device(gpu, rows, n_merges, key="DNA4", **kw):
    """(merges, counts, info) of bpe_train_packed on uploaded copies of the rows."""
    import torch
    from bioseq_amd import bpe
    chars, offs = twin.pack(rows)
    v, info = bpe.bpe_train_packed(_tok(key), torch.from_numpy(chars).to(gpu), torch.from_numpy(offs).to(gpu), n_merges, return_info=True, **kw)
    assert isinstance(v, bpe.BPEVocab) and info["counts"].dtype == np.int64 and info["counts"].shape == (v.M,)
    return v.merges.tolist(), info["counts"].tolist(), info


def _twin(rows, n_merges, key="DNA4", **kw):
    from bioseq_amd import bpe
    v, info = bpe.bpe_train_packed(_tok(key), *twin.pack(rows), n_merges, return_info=True, **kw)
    return v.merges.tolist(), info["counts"].tolist()


def _numpy(rows, n_merges, key="DNA4"):
    from bioseq_amd import bpe
    return bpe.bpe_train_host(_tok(key), *twin.pack(rows), n_merges).merges.tolist()


def _check(gpu, rows, n_merges, key="DNA4", numpy_rule=True, **kw):
    """The device against the twin (merges and counts) and, where asked, the numpy rule (merges); returns the device's triple."""
    host_kw = {k: v for k, v in kw.items() if k == "max_chars"}
    got = _device(gpu, rows, n_merges, key, **kw)
    exp_m, exp_c = _twin(rows, n_merges, key, **host_kw)
    assert got[0] == exp_m and got[1] == exp_c, (got[0][:8], exp_m[:8], got[1][:8], exp_c[:8])
    if numpy_rule:
        assert got[0] == _numpy(rows, n_merges, key)
    return got


def test_known_answers(gpu, bsq):
    for rows, merges, counts in KNOWN:
        got_m, got_c, info = _device(gpu, rows, 40)
        assert got_m == [list(m) for m in merges] and got_c == counts, (rows[0][:12], got_m, got_c)
        assert info["skipped_rows"] == 0 and info["steps_launched"] == 40


@functools.lru_cache(maxsize=None)
def _edge_rows():
    rng = np.random.default_rng(42)
    rows = []
    for n in EDGES:
        rows += [np.full(n, ord("A"), np.uint8), twin.random_row(rng, n, "ACGT"), twin.low_complexity_row(rng, n, "ACGT"),
                 twin.random_row(rng, n, "ACGT", 0.02)]
    return rows


@pytest.mark.parametrize("form", [None, 1, 2])
def test_row_lengths_at_every_edge_in_one_batch(gpu, bsq, form):
    """0 .. 1024 characters, poly-A, random, low-complexity and 2 % N: None and 1 take the wave form, 2 the block form."""
    from bioseq_amd import bpe
    got_m, _, info = _check(gpu, _edge_rows(), 60, form=form)
    assert len(got_m) == 60
    assert info["kernel"] == bpe.bpe_train_kernel_name(1024, form) == ("k_bpe_train_pass<block>" if form == 2 else "k_bpe_train_pass<wave>")


@pytest.mark.parametrize("form", [None, 1, 2])
def test_row_lengths_at_every_edge_one_row_at_a_time(gpu, bsq, form):
    """Every row alone: a poly-A row's merges are the halvings, the other rows are held to the twin (8 merges keep 56 calls quick)."""
    for row in _edge_rows():
        _check(gpu, [row], 8, numpy_rule=False, form=form)


def test_block_form_lengths(gpu, bsq):
    """1025 .. 8192 characters, poly-A and random, 40 merges; the single poly-A row of 8192 gives the header's 12 merges."""
    from bioseq_amd import bpe
    rng = np.random.default_rng(7)
    rows = []
    for n in BLOCK_EDGES:
        rows += [np.full(n, ord("A"), np.uint8), twin.random_row(rng, n, "ACGT")]
    _, _, info = _check(gpu, rows, 40)
    assert info["kernel"] == "k_bpe_train_pass<block>" == bpe.bpe_train_kernel_name()
    for n in BLOCK_EDGES:
        _check(gpu, [np.full(n, ord("A"), np.uint8)], 40, numpy_rule=False)
    got_m, got_c, _ = _device(gpu, [np.full(8192, ord("A"), np.uint8)], 40)
    assert got_m == [list(m) for m in KNOWN[-1][1]] and got_c == KNOWN[-1][2]


@pytest.mark.parametrize("form", [1, 2])
def test_barriers_at_64_position_edges(gpu, bsq, form):
    """An N at positions 63, 64 and 65 of poly-A rows of 130: the run parity restarts behind the barrier."""
    rows = []
    for at in (63, 64, 65):
        row = np.full(130, ord("A"), np.uint8)
        row[at] = ord("N")
        rows.append(row)
    _check(gpu, rows, 20, form=form)
    for row in rows:
        _check(gpu, [row], 20, form=form)


def _ties_rows():
    rng = np.random.default_rng(5)
    return [twin.random_row(rng, 40, "ACGT") for _ in range(30)]


def test_many_ties_and_the_early_stop(gpu, bsq):
    """30 rows of 40 asked for 100 merges: counts of 2 and 3 tie constantly; 1000 merges of a 1 kB sample return fewer."""
    got_m, got_c, _ = _check(gpu, _ties_rows(), 100)
    assert got_c.count(2) + got_c.count(3) > len(got_c) // 2
    rng = np.random.default_rng(6)
    got_m, got_c, info = _check(gpu, [twin.random_row(rng, 1000, "ACGT")], 1000)
    assert 0 < len(got_m) < 1000 and got_c[-1] >= 2 and info["steps_launched"] < 1000


def test_several_workgroups(gpu, bsq):
    """4000 rows of 30 .. 60 characters at 100 merges: 125 workgroups of the wave form, 1000 of the block form."""
    rng = np.random.default_rng(8)
    rows = [twin.random_row(rng, int(rng.integers(30, 61)), "ACGT", 0.01) for _ in range(4000)]
    a = _check(gpu, rows, 100)
    b = _device(gpu, rows, 100, form=2)
    assert a[0] == b[0] and a[1] == b[1]


def test_lds_hash_spill_to_the_global_table(gpu, bsq):
    """AMINO20, 32 rows of 1024 in ONE workgroup's range (the wave form's ranges hold at least 32 rows): before the last merge the range
    holds more distinct pairs than the per-workgroup LDS hash has slots (bsq_bpe_train_lds_slots), so pairs go to the global table directly."""
    from bioseq_amd import bpe, capi
    lds_slots = capi.load().bsq_bpe_train_lds_slots()
    letters = "ACDEFGHIKLMNPQRSTVWY"
    rng = np.random.default_rng(9)
    rows = [twin.random_row(rng, 1024, letters) for _ in range(32)]
    got_m, _, _ = _check(gpu, rows, 150, key="AMINO20", numpy_rule=False, form=1)
    chars, offs = twin.pack(rows)
    v = bpe.BPEVocab(_tok("AMINO20"), np.array(got_m[:-1], np.int64))
    ids, lens = bpe.bpe_tokenize_host(v, chars, offs, 1024, "i")
    pairs = set()
    for row, n in zip(ids, lens):
        pairs.update(zip(row[:n - 1].tolist(), row[1:n].tolist()))
    assert len(pairs) > lds_slots, (len(pairs), lds_slots)


def test_table_overflow_is_an_error_and_the_next_call_is_right(gpu, bsq):
    import torch
    from bioseq_amd import bpe
    rng = np.random.default_rng(10)
    rows = [twin.random_row(rng, 200, "ACGT") for _ in range(20)]
    chars, offs = twin.pack(rows)
    with pytest.raises(RuntimeError, match="overflow"):
        bpe.bpe_train_packed(_tok(), torch.from_numpy(chars).to(gpu), torch.from_numpy(offs).to(gpu), 50, table_slots=16)
    _check(gpu, rows, 50)


def test_call_shape_invariance(gpu, bsq):
    """steps_per_call 1, 7 and the default give equal merges; max_chars=64 with longer rows present is the training on the short rows."""
    rng = np.random.default_rng(11)
    rows = [twin.random_row(rng, int(rng.integers(0, 120)), "ACGT", 0.02) for _ in range(80)]
    base = _check(gpu, rows, 60)
    for spc in (1, 7):
        got = _device(gpu, rows, 60, steps_per_call=spc)
        assert got[0] == base[0] and got[1] == base[1]
    few = _device(gpu, _ties_rows(), 100, steps_per_call=7)  # the stop inside a call of seven steps
    assert few[0] == _device(gpu, _ties_rows(), 100)[0] and few[2]["steps_launched"] % 7 == 0 and few[2]["steps_launched"] < 100
    short = [r for r in rows if len(r) <= 64]
    got = _check(gpu, rows, 60, numpy_rule=False, max_chars=64)
    assert got[2]["skipped_rows"] == len(rows) - len(short) > 0
    assert got[0] == _numpy(short, 60) == _device(gpu, short, 60)[0]


def test_inputs_are_untouched_and_a_store_may_end_its_allocation(gpu, bsq):
    """chars and offsets after the call are what they were; the characters sit at the very end of a 2 MiB allocation."""
    import torch
    from bioseq_amd import bpe
    rng = np.random.default_rng(12)
    rows = [twin.random_row(rng, int(rng.integers(1, 300)), "ACGT", 0.02) for _ in range(50)]
    chars, offs = twin.pack(rows)
    block = torch.zeros(2 << 20, dtype=torch.uint8, device=gpu)
    dchars = block[block.numel() - chars.size:]
    dchars.copy_(torch.from_numpy(chars))
    doffs = torch.from_numpy(offs).to(gpu)
    v = bpe.bpe_train_packed(_tok(), dchars, doffs, 80)
    assert v.merges.tolist() == _numpy(rows, 80)
    assert dchars.cpu().numpy().tobytes() == chars.tobytes() and doffs.cpu().numpy().tobytes() == offs.tobytes()


def test_the_vocabulary_goes_straight_into_the_tokenizer(gpu, bsq):
    import torch
    from bioseq_amd import bpe
    rng = np.random.default_rng(13)
    rows = [twin.random_row(rng, 150, "ACGT") for _ in range(64)]
    chars, offs = twin.pack(rows)
    dchars, doffs = torch.from_numpy(chars).to(gpu), torch.from_numpy(offs).to(gpu)
    v = bpe.bpe_train_packed(_tok(), dchars, doffs, 64)
    tokens, lengths = bpe.bpe_tokenize_packed(v, dchars, doffs, 150, "i")
    exp_t, exp_l = bpe.bpe_tokenize_host(v, chars, offs, 150, "i")
    assert v.M == 64 and tokens.cpu().numpy().tobytes() == exp_t.tobytes() and lengths.cpu().numpy().tobytes() == exp_l.tobytes()
    assert (exp_l < 150).all()


def test_an_empty_batch_and_empty_rows(gpu, bsq):
    import torch
    from bioseq_amd import bpe
    v, info = bpe.bpe_train_packed(_tok(), torch.zeros(0, dtype=torch.uint8, device=gpu), torch.zeros(1, dtype=torch.int64, device=gpu), 10,
                                   return_info=True)
    assert v.M == 0 and info["steps_launched"] == 0
    assert _device(gpu, [b"", b"", b""], 10)[0] == [] and _device(gpu, [b"", b"ACAC", b""], 10)[0] == [[0, 1]]
    assert _device(gpu, [b"ACACAC"], 0)[0] == [] and _device(gpu, [b"A", b"C", b"N"], 10)[0] == []
