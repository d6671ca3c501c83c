"""GPU: span-corruption (T5) batches (bioseq_amd.masking.span_corrupt_packed, bsq_span_corrupt_device) against the independent twin
(tests/span_corrupt_twin.py) bit for bit.  A wave owns a row and walks it in tiles of T = 1024 characters, 16 per lane, four rows per
workgroup: B = 9 is two full workgroups and a partial one, and the rows are a few tiles at most.  Every test reads from the twin's
details that its batch really holds the case it is named for, so a seed that misses the case fails instead of passing silently."""
import ctypes

import numpy as np
import pytest

import span_corrupt_twin as twin

pytestmark = pytest.mark.gpu

T = 1024  # characters a wave takes per tile (bsq_span_dev.h: kTile)
B = 9
POOL = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTNacgtn*\xff", dtype=np.uint8)  # mostly mapped, some N / lower case / junk
TORCH_OF = {"b": "int8", "h": "int16", "i": "int32", "q": "int64", "f": "float32", "d": "float64"}


def _tok(bsq, key, flags):
    eos, bos, pad = flags
    return bsq.Tokenizer(key, bool(eos), bool(bos), bool(pad))


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.array(a)).to(gpu)  # (a copy: np.frombuffer arrays are read-only)


def _batch(rng, pins=None):
    """B rows: lengths 0, 1, T - 1, T, T + 1, 2 T + 3, the rest random below 2 T; pins: {row: bytes} replaces rows 6 ..; the LAST row
    ends at the last byte of chars (the guarded loads)."""
    pins = pins or {}
    lens = rng.integers(0, 2 * T, B).astype(np.int64)
    lens[:6] = (0, 1, T - 1, T, T + 1, 2 * T + 3)
    for r, seq in pins.items():
        lens[r] = len(seq)
    chars = rng.choice(POOL, int(lens.sum())).astype(np.uint8)
    offs = np.zeros(B + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    for r, seq in pins.items():
        chars[offs[r]:offs[r + 1]] = np.frombuffer(seq, np.uint8)
    assert offs[-1] == chars.size and lens[-1] > 0
    return chars, offs


def _device(gpu, tok, chars, offs, P_in, P_tgt, dc="q", ldc="q", **kw):
    """span_corrupt_packed on the device, as four numpy arrays (the matrices as int64)"""
    import torch
    from bioseq_amd import masking
    got = masking.span_corrupt_packed(tok, _dev(chars, gpu), _dev(offs, gpu), P_in, P_tgt, dc, label_dtype=ldc, validate=False, **kw)
    torch.cuda.synchronize()
    assert got[0].dtype == getattr(torch, TORCH_OF[dc]) and got[1].dtype == getattr(torch, TORCH_OF[ldc])
    assert got[2].dtype == torch.int32 and got[3].dtype == torch.int32
    return [t.cpu().numpy().astype(np.int64) for t in got]


def _check(gpu, tok, chars, offs, P_in, P_tgt, dc="q", ldc="q", **kw):
    """The device against the twin, bit for bit; the twin's (inputs, labels, in_len, tgt_len, details)"""
    from bioseq_amd import capi
    exp = twin.corrupt_batch(capi.desc_of(tok), chars, offs, P_in, P_tgt, **kw)
    got = _device(gpu, tok, chars, offs, P_in, P_tgt, dc, ldc, **kw)
    for name, g, e in zip(("inputs", "labels", "in_len", "tgt_len"), got, exp):
        assert g.shape == e.shape and np.array_equal(g, e), (name, np.argwhere(g != e)[:5].tolist(), kw)
    return exp


@pytest.mark.parametrize("flags, span, prob", [((0, 0, 0), 3, 0.3), ((1, 1, 1), 1, 0.5), ((0, 1, 0), 16, 0.05), ((1, 0, 1), 5, 1.0)])
def test_pinned_lengths_around_the_tile(gpu, bsq, flags, span, prob):
    from bioseq_amd import masking
    rng = np.random.default_rng(100 + span)
    chars, offs = _batch(rng)
    tok = _tok(bsq, "DNA4", flags)
    assert masking.span_corrupt_kernel_name(tok, B, 4 * T, 4 * T) == "k_span_corrupt"
    exp = _check(gpu, tok, chars, offs, 2 * T + 3 + flags[0] + flags[1], 2 * T + 8, anchor_prob=prob, span=span, seed=span + 40, first_row=5,
                 max_sentinels=65535 if span == 1 else 1000)
    lens = np.diff(offs)
    assert lens[:6].tolist() == [0, 1, T - 1, T, T + 1, 2 * T + 3] and (lens[6:] < 2 * T).all()
    runs = [d["runs"] for d in exp[4]]
    assert any(a < T <= a + n - 1 for r in runs for a, n in r)  # a run crosses a tile seam
    assert any(a % 16 and a // 16 != (a + n - 1) // 16 for r in runs for a, n in r)  # and one crosses lanes
    assert (exp[2] <= 2 * T + 3).all() and (exp[3] <= 2 * T + 8 - flags[0]).all()  # no row is cut here
    assert (exp[3] > 0).sum() >= 6


def test_one_gap_across_two_seams_and_unmapped_bytes_at_a_seam(gpu, bsq):
    straddle = bytearray(b"ACGT" * (T // 2))
    straddle[T - 3:T + 4] = b"N" * 7
    chars, offs = _batch(np.random.default_rng(1), pins={6: b"G" * (2 * T + 3), 7: bytes(straddle)})
    tok = _tok(bsq, "DNA4", (1, 1, 1))
    exp = _check(gpu, tok, chars, offs, 2 * T + 5, 2 * T + 5, anchor_prob=1.0, span=1, seed=3)
    assert exp[4][6]["runs"] == [(0, 2 * T + 3)] and exp[2][6] == 1 and exp[3][6] == 2 * T + 4  # one sentinel; it and the whole row
    assert exp[4][7]["runs"] == [(0, T - 3), (T + 4, T - 4)] and not any(exp[4][7]["cand"][T - 3:T + 4])
    assert exp[0][7][1:11].tolist() == [7] + [0] * 7 + [8, 5]  # BOS, then: sentinel, the seven unmapped bytes, sentinel, EOS
    # the same rows under a draw: the unmapped run ends one run at T - 4 and the next opens behind it
    exp = _check(gpu, tok, chars, offs, 2 * T + 5, 2 * T + 5, anchor_prob=0.3, span=4, seed=4)
    runs = exp[4][7]["runs"]
    assert any(a + n == T - 3 for a, n in runs) and any(a == T + 4 for a, n in runs)


def test_span_16_looks_back_across_lanes_and_a_seam(gpu, bsq):
    chars, offs = _batch(np.random.default_rng(2), pins={6: b"ACGT" * (T // 2)})
    tok = _tok(bsq, "DNA4", (0, 0, 0))
    exp = _check(gpu, tok, chars, offs, 2 * T + 3, 2 * T + 3, anchor_prob=0.05, span=16, seed=10)
    seam = lane = 0
    for d in exp[4]:
        anchors, cand = d["anchors"], d["cand"]
        for j in range(len(cand)):
            if cand[j] and j >= T and j - 15 < T and not any(anchors[T:j + 1]):
                seam += 1  # covered from the tile before only
            if cand[j] and j % 16 < 15 and not any(anchors[j - j % 16:j + 1]):
                lane += 1  # covered from the lane before only
    assert seam > 0 and lane > 0


def test_max_sentinels_cutoff_in_the_second_tile_and_at_the_run_count(gpu, bsq):
    third_in_second_tile = b"A" * 500 + b"N" + b"C" * 600 + b"N" + b"G" * 300 + b"NN" + b"T" * 40
    chars, offs = _batch(np.random.default_rng(3), pins={6: third_in_second_tile, 7: b"ACGTN" * 3})
    tok = _tok(bsq, "DNA4", (1, 0, 1))
    for cutoff, step, first in ((2, 1, 6), (4, -1, 40), (3, 1, 6)):
        exp = _check(gpu, tok, chars, offs, 2 * T + 8, 2 * T + 8, "h", "h", anchor_prob=1.0, span=2, seed=1, max_sentinels=cutoff,
                     sentinel_first=first, sentinel_step=step)
        runs = exp[4][6]["runs"]
        assert [a for a, _ in runs] == [0, 501, 1102, 1404] and runs[2][0] >= T  # the third run opens in the second tile
        sent = [first + g * step for g in range(cutoff)]
        assert [v for v in exp[0][6] if v in sent] == sent[:min(cutoff, 4)]
        assert exp[3][6] == sum(n + 1 for _, n in runs[:cutoff]) and exp[2][6] == len(third_in_second_tile) - exp[3][6] + 2 * min(cutoff, 4)
        assert len(exp[4][7]["runs"]) == 3  # cutoff 3: max_sentinels equal to the row's run count exactly; 2: one run short; 4: one to spare
    # under a draw: rows with more runs than sentinels, the cutoff falling in the second tile
    exp = _check(gpu, tok, chars, offs, 2 * T + 8, 2 * T + 8, anchor_prob=0.05, span=3, seed=6, max_sentinels=50)
    assert any(len(d["runs"]) > 50 and d["runs"][50][0] >= T for d in exp[4]) and any(0 < len(d["runs"]) <= 50 for d in exp[4])


def test_widths_that_cut_after_a_sentinel_inside_a_run_and_not_at_all(gpu, bsq):
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 40, B).astype(np.int64)
    lens[:2] = (0, 1)
    chars = rng.choice(POOL, int(lens.sum())).astype(np.uint8)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seen = dict(after_sentinel=0, in_run=0, no_room=0, uncut=0)
    for flags in ((1, 1, 1), (0, 0, 0), (1, 0, 0)):
        tok = _tok(bsq, "DNA4", flags)
        first = tok.alphabet_size()
        for P_in, P_tgt in ((1, 1), (2, 2), (8, 8), (15, 17), (17, 15), (33, 31), (47, 49)):
            exp = _check(gpu, tok, chars, offs, P_in, P_tgt, "i", "q", anchor_prob=0.25, span=3, seed=12)
            room_in, room_tgt = max(P_in - flags[0] - flags[1], 0), max(P_tgt - flags[0], 0)
            seen["no_room"] += int(room_in == 0) + int(room_tgt == 0)
            for d, in_len, tgt_len in zip(exp[4], exp[2], exp[3]):
                for body, n, room in ((d["in_body"], in_len, room_in), (d["tgt_body"], tgt_len, room_tgt)):
                    if 0 < room < n:
                        seen["after_sentinel" if body[room - 1] >= first else "in_run"] += 1
                    seen["uncut"] += int(0 < n <= room)
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("dc, ldc, step", [("b", "q", -1), ("h", "h", 1), ("q", "h", -1), ("f", "q", 1), ("d", "i", 1), ("i", "f", -1)])
def test_element_types_and_both_steps(gpu, bsq, dc, ldc, step):
    chars, offs = _batch(np.random.default_rng(5))
    tok = _tok(bsq, "AMINO20", (1, 1, 0))
    first = 30 if step == 1 else 126
    exp = _check(gpu, tok, chars, offs, T + 101, T // 4 + 1, dc, ldc, anchor_prob=0.08, span=3, seed=8, max_sentinels=97, sentinel_first=first,
                 sentinel_step=step, ignore_index=-100 if ldc != "h" else -1)
    assert max(len(d["runs"]) for d in exp[4]) > 97 and (exp[2] > T + 99).any() and (exp[3] > T // 4).any()  # the cutoff and both cuts


def test_either_matrix_may_be_null(gpu, bsq):
    import torch
    from bioseq_amd import capi
    L = capi.load()
    chars, offs = _batch(np.random.default_rng(6))
    tok = _tok(bsq, "DNA4", (1, 1, 1))
    desc = capi.desc_of(tok)
    kw = dict(anchor_prob=0.1, span=3, seed=2)
    exp = twin.corrupt_batch(desc, chars, offs, 300, 200, **kw)
    m = capi.SpanCorrupt(0.1, 3, 100, 7, 1, -100, 2, 0)
    dc, do = _dev(chars, gpu), _dev(offs, gpu)
    for want_in, want_lab, want_len in ((True, False, True), (False, True, True), (True, True, False)):
        inp = torch.full((B, 300), 99, dtype=torch.int16, device=gpu)
        lab = torch.full((B, 200), 99, dtype=torch.int64, device=gpu)
        lens = torch.full((2, B), -7, dtype=torch.int32, device=gpu)
        with capi.launching(dc.device) as stream:
            capi.check(L.bsq_span_corrupt_device(ctypes.byref(desc), dc.data_ptr(), do.data_ptr(), B, 300, 200, ctypes.byref(m), capi.I16,
                                                 inp.data_ptr() if want_in else None, capi.U64, lab.data_ptr() if want_lab else None,
                                                 lens[0].data_ptr() if want_len else None, lens[1].data_ptr() if want_len else None, stream))
        torch.cuda.synchronize()
        assert np.array_equal(inp.cpu().numpy(), exp[0]) if want_in else bool((inp == 99).all())
        assert np.array_equal(lab.cpu().numpy(), exp[1]) if want_lab else bool((lab == 99).all())
        assert np.array_equal(lens.cpu().numpy(), np.stack([exp[2], exp[3]])) if want_len else bool((lens == -7).all())
    with capi.launching(dc.device) as stream:
        st = L.bsq_span_corrupt_device(ctypes.byref(desc), dc.data_ptr(), do.data_ptr(), B, 300, 200, ctypes.byref(m), capi.I16, None, capi.U64, None,
                                       None, None, stream)
    assert st == capi.ERR_INVALID_ARG


@pytest.mark.parametrize("code, tname, shift", [(0, "int8", 5), (1, "int16", 3), (2, "int32", 1), (3, "int64", 1), (4, "float32", 3), (5, "float64", 1)])
def test_matrices_that_start_off_a_16_byte_boundary(gpu, bsq, code, tname, shift):
    """The bodies and the tails leave as 16-byte vectors aligned in memory: matrices that start `shift` elements behind a boundary, rows
    of an odd width, and the elements around both matrices untouched."""
    import torch
    from bioseq_amd import capi
    L = capi.load()
    chars, offs = _batch(np.random.default_rng(9))
    tok = _tok(bsq, "DNA4", (1, 1, 1))
    desc = capi.desc_of(tok)
    P_in, P_tgt = T + 37, T // 4 + 11
    exp = twin.corrupt_batch(desc, chars, offs, P_in, P_tgt, anchor_prob=0.1, span=3, seed=2, ignore_index=-7)
    assert (exp[2] > P_in - 2).any() and (exp[2] < P_in - 2).any() and (exp[3] > P_tgt - 1).any() and (exp[3] < P_tgt - 1).any()  # cut and uncut rows
    m = capi.SpanCorrupt(0.1, 3, 100, 7, 1, -7, 2, 0)
    dt = getattr(torch, tname)
    inp = torch.full((shift + B * P_in + 16,), 99, dtype=dt, device=gpu)
    lab = torch.full((shift + B * P_tgt + 16,), 99, dtype=dt, device=gpu)
    dc, do = _dev(chars, gpu), _dev(offs, gpu)
    with capi.launching(dc.device) as stream:
        capi.check(L.bsq_span_corrupt_device(ctypes.byref(desc), dc.data_ptr(), do.data_ptr(), B, P_in, P_tgt, ctypes.byref(m), code,
                                             inp[shift:].data_ptr(), code, lab[shift:].data_ptr(), None, None, stream))
    torch.cuda.synchronize()
    for got, want, P in ((inp, exp[0], P_in), (lab, exp[1], P_tgt)):
        got = got.cpu().numpy().astype(np.int64)
        assert np.array_equal(got[shift:shift + B * P].reshape(B, P), want)
        assert (got[:shift] == 99).all() and (got[shift + B * P:] == 99).all()


@pytest.mark.parametrize("flags", [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 1)])
def test_anchor_prob_0_is_tokenize_packed(gpu, bsq, flags):
    import torch
    from bioseq_amd import masking
    chars, offs = _batch(np.random.default_rng(7))
    tok = _tok(bsq, "DNA4", flags)
    P = 2 * T + 5
    dc, do = _dev(chars, gpu), _dev(offs, gpu)
    inputs, labels, in_len, tgt_len = masking.span_corrupt_packed(tok, dc, do, P, 3, "h", anchor_prob=0.0)
    plain = tok.tokenize_packed(dc, do, P, "h", True)
    assert torch.equal(inputs, plain) and torch.equal(in_len.cpu(), torch.from_numpy(np.diff(offs)).int()) and not bool(tgt_len.any())
    want = [4 + flags[1]] * flags[0] + [-100] * (3 - flags[0])
    assert labels.cpu().tolist() == [want] * B
    with pytest.raises(RuntimeError):  # validate: the over-long check of tokenize_packed on the uncorrupted rows
        masking.span_corrupt_packed(tok, dc, do, 2 * T, 3, "h", anchor_prob=0.0)


def test_span_corrupt_dataset_groups_and_prefetch(gpu, bsq, tmp_path):
    import torch
    from bioseq_amd import masking
    from bioseq_amd.flatfile import FlatFile, write_flatfile
    from bioseq_amd.loaders import FlatFileDataset
    rng = np.random.default_rng(8)
    lens = rng.integers(0, 300, 200)
    lens[:3] = (0, 5, 700)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGTACGTACGTACGTNacgt", np.uint8), int(n))) for n in lens]
    ff = FlatFile(write_flatfile(seqs, str(tmp_path / "span.ff")))
    tok = _tok(bsq, "DNA4", (1, 1, 1))

    def epoch(shuffle, crop=None, rc=0.0, target_len=None, **opts):
        ds = FlatFileDataset(ff, tok, device=gpu, span_corrupt=True, span=3, maskfrac=0.2, token_dtype="i", crop=crop, revcomp_frac=rc, target_len=target_len)
        g = torch.Generator(device=gpu).manual_seed(5)
        out = [(a.clone(), b.clone()) for a, b in ds.batches(64, shuffle=shuffle, generator=g, **opts)]
        torch.cuda.synchronize()
        return ds, out

    for kw in (dict(shuffle=False), dict(shuffle=True), dict(shuffle=True, crop=128, rc=0.5, target_len=40)):
        ds, one = epoch(**kw)
        width = (kw.get("crop") or 700) + 2
        assert ds.max_seq_len == width and ds.target_len == kw.get("target_len", width) and len(one) == 4
        assert all(a.dtype == torch.int32 and b.dtype == torch.int64 and a.shape[1] == width and b.shape[1] == ds.target_len for a, b in one)
        for opts in (dict(group=2), dict(prefetch=2), dict(group=2, prefetch=2)):
            _, got = epoch(**kw, **opts)
            assert len(got) == len(one) and all(torch.equal(p, r) and torch.equal(q, s) for (p, q), (r, s) in zip(one, got)), (kw, opts)
    # the unshuffled epoch is the direct call with the dataset's first mask key (seed 13), rows keyed by their index
    ds, one = epoch(shuffle=False)
    key = (13 * 0x9E3779B97F4A7C15 + 1) & (2 ** 64 - 1)
    chars = np.frombuffer(b"".join(seqs), np.uint8)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    di, dl, _, _ = masking.span_corrupt_packed(tok, _dev(chars, gpu), _dev(offs, gpu), 702, 702, "i", frac=0.2, span=3, seed=key)
    assert torch.equal(torch.cat([a for a, _ in one]), di) and torch.equal(torch.cat([b for _, b in one]), dl)
    assert bool((dl[:, 0] >= 7).sum() > 100)  # label rows open with a sentinel
    a, b = ds[2]
    assert a.shape == (702,) and b.shape == (702,)
    for bad in (dict(cnn=True), dict(augment=2), dict(masked=True), dict(kmer=3), dict(pack="nextfit"), dict(spectrum=3), dict(target_len=0),
                dict(span=17), dict(maskfrac=1.5)):
        with pytest.raises(ValueError):
            FlatFileDataset(ff, tok, device=gpu, **dict(dict(span_corrupt=True), **bad))
