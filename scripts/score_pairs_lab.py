#!/usr/bin/env python3
"""The scored alignment of row pairs (bsq_score_pairs_device) as whole calls: pairs per second and DP cells per second (the sum of
la * lb over the list) in local mode without and with ends and in global mode, beside the edit distance (bsq_edit_pairs_device) on the
same lists and the host twin on one thread at a 1/64 sample of each list -- for scale, not a threshold.  Seeded random rows; pair k is
row k of store A against row k of store B.

    reads     1 048 576 pairs of DNA4 reads of 150 characters, B a copy of A with 3 % substitutions, +2 / -3 {5, 2}: max_len 256, form 1
    protein   262 144 pairs of AMINO20 rows of 50 .. 1024 residues, independent lengths, BLOSUM62 {11, 1}: max_len 4096 (form 3) and 1024 (form 2)
    long      4 096 pairs of DNA4 rows of 4096 x 4096 characters, +2 / -3 {5, 2}: form 3, every lane of a wave busy

Timing: device events around >= 0.25 s of work (at least 4 calls) after a warm-up, the calls alternating between two sets of stores,
lists and outputs, so a call finds none of its inputs in cache from the call before at the larger shapes; nothing here was timed with
a profiler attached.  Before timing, the device's scores and ends of the sample are asserted equal to the host twin's.

    python scripts/score_pairs_lab.py reads|protein|long [--quick]     (--quick: an eighth of the pairs and short timings)
"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bioseq_amd import Tokenizer, align, capi  # noqa: E402

QUICK = "--quick" in sys.argv
SECONDS = 0.05 if QUICK else 0.25
SHRINK = 8 if QUICK else 1
lib = align._lib
AMINO = "ACDEFGHIKLMNPQRSTVWY"


def store(rng, lengths, letters):
    """(chars, offsets) of random rows of these lengths"""
    offs = np.zeros(lengths.size + 1, np.int64)
    np.cumsum(lengths, out=offs[1:])
    return np.frombuffer(letters.encode(), np.uint8)[rng.integers(0, len(letters), int(offs[-1]), dtype=np.uint8)], offs


def timed(fn, seconds=SECONDS, least=4):
    fn(0), fn(1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(2):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    reps = max(least, int(seconds / max(a.elapsed_time(b) / 2e3, 1e-6)))
    reps += reps & 1
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us


def measure(dev, name, key, sets, max_len):
    """sets: two (chars_a, offsets_a, chars_b, offsets_b) of numpy arrays with equal lengths row by row"""
    tok = Tokenizer(key, False, False, False)
    matrix, o, e = (align.blosum62_matrix(tok), 11, 1) if key == "AMINO20" else (align.score_matrix(tok, 2, -3), 5, 2)
    desc = capi.desc_of(tok)
    n = sets[0][1].size - 1
    idx = np.arange(n, dtype=np.int64)
    cells = int((np.diff(sets[0][1]) * np.diff(sets[0][3])).sum())
    dsets = [[torch.from_numpy(x).to(dev) for x in s] + [torch.from_numpy(idx).to(dev), torch.from_numpy(idx.copy()).to(dev),
                                                         torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev)]
             for s in sets]
    stream = ctypes.c_void_p(capi.raw_stream(dev))
    sample = idx[::64].copy()
    sample_cells = int((np.diff(sets[0][1])[::64] * np.diff(sets[0][3])[::64]).sum())
    head = "%-8s %s max_len %4d | %8d pairs, %7.2f G cells |" % (name, key, max_len, n, cells / 1e9)
    for mode, with_ends in (("local", False), ("local", True), ("global", False)):
        sc = capi.Score(max_len, 0, align._MODES[mode], o, e)
        np.ctypeslib.as_array(sc.matrix)[:matrix.shape[0], :matrix.shape[1]] = matrix

        def call(i):
            ca, oa, cb, ob, row, col, score, ends = dsets[i & 1]
            capi.check(lib.bsq_score_pairs_device(ctypes.byref(desc), ca.data_ptr(), oa.data_ptr(), n, cb.data_ptr(), ob.data_ptr(), n, row.data_ptr(),
                                                  col.data_ptr(), n, ctypes.byref(sc), score.data_ptr(), ends.data_ptr() if with_ends else None, stream))

        t0 = time.perf_counter()
        host, host_ends = align.score_pairs_host(tok, sets[0][0], sets[0][1], sample, sample, sets[0][2], sets[0][3], matrix=matrix, gap_open=o, gap_extend=e,
                                                 mode=mode, ends=True, max_len=max_len)
        th = time.perf_counter() - t0
        call(0)
        torch.cuda.synchronize()
        assert np.array_equal(dsets[0][6].cpu().numpy()[::64], host) and (host > align.CODE_BELOW).all(), "the device and the host twin differ"
        assert not with_ends or np.array_equal(dsets[0][7].cpu().numpy()[::64], host_ends), "the ends differ"
        us = timed(call)
        print("%s %-31s %10.1f us per call, %8.2f M pairs/s, %8.1f G cells/s | host twin, one thread, %d pairs: %.3f s, %.3f M pairs/s, %.2f G cells/s | "
              "sample equal" % (head, align.score_kernel_name(mode=mode, ends=with_ends, max_len=max_len), us, n / us, cells / us / 1e3, sample.size, th,
                                sample.size / th / 1e6, sample_cells / th / 1e9), flush=True)
    ed = capi.Edit(max_len, 0)

    def edit(i):
        ca, oa, cb, ob, row, col, score, _ = dsets[i & 1]
        capi.check(lib.bsq_edit_pairs_device(ctypes.byref(desc), ca.data_ptr(), oa.data_ptr(), n, cb.data_ptr(), ob.data_ptr(), n, row.data_ptr(),
                                             col.data_ptr(), n, ctypes.byref(ed), score.data_ptr(), stream))

    us = timed(edit)
    print("%s %-31s %10.1f us per call, %8.2f M pairs/s, %8.1f G cells/s | (the unit-cost edit distance on the same lists)"
          % (head, align.edit_kernel_name(max_len), us, n / us, cells / us / 1e3), flush=True)


def part_reads(dev):
    n = 1048576 // SHRINK
    sets = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        ca, oa = store(rng, np.full(n, 150, np.int64), "ACGT")
        cb = ca.copy()
        hit = rng.random(cb.size) < 0.03
        cb[hit] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(hit.sum()))]
        sets.append((ca, oa, cb, oa.copy()))
    measure(dev, "reads", "DNA4", sets, 256)


def part_protein(dev):
    n = 262144 // SHRINK
    sets = []
    for seed in (3, 4):
        rng = np.random.default_rng(seed)
        sets.append(store(rng, rng.integers(50, 1025, n), AMINO) + store(rng, rng.integers(50, 1025, n), AMINO))
    measure(dev, "protein", "AMINO20", sets, 4096)
    measure(dev, "protein", "AMINO20", sets, 1024)


def part_long(dev):
    n = 4096 // SHRINK
    sets = []
    for seed in (5, 6):
        rng = np.random.default_rng(seed)
        sets.append(store(rng, np.full(n, 4096, np.int64), "ACGT") + store(rng, np.full(n, 4096, np.int64), "ACGT"))
    measure(dev, "long", "DNA4", sets, 4096)


def main():
    parts = {"reads": part_reads, "protein": part_protein, "long": part_long}
    chosen = [a for a in sys.argv[1:] if a in parts]
    if not chosen:
        sys.exit(__doc__)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    print("# scored alignment of row pairs: whole calls, buffers alternating; us per call", flush=True)
    for name in chosen:
        parts[name](dev)


if __name__ == "__main__":
    main()
