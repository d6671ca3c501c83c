#!/usr/bin/env python3
"""The alignment statistics of row pairs (bsq_align_stats_device) as whole calls: pairs per second and DP cells per second (the sum of
la * lb over the list) in local and in global mode, each beside the scored alignment with ends (bsq_score_pairs_device, ends != NULL) on
the same lists and at the same max_len, the two taking turns, and the host twin on one thread at a 1/64 sample of each list -- for
scale, not a threshold.  Seeded random rows, the lists of scripts/score_pairs_lab.py; pair k is row k of store A against row k of B.

    reads     1 048 576 pairs of DNA4 reads of 150 characters, B a copy of A with 3 % substitutions, +2 / -3 {5, 2}: max_len 256
              (statistics: 16 lanes per pair; score: 4)
    protein   262 144 pairs of AMINO20 rows of 50 .. 1024 residues, independent lengths, BLOSUM62 {11, 1}: max_len 1024
              (statistics: 64 lanes per pair; score: 16)
    long      4 096 pairs of DNA4 rows of 2048 x 2048 characters, +2 / -3 {5, 2}: 64 lanes per pair, every lane of a wave busy
              (score: 64 lanes of which 32 own rows)

Timing: device events around >= 0.25 s of work (at least 4 calls) after a warm-up, the calls alternating between two sets of stores,
lists and outputs; the statistics and the score are timed in turn, twice each, and the smaller figure of each is printed; nothing here
was timed with a profiler attached.  Before timing, the device's scores and statistics of the sample are asserted equal to the host
twin's, and the scores and ends equal to the score kernel's on the whole list.

    python scripts/align_stats_lab.py reads|protein|long [--quick]     (--quick: an eighth of the pairs and short timings)
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
                                                         torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 6), dtype=torch.int32, device=dev),
                                                         torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev)]
             for s in sets]
    stream = ctypes.c_void_p(capi.raw_stream(dev))
    sample = idx[::64].copy()
    sample_cells = int((np.diff(sets[0][1])[::64] * np.diff(sets[0][3])[::64]).sum())
    head = "%-8s %s max_len %4d | %8d pairs, %7.2f G cells |" % (name, key, max_len, n, cells / 1e9)
    for mode in ("local", "global"):
        sc = capi.Score(max_len, 0, align._MODES[mode], o, e)
        np.ctypeslib.as_array(sc.matrix)[:matrix.shape[0], :matrix.shape[1]] = matrix

        def stats(i):
            ca, oa, cb, ob, row, col, score, st, _, _ = dsets[i & 1]
            capi.check(lib.bsq_align_stats_device(ctypes.byref(desc), ca.data_ptr(), oa.data_ptr(), n, cb.data_ptr(), ob.data_ptr(), n, row.data_ptr(),
                                                  col.data_ptr(), n, ctypes.byref(sc), score.data_ptr(), st.data_ptr(), stream))

        def score_ends(i):
            ca, oa, cb, ob, row, col, _, _, score, ends = dsets[i & 1]
            capi.check(lib.bsq_score_pairs_device(ctypes.byref(desc), ca.data_ptr(), oa.data_ptr(), n, cb.data_ptr(), ob.data_ptr(), n, row.data_ptr(),
                                                  col.data_ptr(), n, ctypes.byref(sc), score.data_ptr(), ends.data_ptr(), stream))

        t0 = time.perf_counter()
        host, host_stats = align.stats_pairs_host(tok, sets[0][0], sets[0][1], sample, sample, sets[0][2], sets[0][3], matrix=matrix, gap_open=o, gap_extend=e,
                                                  mode=mode, max_len=max_len)
        th = time.perf_counter() - t0
        stats(0), score_ends(0)
        torch.cuda.synchronize()
        got, got_stats, ref, ref_ends = (x.cpu().numpy() for x in dsets[0][6:10])
        assert np.array_equal(got[::64], host) and (host > align.CODE_BELOW).all() and np.array_equal(got_stats[::64], host_stats), "the device and the host twin differ"
        assert np.array_equal(got, ref) and np.array_equal(got_stats[:, 2:4], ref_ends), "the statistics and the score kernel differ in score or ends"
        ident = float(np.mean(got_stats[:, 4] / np.maximum(got_stats[:, 5], 1)))
        us_stats, us_score = [], []
        for _ in range(2):
            us_stats.append(timed(stats))
            us_score.append(timed(score_ends))
        us, ref_us = min(us_stats), min(us_score)
        print("%s %-26s %10.1f us per call, %8.2f M pairs/s, %8.1f G cells/s | %-29s %10.1f us, %8.1f G cells/s | ratio %.2f | mean identity %.3f | "
              "host twin, one thread, %d pairs: %.3f s, %.2f G cells/s | sample equal"
              % (head, align.stats_kernel_name(mode=mode, max_len=max_len), us, n / us, cells / us / 1e3, align.score_kernel_name(mode=mode, ends=True, max_len=max_len),
                 ref_us, cells / ref_us / 1e3, us / ref_us, ident, sample.size, th, sample_cells / th / 1e9), flush=True)


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
    measure(dev, "protein", "AMINO20", sets, 1024)


def part_long(dev):
    n = 4096 // SHRINK
    sets = []
    for seed in (5, 6):
        rng = np.random.default_rng(seed)
        sets.append(store(rng, np.full(n, 2048, np.int64), "ACGT") + store(rng, np.full(n, 2048, np.int64), "ACGT"))
    measure(dev, "long", "DNA4", sets, 2048)


def main():
    parts = {"reads": part_reads, "protein": part_protein, "long": part_long}
    chosen = [a for a in sys.argv[1:] if a in parts]
    if not chosen:
        sys.exit(__doc__)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    print("# alignment statistics of row pairs beside the score with ends: whole calls, buffers alternating; us per call", flush=True)
    for name in chosen:
        parts[name](dev)


if __name__ == "__main__":
    main()
