#!/usr/bin/env python3
"""The thresholded sketch pair list (bsq_sketch_pairs_count_device / bsq_sketch_pairs_emit_device) against the composition it replaces
-- sketch_compare -> threshold -> torch.nonzero on this same build -- and at a size the dense form cannot do.  int32 sketches of seeded
random DNA4 reads of 600 characters (k = 21, canonical), 3 % of the rows copies of an earlier row with 1 % substitutions.

    yardstick   N x N x S for 4096 x 128, 8192 x 1024 and 131072 x 128 (the dense matrices of the last are 137 GB of the device's 288, and
                twice the rows would be 550 GB): k_sketch_compare alone, the whole composition (threshold and nonzero in row blocks of
                2^30 elements), the count call, the emit call, their sum and `sketch_pairs` as Python calls it (with its 8-byte
                read-back); min_jaccard 0.5, min_match 1, cross (b = a given explicitly, every tile computed).  Results asserted equal.
    segments    the count call at 8192 x 8192 x 1024 and 4096 x 4096 x 128 for segments = 1, 2, 4, ... 64 and the library's choice (*).
    big         262144 x 262144 x 128, upper: count, emit, bucket pairs per second (the tiles on and above the diagonal), with the
                library's choice of segments and its neighbour.

Timing: device events around >= 0.25 s of work (at least 4 calls; `big`: 2 calls) after a warm-up, the calls alternating between two sets of
input and output buffers.  The inputs of one call are re-read from cache by design (a strip meets every tile of b), so a set is not
evicted between calls at the small sizes; nothing here was timed with a profiler attached.

    python scripts/sketch_pairs_lab.py yardstick|segments|big [--quick]     (--quick: an eighth of the rows and short timings)
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bioseq_amd import Tokenizer, capi, sketch  # noqa: E402

QUICK = "--quick" in sys.argv
SECONDS = 0.05 if QUICK else 0.25
SHRINK = 8 if QUICK else 1
L = 600
lib = sketch._lib
T_HALF = 32768  # min_jaccard 0.5


def sketches(dev, seed, B, S):
    """(B, S) int32 sketches of random reads, 3 % of them near-copies of an earlier row"""
    rng = np.random.default_rng(seed)
    chars = rng.integers(0, 4, (B, L), dtype=np.uint8)
    dup = rng.choice(np.arange(1, B), max(1, B * 3 // 100), replace=False)
    src = (rng.random(dup.size) * dup).astype(np.int64)  # an earlier row
    chars[dup] = chars[src]
    edits = rng.integers(0, L, (dup.size, L // 100))
    chars[dup[:, None], edits] = rng.integers(0, 4, edits.shape, dtype=np.uint8)
    chars = np.frombuffer(b"ACGT", np.uint8)[chars].reshape(-1)
    offs = np.arange(B + 1, dtype=np.int64) * L
    tok = Tokenizer("DNA4", False, False, False)
    return sketch.minhash_packed(tok, torch.from_numpy(chars).to(dev), torch.from_numpy(offs).to(dev), 21, S, canonical=True)


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


class Pairs:
    """the raw count and emit calls on two alternating sets of buffers"""

    def __init__(self, dev, sk, upper, segments, capacity):
        self.B, self.S = sk.shape
        self.sets = [sk, sk.clone()]
        self.rule = capi.SketchPairs(1, T_HALF, int(upper), segments)
        self.nseg = lib.bsq_sketch_pairs_segments(self.B, self.B, segments)
        self.segs = [torch.empty(self.B * self.nseg + 1, dtype=torch.int64, device=dev) for _ in range(2)]
        self.offs = [torch.empty(self.B + 1, dtype=torch.int64, device=dev) for _ in range(2)]
        self.cap = capacity
        self.out = [[torch.empty(capacity, dtype=dt, device=dev) for dt in (torch.int64, torch.int64, torch.int32, torch.int32)] for _ in range(2)]
        self.stream = ctypes.c_void_p(capi.raw_stream(dev))

    def count(self, i):
        a = self.sets[i & 1]
        capi.check(lib.bsq_sketch_pairs_count_device(a.data_ptr(), self.B, a.data_ptr(), self.B, self.S, capi.I32, ctypes.byref(self.rule),
                                                     self.segs[i & 1].data_ptr(), self.offs[i & 1].data_ptr(), self.stream))

    def emit(self, i):
        a = self.sets[i & 1]
        capi.check(lib.bsq_sketch_pairs_emit_device(a.data_ptr(), self.B, a.data_ptr(), self.B, self.S, capi.I32, ctypes.byref(self.rule),
                                                    self.segs[i & 1].data_ptr(), self.cap, *(o.data_ptr() for o in self.out[i & 1]), self.stream))

    def both(self, i):
        self.count(i), self.emit(i)


def composition(a, b):
    """what a user writes today: the dense matrices, the threshold in exact int32 arithmetic, nonzero, the values of the hits -- the
    last three in blocks of at most 2^30 elements: torch.nonzero refuses a mask of 2^31 elements, and the temporaries stay small"""
    m, e = sketch.sketch_compare(a, b)
    rows = max(1, (1 << 30) // b.shape[0])
    out = []
    for i0 in range(0, a.shape[0], rows):
        mm, ee = m[i0:i0 + rows], e[i0:i0 + rows]
        row, col = torch.nonzero((mm >= 1) & (mm * 65536 >= ee * T_HALF), as_tuple=True)
        out.append((row + i0, col, mm[row, col], ee[row, col]))
    return tuple(torch.cat(x) for x in zip(*out))


def part_yardstick(dev):
    print("# yardstick: N x N x S int32, cross, min_jaccard 0.5, min_match 1; us per call", flush=True)
    for N, S in ((4096, 128), (8192, 1024), (131072 // SHRINK, 128)):
        sk = sketches(dev, N + S, N, S)
        want = composition(sk, sk)
        total = want[0].numel()
        p = Pairs(dev, sk, False, 0, total)
        p.both(0), p.both(1)
        torch.cuda.synchronize()
        for k in range(2):
            assert int(p.offs[k][-1]) == total and all(torch.equal(x, y) for x, y in zip(p.out[k], want)), "the pair list and the composition differ"
        got = sketch.sketch_pairs(sk, sk, min_jaccard=0.5)
        assert all(torch.equal(x, y) for x, y in zip(got[:4], want))
        del want, got
        nd = 2 if 16 * N * N <= 100 << 30 else 1  # (the largest size has room for one set of dense outputs only)
        dense = [[torch.empty((N, N), dtype=torch.int32, device=dev) for _ in range(2)] for _ in range(nd)]

        def compare(i):
            a, (m, e) = p.sets[i & 1], dense[i % nd]
            capi.check(lib.bsq_sketch_compare_device(a.data_ptr(), N, a.data_ptr(), N, S, capi.I32, m.data_ptr(), e.data_ptr(), p.stream))

        td = timed(compare)
        del dense
        torch.cuda.empty_cache()
        tc, te, ts = timed(p.count), timed(p.emit), timed(p.both)
        tp = timed(lambda i: sketch.sketch_pairs(p.sets[i & 1], p.sets[i & 1], min_jaccard=0.5))
        tw = timed(lambda i: composition(p.sets[i & 1], p.sets[i & 1]))
        print("N=%6d S=%5d pairs %8d segments %2d | k_sketch_compare %10.1f (%5.2f T bucket pairs/s) | compare + threshold + nonzero %10.1f | "
              "count %10.1f emit %10.1f count + emit %10.1f = %.2fx the dense kernel, %.2fx the composition | sketch_pairs() %10.1f | results equal"
              % (N, S, total, p.nseg, td, N * N * S / td / 1e6, tw, tc, te, ts, ts / td, ts / tw, tp), flush=True)
        del p, sk
        torch.cuda.empty_cache()


def part_segments(dev):
    print("# segments: the count call, N x N x S int32, cross; us per call (*: the library's choice)", flush=True)
    for N, S in ((8192, 1024), (4096, 128)):
        sk = sketches(dev, N + S, N, S)
        chosen = lib.bsq_sketch_pairs_segments(N, N, 0)
        line = "N=%5d S=%5d strips %3d |" % (N, S, N // 64)
        for seg in (1, 2, 4, 8, 16, 32, 64):
            p = Pairs(dev, sk, False, seg, 1)
            line += " %2d%s %9.1f" % (p.nseg, "*" if p.nseg == chosen else " ", timed(p.count))
            del p
        print(line, flush=True)


def part_big(dev):
    N, S = 262144 // SHRINK, 128
    print("# big: %d x %d x %d int32, upper, min_jaccard 0.5, min_match 1; ms per call, bucket pairs of the tiles computed" % (N, N, S), flush=True)
    sk = sketches(dev, 7, N, S)
    tiles = (N // 64) * (N // 64 + 1) // 2
    chosen = lib.bsq_sketch_pairs_segments(N, N, 0)
    for seg in (chosen, 2 if chosen == 1 else chosen // 2):
        p = Pairs(dev, sk, True, seg, 1 << 24)
        tc, te = timed(p.count, least=2), timed(p.emit, least=2)
        total = int(p.offs[0][-1])
        assert total == int(p.offs[1][-1]) and total <= p.cap
        row, col = p.out[0][0][:total], p.out[0][1][:total]
        assert bool((row < col).all()) and bool(((row[1:] > row[:-1]) | ((row[1:] == row[:-1]) & (col[1:] > col[:-1]))).all()), "order"
        print("segments %2d%s | count %8.1f ms (%5.2f T/s) emit %8.1f ms (%5.2f T/s) sum %8.1f ms | %d pairs listed, first (%d, %d)"
              % (p.nseg, "*" if p.nseg == chosen else " ", tc / 1e3, tiles * 4096 * S / tc / 1e6, te / 1e3, tiles * 4096 * S / te / 1e6,
                 (tc + te) / 1e3, total, int(row[0]), int(col[0])), flush=True)
        del p
        torch.cuda.empty_cache()


def main():
    parts = {"yardstick": part_yardstick, "segments": part_segments, "big": part_big}
    chosen = [a for a in sys.argv[1:] if a in parts]
    if not chosen:
        sys.exit(__doc__)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    for name in chosen:
        parts[name](dev)


if __name__ == "__main__":
    main()
