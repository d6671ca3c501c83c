#!/usr/bin/env python3
"""The sketch clusters (bsq_sketch_clusters_device: k_cluster_init + k_sketch_link + k_cluster_labels) against two yardsticks of the same
build: the count call of the pair list alone on the same input (the same walk of upper tiles, with no union), and the composition a user
would write without the call -- `sketch_pairs` (count + emit) and then label propagation in torch, `scatter_reduce(amin)` over both
directions of the list until nothing changes -- with equal labels asserted.  int32 sketches, upper, min_jaccard 0.5, min_match 1, at
N x S = 4096 x 128, 8192 x 1024, 131072 x 128 and 262144 x 128, on two kinds of input:

    sparse   seeded random DNA4 reads of 600 characters (k = 21, canonical), 3 % of the rows copies of an earlier row with 1 %
             substitutions: the generator of scripts/sketch_pairs_lab.py.  Most tiles have no hit.
    dense    one sketch row repeated N times: every pair passes, every tile is full of hits and the store is one cluster -- the case the
             cached roots exist for.  The composition exists only while the list of N (N - 1) / 2 pairs fits (20 bytes a pair with
             `either` dropped: 0.17 GB at 4096, 0.67 GB at 8192, 172 GB at 131072): it is run at the first two sizes and skipped beyond.

Timing: device events around >= 0.25 s of work (at least 4 calls, 2 at the two large sizes) after a warm-up, the calls alternating between
two sets of input, scratch and output buffers; the whole call is timed, the two small launches around the link launch included, as the
count call's two (three) small launches are.  Nothing here was timed with a profiler attached.

    python scripts/sketch_clusters_lab.py sparse|dense [--quick] [--sizes 4096x128,8192x1024]     (--quick: an eighth of the rows, short timings)
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402

from bioseq_amd import capi, sketch  # noqa: E402
import sketch_pairs_lab as pairs_lab  # noqa: E402  (the generator, the timer and the raw count / emit calls)

QUICK = "--quick" in sys.argv
SHRINK = 8 if QUICK else 1
SIZES = ((4096, 128), (8192, 1024), (131072, 128), (262144, 128))
LIST_LIMIT = 1 << 28  # pairs the composition may list (5 GB of row, col and match)
lib = sketch._lib


class Clusters:
    """the raw call on two alternating sets of buffers"""

    def __init__(self, dev, sk):
        self.B, self.S = sk.shape
        self.sets = [sk, sk.clone()]
        self.rule = capi.SketchPairs(1, pairs_lab.T_HALF, 1, 0)
        self.parent = [torch.empty(self.B, dtype=torch.int64, device=dev) for _ in range(2)]
        self.labels = [torch.empty(self.B, dtype=torch.int64, device=dev) for _ in range(2)]
        self.stream = ctypes.c_void_p(capi.raw_stream(dev))

    def call(self, i):
        a = self.sets[i & 1]
        capi.check(lib.bsq_sketch_clusters_device(a.data_ptr(), self.B, self.S, capi.I32, ctypes.byref(self.rule), self.parent[i & 1].data_ptr(),
                                                  self.labels[i & 1].data_ptr(), self.stream))


def propagate(row, col, n):
    """labels by propagation: every node takes the smallest label among itself and its neighbours until nothing changes"""
    lab = torch.arange(n, dtype=torch.int64, device=row.device)
    rounds = 0
    while True:
        new = lab.scatter_reduce(0, col, lab[row], "amin").scatter_reduce(0, row, lab[col], "amin")
        rounds += 1
        if torch.equal(new, lab):
            return lab, rounds
        lab = new


def composition(a):
    row, col = sketch.sketch_pairs(a, min_jaccard=0.5, either=False)[:2]
    return propagate(row, col, a.shape[0])


def measure(dev, kind, N, S, sk):
    least = 2 if N > 65536 else 4
    c = Clusters(dev, sk)
    c.call(0), c.call(1)
    torch.cuda.synchronize()
    assert torch.equal(c.labels[0], c.labels[1])
    labels = c.labels[0].clone()
    assert bool((labels <= torch.arange(N, device=dev)).all()) and torch.equal(labels[labels], labels)
    assert torch.equal(sketch.sketch_clusters(sk, min_jaccard=0.5), labels)
    nclusters = int((labels == torch.arange(N, device=dev)).sum())
    tl = pairs_lab.timed(c.call, least=least)
    p = pairs_lab.Pairs(dev, sk, True, 0, 1)
    p.sets = c.sets
    tc = pairs_lab.timed(p.count, least=least)
    total = int(p.offs[0][-1])
    del p
    line = ("%-6s N=%6d S=%5d pairs %11d clusters %7d | sketch_clusters %10.1f us | count call of sketch_pairs %10.1f us: clusters / count %5.2f"
            % (kind, N, S, total, nclusters, tl, tc, tl / tc))
    if total <= LIST_LIMIT:
        got, rounds = composition(sk)
        assert torch.equal(got, labels), "the composition and the call differ"
        tw = pairs_lab.timed(lambda i: composition(c.sets[i & 1]), least=least)
        line += " | sketch_pairs + propagation (%d rounds) %10.1f us: clusters / composition %5.2f | labels equal" % (rounds, tw, tl / tw)
    else:
        line += " | composition skipped: its list would be %.0f GB" % (total * 20 / 1e9)
    print(line, flush=True)


def part(dev, kind, sizes):
    print("# %s: N x S int32, upper, min_jaccard 0.5, min_match 1; us per call" % kind, flush=True)
    for N, S in sizes:
        N //= SHRINK
        sk = pairs_lab.sketches(dev, N + S, N if kind == "sparse" else 64, S)
        if kind == "dense":
            sk = sk[7:8].expand(N, S).contiguous()
        measure(dev, kind, N, S, sk)
        del sk
        torch.cuda.empty_cache()


def main():
    chosen = [a for a in sys.argv[1:] if a in ("sparse", "dense")]
    if not chosen:
        sys.exit(__doc__)
    sizes = SIZES
    if "--sizes" in sys.argv:
        sizes = tuple(tuple(int(v) for v in s.split("x")) for s in sys.argv[sys.argv.index("--sizes") + 1].split(","))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    for kind in chosen:
        part(dev, kind, sizes)


if __name__ == "__main__":
    main()
