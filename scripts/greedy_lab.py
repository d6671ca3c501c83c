#!/usr/bin/env python3
"""Greedy representatives of an edge list (bsq_greedy_pairs_device: rounds of k_greedy_mark + k_greedy_decide, then the assignment) against
three yardsticks of the same build, on one device, with equal results asserted:

    cluster_pairs   the connected components of the same list: one union-find launch between two small ones.  The ratio to it is the
                    price of the rounds.
    torch rounds    the composition a user would write without the call: the same rounds in torch -- entries oriented once, marks by
                    `scatter_reduce(amax)`, masked state updates, one read-back a round to stop, a final `scatter_reduce(amin)` -- for
                    index order without weights.
    host twin       `greedy_pairs_host` (the sequential visit) on one thread, timed once.

Lists:
    sparse NxS   what `sketch_pairs(min_jaccard=0.5)` lists on seeded random DNA4 reads with 3 % planted near-duplicates (the generator of
                 scripts/sketch_pairs_lab.py) at the sizes of profiles/r21/sketch_clusters_lab.txt; n = N.
    cliques      65 536 nodes: four cliques of 1500 nodes each and 100 000 random entries.
    path         the path of 300 nodes in index order: 300 rounds in which nothing else happens -- what a round costs.
    random       2^21 nodes, 2^25 random entries (512 MiB of row and col): what a round costs when the list is the cost.

The device call is timed three ways: `greedy` as `greedy_pairs` runs it by default (16 rounds a call, doubling, an 8-byte read-back after
every call), `one call` with max_rounds = the rounds the list needs and nothing read back, and `key+weight` (one call, a random key with
ties and a random weight with ties: all three assignment passes).  Whole calls, a host clock around work that ends in a synchronise,
the calls alternating in one process; every figure is the median of ROUNDS windows and `spread` is (max - min) / median of the default
call's windows.  Per round: (one call - a call of 0 rounds) / rounds, against the time the list's bytes (16 a entry) take at 8 TB/s.
Nothing here was timed with a profiler attached.

    python scripts/greedy_lab.py [--quick] [sparse] [cliques] [path] [random]      (--quick: small sizes, short windows)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bioseq_amd import sketch  # noqa: E402

QUICK = "--quick" in sys.argv
ROUNDS = 3 if QUICK else 7
WINDOW = 0.01 if QUICK else 0.05  # seconds of work per window
SPARSE = ((4096, 128), (8192, 1024)) if QUICK else ((4096, 128), (8192, 1024), (131072, 128), (262144, 128))


def torch_rounds(row, col, n):
    """index order, no weights: (rep, rounds)"""
    ok = (row != col) & (row >= 0) & (row < n) & (col >= 0) & (col < n)
    row, col = row[ok], col[ok]
    u, v = torch.minimum(row, col), torch.maximum(row, col)
    state = torch.zeros(n, dtype=torch.int64, device=row.device)  # 0 undecided, 1 representative, 2 member
    rounds = 0
    while True:
        su = state[u]
        live = (state[v] == 0) & (su != 2)
        mark = torch.zeros(n, dtype=torch.int64, device=row.device).scatter_reduce(0, v[live], 2 + (su[live] == 1).to(torch.int64), "amax")
        open_ = state == 0
        state = torch.where(open_ & (mark == 3), 2, torch.where(open_ & (mark == 0), 1, state))
        rounds += 1
        if not bool((state == 0).any()):
            break
    cand = (state[v] == 2) & (state[u] == 1)
    ident = torch.arange(n, dtype=torch.int64, device=row.device)
    first = torch.full((n,), n, dtype=torch.int64, device=row.device).scatter_reduce(0, v[cand], u[cand], "amin")
    return torch.where(state == 2, first, ident), rounds


def rounds_needed(row, col, n, **kw):
    """the fewest rounds after which nothing is left (the count falls with every round: a bisection)"""
    left = lambda r: int(sketch.greedy_pairs(row, col, n, max_rounds=r, **kw)[1])
    if left(0) == 0:
        return 0
    lo, hi = 0, 8
    while left(hi) > 0:
        lo, hi = hi, hi * 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if left(mid) > 0 else (lo, mid)
    return hi


def windows(calls):
    """{name: [seconds per call, one per round]}: in every round each call gets one window of ~WINDOW seconds, in turn"""
    reps = {}
    for name, fn in calls.items():
        fn(), torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(), torch.cuda.synchronize()
        reps[name] = max(1, int(WINDOW / max(time.perf_counter() - t0, 1e-6)))
    out = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) / reps[name])
    return out


def measure(name, row, col, n, host=True):
    dev, m = row.device, row.numel()
    rep = sketch.greedy_pairs(row, col, n)
    needed = rounds_needed(row, col, n)
    readbacks, done, step = 0, 0, 16
    while True:
        readbacks, done, step = readbacks + 1, done + step, step * 2
        if done >= needed:
            break
    got, torch_needed = torch_rounds(row, col, n)
    assert torch.equal(got, rep), "the torch rounds and the call differ"
    assert torch_needed == max(needed, 1)
    one, left = sketch.greedy_pairs(row, col, n, max_rounds=needed)
    assert int(left) == 0 and torch.equal(one, rep)
    g = torch.Generator(device="cpu").manual_seed(n + m)
    key = torch.randint(-3, 4, (n,), generator=g).to(dev)
    weight = torch.randint(-2, 3, (m,), generator=g, dtype=torch.int32).to(dev)
    kw_rounds = rounds_needed(row, col, n, key=key, weight=weight)
    small = n <= 1 << 17
    if small:
        assert np.array_equal(sketch.greedy_pairs_host(row.cpu().numpy(), col.cpu().numpy(), n, key=key.cpu().numpy(), weight=weight.cpu().numpy()),
                              sketch.greedy_pairs(row, col, n, key=key, weight=weight).cpu().numpy())
    t = windows({
        "greedy": lambda: sketch.greedy_pairs(row, col, n),
        "one call": lambda: sketch.greedy_pairs(row, col, n, max_rounds=needed),
        "no round": lambda: sketch.greedy_pairs(row, col, n, max_rounds=0),
        "key+weight": lambda: sketch.greedy_pairs(row, col, n, key=key, weight=weight, max_rounds=kw_rounds),
        "cluster_pairs": lambda: sketch.cluster_pairs(row, col, n),
        "torch rounds": lambda: torch_rounds(row, col, n),
    })
    med = {k: float(np.median(v)) * 1e6 for k, v in t.items()}
    spread = (max(t["greedy"]) - min(t["greedy"])) / float(np.median(t["greedy"]))
    per_round = (med["one call"] - med["no round"]) / max(needed, 1)
    floor = m * 16 / 8e12 * 1e6
    line = ("%-16s n=%8d entries %9d reps %8d rounds %3d read-backs %d | greedy %10.1f us (spread %4.1f %%) | one call %10.1f us | key+weight (%d rounds) %10.1f us"
            " | cluster_pairs %9.1f us: greedy / cluster_pairs %6.2f | torch rounds %10.1f us: greedy / torch %5.2f | a round %8.2f us, its list at 8 TB/s %7.2f us"
            % (name, n, m, int((rep == torch.arange(n, device=dev)).sum()), needed, readbacks, med["greedy"], spread * 100, med["one call"], kw_rounds,
               med["key+weight"], med["cluster_pairs"], med["greedy"] / med["cluster_pairs"], med["torch rounds"], med["greedy"] / med["torch rounds"],
               per_round, floor))
    if host:
        r, c = row.cpu().numpy(), col.cpu().numpy()
        t0 = time.perf_counter()
        want = sketch.greedy_pairs_host(r, c, n)
        line += " | host twin %10.1f us" % ((time.perf_counter() - t0) * 1e6)
        assert np.array_equal(want, rep.cpu().numpy()), "the host twin and the call differ"
    print(line + " | results equal", flush=True)


def part_sparse(dev):
    import sketch_pairs_lab as pairs_lab
    for N, S in SPARSE:
        sk = pairs_lab.sketches(dev, N + S, N, S)
        row, col, *_ = sketch.sketch_pairs(sk, min_jaccard=0.5, either=False)
        del sk
        torch.cuda.empty_cache()
        measure("sparse %dx%d" % (N, S), row, col, N)


def part_cliques(dev):
    n, size, extra = (8192, 200, 10000) if QUICK else (65536, 1500, 100000)
    rng = np.random.default_rng(5)
    rows, cols = [rng.integers(0, n, extra)], [rng.integers(0, n, extra)]
    for _ in range(4):
        nodes = rng.choice(n, size, replace=False)
        i, j = np.triu_indices(size, 1)
        rows.append(nodes[i]), cols.append(nodes[j])
    p = rng.permutation(sum(r.size for r in rows))
    measure("cliques", torch.from_numpy(np.concatenate(rows)[p].astype(np.int64)).to(dev), torch.from_numpy(np.concatenate(cols)[p].astype(np.int64)).to(dev), n)


def part_path(dev):
    a = torch.arange(299, dtype=torch.int64, device=dev)
    measure("path", a, a + 1, 300)


def part_random(dev):
    n, m = (1 << 16, 1 << 20) if QUICK else (1 << 21, 1 << 25)
    g = torch.Generator(device="cpu").manual_seed(9)
    measure("random", torch.randint(0, n, (m,), generator=g).to(dev), torch.randint(0, n, (m,), generator=g).to(dev), n)


def main():
    parts = {"sparse": part_sparse, "cliques": part_cliques, "path": part_path, "random": part_random}
    chosen = [a for a in sys.argv[1:] if a in parts] or list(parts)
    if not torch.cuda.is_available():
        sys.exit("greedy_lab.py measures on a device: none is visible")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    print("# greedy representatives: us per whole call, medians of %d windows of >= %.0f ms, calls alternating in one process" % (ROUNDS, WINDOW * 1e3), flush=True)
    for name in chosen:
        parts[name](dev)


if __name__ == "__main__":
    main()
