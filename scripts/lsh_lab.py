#!/usr/bin/env python3
"""Banded LSH candidate search (`sketch.lsh_pairs`; include/bsq.h, "LSH candidates of a sketch matrix") against the all-pairs list
`sketch.sketch_pairs` of the same build, on the inputs of scripts/sketch_pairs_lab.py: int32 sketches of 128 buckets of seeded random
DNA4 reads of 600 characters (k = 21, canonical), 3 % of the rows copies of an earlier row with 1 % substitutions.  Beyond 262 144 rows
the store is made of blocks of 262 144 rows with seeds of their own (the copies stay inside a block) and `sketch_pairs` is no longer run.

    sizes    for 4096 ... 262 144 rows, then 1 Mi and 4 Mi: `lsh_pairs` (min_jaccard 0.5, rows_per_band = lsh_rows_per_band(128, 0.5),
             max_bucket 32) and `sketch_pairs` (b=None) as whole Python calls, read-backs included, in alternation; the share of
             `sketch_pairs`' list that `lsh_pairs` returns (the measured recall; the rest of its list must be empty) beside `lsh_recall`
             at 0.5; time per row; and the split of one `lsh_pairs` call over keys, sort, count + scan + emit, unique, list compare + rule.
    worst    one row repeated: with the centre rule (max_bucket 32) and without it (max_bucket = N, every pair of every band).
    keys     `k_lsh_keys` alone (band-major keys through the LDS image) beside the transpose torch would need if the kernel wrote
             (N, T) instead: `keys.t().contiguous()` of an (N, T) int64 matrix -- a lower bound on that alternative's extra cost.
    list     `sketch_compare_list` alone on long lists over 1 Mi rows -- neighbours (col = row + 1 ... 16: both sides near each other)
             and random columns (every b row a fresh 512-byte read) -- as bytes of rows read per second beside 8 TB/s.

Timing: a host clock around whole calls that end in a device synchronise (the calls read sizes back, so they cannot be enqueued ahead);
medians of ROUNDS windows, the two calls of a comparison taking turns; the stages of the split by device events around each stage of one
pipeline that repeats what `lsh_pairs` does.  Nothing here was timed with a profiler attached, and no counters-only run was taken.

    python scripts/lsh_lab.py [--quick] [--out PATH] [sizes] [worst] [keys] [list]      (default PATH: profiles/r29/lsh_lab.txt)
"""
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402

from bioseq_amd import capi, sketch  # noqa: E402
from sketch_pairs_lab import sketches  # noqa: E402

QUICK = "--quick" in sys.argv
ROUNDS = 3 if QUICK else 5
S = 128
BLOCK = 262144
SIZES = (4096, 16384) if QUICK else (4096, 16384, 65536, 262144, 1 << 20, 1 << 22)
lib = sketch._lib
_out = None


def say(line):
    print(line, flush=True)
    _out.write(line + "\n")
    _out.flush()


def store(dev, N):
    if N <= BLOCK:
        return sketches(dev, N + S, N, S)
    return torch.cat([sketches(dev, N + S + c, BLOCK, S) for c in range(N // BLOCK)])


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def medians(calls, rounds=ROUNDS):
    """{name: median seconds of a whole call}, the calls taking turns; each runs once before anything is timed"""
    for fn in calls.values():
        fn()
    times = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            times[name].append(wall(fn)[0])
    return {name: statistics.median(v) for name, v in times.items()}


def stages(a, r, max_bucket):
    """what `lsh_pairs(a)` does, stage by stage, with device events: ({stage: ms}, candidates before the union, after it)"""
    dev, N, T = a.device, a.shape[0], S // r
    rule = capi.Lsh(r, max_bucket, 0, 0)
    stream = ctypes.c_void_p(capi.raw_stream(dev))
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    marks[0].record()
    keys = torch.empty((T, N), dtype=torch.int64, device=dev)
    capi.check(lib.bsq_lsh_keys_device(a.data_ptr(), N, S, capi.I32, ctypes.byref(rule), keys.data_ptr(), N, stream))
    marks[1].record()
    keys, order = torch.sort(keys, dim=1, stable=True)
    marks[2].record()
    counts = torch.empty(T * N, dtype=torch.int64, device=dev)
    capi.check(lib.bsq_lsh_count_device(keys.data_ptr(), T, N, ctypes.byref(rule), counts.data_ptr(), stream))
    ends = torch.cumsum(counts, 0)
    total = int(ends[-1].item())
    codes = torch.empty(total, dtype=torch.int64, device=dev)
    capi.check(lib.bsq_lsh_emit_device(keys.data_ptr(), order.data_ptr(), T, N, ctypes.byref(rule), (ends - counts).data_ptr(), total,
                                       codes.data_ptr(), stream))
    marks[3].record()
    del keys, order, counts, ends
    codes = torch.unique(codes)
    row = torch.div(codes, N, rounding_mode="floor")
    col = codes - row * N
    marks[4].record()
    match, eith = sketch.sketch_compare_list(a, row, col)
    keep = (match >= 1) & (match.to(torch.int64) * 65536 >= eith.to(torch.int64) * 32768)
    n = int(keep.sum().item())
    marks[5].record()
    torch.cuda.synchronize()
    names = ("keys", "sort", "count + scan + emit", "unique", "list compare + rule")
    return {name: marks[k].elapsed_time(marks[k + 1]) for k, name in enumerate(names)}, total, codes.numel(), n


def part_sizes(dev):
    r = sketch.lsh_rows_per_band(S, 0.5)
    say("# sizes: N x %d int32, min_jaccard 0.5, rows_per_band %d (%d bands, lsh_recall(0.5) = %.4f), max_bucket 32; whole calls, ms (median of %d)"
        % (S, r, S // r, sketch.lsh_recall(0.5, r, S // r), ROUNDS))
    for N in SIZES:
        a = store(dev, N)
        calls = {"lsh": lambda: sketch.lsh_pairs(a, rows_per_band=r)}
        if N <= BLOCK:
            calls["all"] = lambda: sketch.sketch_pairs(a)
        t = medians(calls, ROUNDS if N <= BLOCK else 3)
        got = sketch.lsh_pairs(a, rows_per_band=r)
        line = "N=%8d | lsh_pairs %10.2f ms  %7.3f us/row  %7d pairs" % (N, t["lsh"] * 1e3, t["lsh"] * 1e6 / N, got[0].numel())
        if N <= BLOCK:
            full = sketch.sketch_pairs(a)
            fc, gc = full[0] * N + full[1], got[0] * N + got[1]
            found = int(torch.isin(fc, gc).sum().item())
            assert found == gc.numel(), "lsh_pairs lists a pair that sketch_pairs does not"
            line += " | sketch_pairs %10.2f ms  %7.3f us/row  %7d pairs  = %7.2fx | measured recall %.4f (%d of %d)" % (
                t["all"] * 1e3, t["all"] * 1e6 / N, fc.numel(), t["all"] / t["lsh"], found / max(1, fc.numel()), found, fc.numel())
            del full, fc, gc
        else:
            line += " | sketch_pairs not run"
        say(line)
        stages(a, r, 32)  # (warm)
        ms, before, after, n = stages(a, r, 32)
        say("           split (ms): " + "  ".join("%s %.2f" % kv for kv in ms.items()) + "  | sum %.2f | candidates %d before the union, %d after, %d pass"
            % (sum(ms.values()), before, after, n))
        del a, got
        torch.cuda.empty_cache()


def part_worst(dev):
    r = sketch.lsh_rows_per_band(S, 0.5)
    say("# worst: one row repeated N times (every band one run of N rows), rows_per_band %d; whole calls of lsh_pairs, ms" % r)
    one = sketches(dev, 99, 16, S)[3:4]
    for N in ((4096,) if QUICK else (4096, 262144, 1 << 20)):
        a = one.expand(N, S).contiguous()
        calls = {"centre": lambda: sketch.lsh_pairs(a, rows_per_band=r, max_bucket=32)}
        if N <= 4096:
            calls["all pairs"] = lambda: sketch.lsh_pairs(a, rows_per_band=r, max_bucket=N)
        t = medians(calls, 3)
        line = "N=%8d | centre rule (max_bucket 32) %10.2f ms, %d pairs listed" % (N, t["centre"] * 1e3, sketch.lsh_pairs(a, rows_per_band=r)[0].numel())
        if N <= 4096:
            n_all = sketch.lsh_pairs(a, rows_per_band=r, max_bucket=N)[0].numel()
            line += " | without it (max_bucket N) %10.2f ms, %d pairs listed from %d candidates before the union = %.1fx" % (
                t["all pairs"] * 1e3, n_all, (S // r) * N * (N - 1) // 2, t["all pairs"] / t["centre"])
        say(line)
        del a
        torch.cuda.empty_cache()


def part_keys(dev):
    r = sketch.lsh_rows_per_band(S, 0.5)
    T = S // r
    say("# keys: k_lsh_keys alone, N x %d int32 -> (%d, N) int64, beside torch's transpose of an (N, %d) int64 matrix; device events, median of %d, ms"
        % (S, T, T, ROUNDS))

    def events(fn):
        fn()
        times = []
        for _ in range(ROUNDS):
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            times.append(b.elapsed_time(e))
        return statistics.median(times)

    for N in ((65536,) if QUICK else (262144, 1 << 20, 1 << 22)):
        a = store(dev, N)
        tk = events(lambda: sketch.lsh_keys(a, r))
        wide = sketch.lsh_keys(a, r).t().contiguous()  # (N, T): what a lane-per-(row, band) kernel would write without the LDS image
        tt = events(lambda: wide.t().contiguous())
        moved = N * S * 4 + T * N * 8
        say("N=%8d | k_lsh_keys %8.3f ms (%.2f TB/s of sketches read and keys written) | (N, T) -> (T, N) in torch %8.3f ms = %.2fx the whole kernel"
            % (N, tk, moved / tk / 1e9, tt, tt / tk))
        del a, wide
        torch.cuda.empty_cache()


def part_list(dev):
    N = (1 << 17) if QUICK else (1 << 20)
    P = (1 << 21) if QUICK else (1 << 24)
    say("# list: sketch_compare_list alone, %d pairs over %d x %d int32 rows (%s), sorted by row; device events, median of %d"
        % (P, N, S, sketch.lsh_kernel_name(S).split(";")[1], ROUNDS))
    a = store(dev, N)
    gen = torch.Generator(device=dev).manual_seed(5)
    row = torch.sort(torch.randint(0, N - 16, (P,), generator=gen, device=dev))[0]
    lists = {"neighbours (col = row + 1 .. 16)": row + torch.randint(1, 17, (P,), generator=gen, device=dev),
             "random columns": torch.randint(0, N, (P,), generator=gen, device=dev)}
    for name, col in lists.items():
        sketch.sketch_compare_list(a, row, col)
        times = []
        for _ in range(ROUNDS):
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record()
            sketch.sketch_compare_list(a, row, col)
            e.record()
            torch.cuda.synchronize()
            times.append(b.elapsed_time(e))
        ms = statistics.median(times)
        rows_bytes = 2 * P * S * 4
        say("%-34s %9.3f ms | %6.1f M pairs/s | rows read %.2f TB/s = %.0f %% of 8 TB/s (the list and the outputs add %.0f %% to the bytes)"
            % (name, ms, P / ms / 1e3, rows_bytes / ms / 1e9, rows_bytes / ms / 1e9 / 8 * 100, 24 * P / rows_bytes * 100))


def main():
    global _out
    parts = {"sizes": part_sizes, "worst": part_worst, "keys": part_keys, "list": part_list}
    chosen = [p for p in sys.argv[1:] if p in parts] or list(parts)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r29", "lsh_lab.txt")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    with open(path, "a" if "--append" in sys.argv else "w") as _out:
        say("# scripts/lsh_lab.py %s on %s" % (" ".join(p for p in sys.argv[1:] if p in parts or p == "--quick"), torch.cuda.get_device_name(0)))
        for name in chosen:
            parts[name](dev)


if __name__ == "__main__":
    main()
