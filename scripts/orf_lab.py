#!/usr/bin/env python3
"""ORF extraction of a resident store (bsq_orf_count_device, bsq_orf_emit_device): what the kernels cost alone, on six-frame
translations of uniform A, C, G, T with min_len 30.

Shapes (the translate lab's): 262 144 x 512 characters, 1 M reads x 150, 4 096 contigs of 2 000 - 200 000.  Every figure is event-timed
over back-to-back launches that CYCLE over copies of the input (distinct random characters, more than 600 MiB in all), so no launch
finds its input in the 256 MiB Infinity Cache: the cold regime.  Per shape:
    the six-frame bsq_translate_packed_device launch that produces the residues (the yardstick: count + emit read two bytes per source
    character twice and do no table work);
    count (k_orf_count + k_orf_offsets), emit (k_orf_emit) and the bsq_views_packed_device launch that copies the ORFs out, each with
    its fraction of 8 TB/s on algorithmic bytes (count: residues + offsets read, offsets written; emit: residues + both offsets read,
    three arrays written; views: the arrays and the ORFs read, the ORFs and their offsets written);
    a torch composition that yields the same three arrays (== stop -> segment starts -> cumsum -> bincount -> filter -> searchsorted),
    checked equal on the first copy.

    python scripts/orf_lab.py [--quick]
    python scripts/orf_lab.py --pmc            one cold count + emit of 262 144 x 512 for a counters-only rocprofv3 --pmc run
    python scripts/orf_lab.py --pmc-read DIR   the counters of that run's k_orf_count and k_orf_emit dispatches
    python scripts/orf_lab.py --trace-read DIR the time of every kernel of a `rocprofv3 --kernel-trace` run of `orf_lab.py --quick`, by grid
"""
import csv
import ctypes
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bioseq_amd import capi, orfs, translate  # noqa: E402

ROOF = 8e12  # bytes / s, the MI355X HBM3E peak
COLD_BYTES = 600 << 20
MIN_LEN = 30
STOP = ord("*")


def make_store(lens, seed, dev):
    """(chars, offsets) on the device: uniform A, C, G, T."""
    g = torch.Generator(device=dev).manual_seed(seed)
    offs = torch.zeros(len(lens) + 1, dtype=torch.int64)
    offs[1:] = torch.cumsum(torch.as_tensor(lens, dtype=torch.int64), 0)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    chars = letters[torch.randint(0, 4, (int(offs[-1]),), device=dev, generator=g)]
    return chars, offs.to(dev)


def timed(fn, copies, loops):
    for k in range(min(copies, 3)):
        fn(k)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for k in range(loops):
        fn(k % copies)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / loops * 1e3


def torch_composition(chars, offsets, total):
    """(row, start, length) of the ORFs of a packed residue batch in the framework: no start-residue rule."""
    stop = chars[:total] == STOP
    begins = torch.zeros(total + 1, dtype=torch.bool, device=chars.device)
    begins[offsets[:-1]] = True   # a segment begins at every row's first residue
    begins[1:][stop] = True       # ... and behind every stop
    seg = torch.cumsum(begins[:total], 0)
    size = torch.bincount(seg[~stop], minlength=int(seg[-1]) + 1)[1:]  # residues of every segment, stops left out
    first = torch.nonzero(begins[:total]).squeeze(1)
    keep = size >= MIN_LEN
    first, size = first[keep], size[keep]
    row = torch.searchsorted(offsets, first, right=True) - 1
    return row, first - offsets[row], size


def shape(name, lens, quick, dev):
    lib = capi.load()
    stream = ctypes.c_void_p(capi.raw_stream(dev))
    n = len(lens)
    total = int(np.sum(lens))
    lens_np = np.asarray(lens, dtype=np.int64)
    n_out = 6 * n
    residues = 2 * sum(int(translate.translated_length(lens_np, c).sum()) for c in range(3))
    copies = max(2, -(-COLD_BYTES // total))
    loops = 2 * copies if quick else max(24, 6 * copies)
    t = translate._rule("six", 1, "X", "*")[0]
    rule = capi.Orf(STOP, -1, MIN_LEN)
    stores = [make_store(lens, 100 + k, dev) for k in range(copies)]
    prots = [(torch.empty(residues, dtype=torch.uint8, device=dev), torch.empty(n_out + 1, dtype=torch.int64, device=dev)) for _ in range(copies)]

    def run_translate(k):
        (ch, of), (pc, po) = stores[k], prots[k]
        capi.check(lib.bsq_translate_packed_device(ch.data_ptr(), of.data_ptr(), n, None, None, n, ctypes.byref(t), pc.data_ptr(), residues,
                                                   po.data_ptr(), None, stream))

    us_translate = timed(run_translate, copies, loops)
    del stores
    orf_offs = [torch.empty(n_out + 1, dtype=torch.int64, device=dev) for _ in range(copies)]
    sums = torch.empty(1, dtype=torch.int64, device=dev)

    def run_count(k):
        pc, po = prots[k]
        capi.check(lib.bsq_orf_count_device(pc.data_ptr(), po.data_ptr(), n_out, ctypes.byref(rule), orf_offs[k].data_ptr(), sums.data_ptr(), stream))

    us_count = timed(run_count, copies, loops)
    for k in range(copies):
        run_count(k)
    counts = [int(o[-1].item()) for o in orf_offs]
    bound = max(counts)
    arrays = [[torch.zeros(bound, dtype=torch.int64, device=dev) for _ in range(3)] for _ in range(copies)]

    def run_emit(k):
        pc, po = prots[k]
        r, s, ln = arrays[k]
        capi.check(lib.bsq_orf_emit_device(pc.data_ptr(), po.data_ptr(), n_out, ctypes.byref(rule), orf_offs[k].data_ptr(), bound,
                                           r.data_ptr(), s.data_ptr(), ln.data_ptr(), stream))

    us_emit = timed(run_emit, copies, loops)
    orf_bytes = [int(a[2].sum().item()) for a in arrays]
    out = torch.empty(max(orf_bytes), dtype=torch.uint8, device=dev)
    out_offs = torch.empty(bound + 1, dtype=torch.int64, device=dev)

    def run_views(k):
        pc, po = prots[k]
        r, s, ln = arrays[k]
        capi.check(lib.bsq_views_packed_device(pc.data_ptr(), po.data_ptr(), n_out, r.data_ptr(), s.data_ptr(), ln.data_ptr(), None, counts[k],
                                               out.data_ptr(), out.numel(), out_offs.data_ptr(), None, stream))

    us_views = timed(run_views, copies, loops)
    # the torch composition: the same arrays (checked on the first copy), fewer loops -- it allocates and synchronises
    row, start, length = torch_composition(prots[0][0], prots[0][1], residues)
    same = all(torch.equal(a, b[:counts[0]]) for a, b in zip((row, start, length), arrays[0]))
    del row, start, length
    us_torch = timed(lambda k: torch_composition(prots[k][0], prots[k][1], residues), copies, max(4, loops // 6))
    b_count = residues + 8 * (n_out + 1) + 8 * (n_out + 1)
    b_emit = residues + 16 * (n_out + 1) + 24 * counts[0]
    b_views = 24 * counts[0] + 2 * orf_bytes[0] + 8 * (counts[0] + 1)
    frac = lambda nbytes, us: nbytes / (us * 1e-6) / ROOF  # noqa: E731
    print("%-26s %8d rows %7.1f MB of residues, %d ORFs of %.1f MB" % (name, n_out, residues / 1e6, counts[0], orf_bytes[0] / 1e6))
    print("    translate six %9.1f us" % us_translate)
    print("    count         %9.1f us  %.3f of 8 TB/s on %7.1f MB" % (us_count, frac(b_count, us_count), b_count / 1e6))
    print("    emit          %9.1f us  %.3f of 8 TB/s on %7.1f MB" % (us_emit, frac(b_emit, us_emit), b_emit / 1e6))
    print("    views copy    %9.1f us  %.3f of 8 TB/s on %7.1f MB" % (us_views, frac(b_views, us_views), b_views / 1e6))
    print("    count + emit  %9.1f us = %.2fx the translate launch in front of them" % (us_count + us_emit, (us_count + us_emit) / us_translate))
    print("    torch composition %9.1f us (%s): count + emit are %.1fx faster" % (us_torch, "equal arrays" if same else "ARRAYS DIFFER",
                                                                                us_torch / (us_count + us_emit)), flush=True)


def pmc_launch(dev):
    """A warm-up count + emit on one batch, then ONE of each on another (268 MB of residues nobody has read)."""
    n, L = 262144, 512
    lens = np.full(n, L, dtype=np.int64)
    batches = [translate.translate_packed(*make_store(lens, seed, dev), frame="six", validate=False) for seed in (1, 2)]
    torch.cuda.synchronize()
    for pc, po in batches:
        row = orfs.find_orfs_packed(pc, po, min_len=MIN_LEN)[0]
        torch.cuda.synchronize()
    print("batch: %d rows, %d residues, %d ORFs" % (6 * n, int(batches[1][1][-1].item()), row.numel()))


def pmc_read(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True):
        with open(path) as fh:
            rows += list(csv.DictReader(fh))
    for kernel in ("k_orf_count", "k_orf_emit"):
        mine = [r for r in rows if kernel in r.get("Kernel_Name", "")]
        if not mine:
            print("no %s dispatch with counters under %s" % (kernel, directory))
            continue
        last = max(int(r["Dispatch_Id"]) for r in mine)
        for name in sorted({r["Counter_Name"] for r in mine}):
            value = sum(float(r["Counter_Value"]) for r in mine if r["Counter_Name"] == name and int(r["Dispatch_Id"]) == last)
            print("%s, the second (cold) launch: %s = %.0f" % (kernel, name, value))


def trace_read(directory):
    """Mean duration of every k_orf_* / k_translate_* / k_views_* dispatch of a `rocprofv3 --kernel-trace` run of this script, by kernel
    and grid size (a shape's launches share a grid)."""
    groups = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                found = re.search(r"k_(orf|translate|views)_[a-z0-9_]+(<[^>]*>)?", r.get("Kernel_Name", ""))
                if not found:
                    continue
                key = (found.group(0), int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0))
                groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (name, grid), us in sorted(groups.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        us.sort()
        print("grid %10d  %-40s %5d dispatches  median %9.1f us  mean %9.1f us" % (grid, name, len(us), us[len(us) // 2], sum(us) / len(us)))


def main():
    if "--pmc-read" in sys.argv:
        return pmc_read(sys.argv[sys.argv.index("--pmc-read") + 1])
    if "--trace-read" in sys.argv:
        return trace_read(sys.argv[sys.argv.index("--trace-read") + 1])
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    if "--pmc" in sys.argv:
        return pmc_launch(dev)
    quick = "--quick" in sys.argv
    rng = np.random.default_rng(16)
    print("cold regime: every launch of a loop reads a copy of its input the caches do not hold (copies cycle over > %d MiB); six frames, "
          "uniform ACGT, min_len %d" % (COLD_BYTES >> 20, MIN_LEN))
    shape("262144 x 512", np.full(262144, 512, dtype=np.int64), quick, dev)
    shape("1M reads x 150", np.full(1 << 20, 150, dtype=np.int64), quick, dev)
    shape("4096 contigs 2000-200000", rng.integers(2000, 200001, 4096), quick, dev)


if __name__ == "__main__":
    main()
