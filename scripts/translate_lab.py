#!/usr/bin/env python3
"""Codon translation of a resident store (bsq_translate_packed_device): what the kernels cost alone, on DNA4-like input.

Shapes: 1 M reads x 150 (frame 0, six frames), 262 144 x 512 (frame 0, frame 4, six frames), 4 096 contigs of 2 000 - 200 000 (six
frames).  Every figure is event-timed over back-to-back launches that CYCLE over copies of the store (distinct random characters, more
than 512 MiB of input in all), so no launch finds its input in the 256 MiB Infinity Cache: the cold regime.  Per shape:
    time;  the fraction of 8 TB/s on algorithmic bytes = characters read once + residues written + offsets read and written;
    the ratio to views.gather_views of the same rows in the same run (a copy reading the same bytes and writing three times as many:
    the nearest byte-rate yardstick the library has; reported, not gated);
    on the rectangular shapes the ratio to the torch composition lut[chars] -> (B, m, 3) -> weighted sum -> table gather (plus a flip
    and the complement for the reverse frame), which handles no unknown codon and no ragged store.

    python scripts/translate_lab.py [--quick]
    python scripts/translate_lab.py --pmc            one six-frame launch of 262 144 x 512 for a counters-only rocprofv3 --pmc run
    python scripts/translate_lab.py --pmc-read DIR   FETCH_SIZE of that run's k_translate_place dispatch against the store's bytes
"""
import csv
import ctypes
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bioseq_amd import capi, translate  # noqa: E402

ROOF = 8e12  # bytes / s, the MI355X HBM3E peak
COLD_BYTES = 600 << 20


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


def rule(frame):
    return translate._rule(frame, 1, "X", "*")[0]


def torch_composition(chars2d, frame, tables):
    """The framework's way on a rectangular batch (B, L): residues (B, m).  No unknown codon, no ragged rows."""
    lut, comp_lut, table = tables
    f = frame % 3
    B, L = chars2d.shape
    m = (L - f) // 3
    x = chars2d if frame < 3 else torch.flip(chars2d, (1,))
    codes = torch.index_select(comp_lut if frame >= 3 else lut, 0, x[:, f:f + 3 * m].reshape(-1).int()).view(B, m, 3)
    idx = codes[..., 0] * 16 + codes[..., 1] * 4 + codes[..., 2]
    return torch.index_select(table, 0, idx.reshape(-1).int()).view(B, m)


def shape(name, lens, frames, rect, quick, dev):
    lib = capi.load()
    stream = ctypes.c_void_p(capi.raw_stream(dev))
    n = len(lens)
    total = int(np.sum(lens))
    copies = max(2, -(-COLD_BYTES // total))
    stores = [make_store(lens, 100 + k, dev) for k in range(copies)]
    loops = 2 * copies if quick else max(24, 6 * copies)
    lens_np = np.asarray(lens, dtype=np.int64)
    # the torch composition's tables: NCBI numbers T C A G
    lut = torch.zeros(256, dtype=torch.uint8, device=dev)
    comp_lut = torch.zeros(256, dtype=torch.uint8, device=dev)
    for ch, num in ((b"T", 0), (b"C", 1), (b"A", 2), (b"G", 3)):
        lut[ch[0]] = num
        comp_lut[ch[0]] = (num + 2) % 4
    table = torch.from_numpy(translate.codon_table(1)).to(dev)
    seq = torch.arange(n, dtype=torch.int64, device=dev)
    zero = torch.zeros(n, dtype=torch.int64, device=dev)
    length = stores[0][1][1:] - stores[0][1][:-1]
    ones = torch.ones(n, dtype=torch.uint8, device=dev)
    copy_out = torch.empty(total, dtype=torch.uint8, device=dev)
    copy_offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    for frame in frames:
        six = frame == "six"
        t = rule(frame)
        n_out = 6 * n if six else n
        residues = (2 * sum(int(translate.translated_length(lens_np, c).sum()) for c in range(3)) if six
                    else int(translate.translated_length(lens_np, frame).sum()))
        out = torch.empty(residues, dtype=torch.uint8, device=dev)
        out_offs = torch.empty(n_out + 1, dtype=torch.int64, device=dev)

        def run(k):
            ch, of = stores[k]
            capi.check(lib.bsq_translate_packed_device(ch.data_ptr(), of.data_ptr(), n, None, None, n, ctypes.byref(t), out.data_ptr(), residues,
                                                       out_offs.data_ptr(), None, stream))

        def copy(k):  # views.gather_views of the same rows, the strand of the frame
            ch, of = stores[k]
            capi.check(lib.bsq_views_packed_device(ch.data_ptr(), of.data_ptr(), n, seq.data_ptr(), zero.data_ptr(), length.data_ptr(),
                                                   ones.data_ptr() if (not six and frame >= 3) else None, n, copy_out.data_ptr(), total,
                                                   copy_offs.data_ptr(), None, stream))

        us = timed(run, copies, loops)
        us_copy = timed(copy, copies, loops)
        nbytes = total + residues + 8 * (n + 1) + 8 * (n_out + 1)
        line = "%-28s frame %-3s %9.1f us  %.3f of 8 TB/s on %7.1f MB  | gather_views %9.1f us: %.2fx its time" % (
            name, frame, us, nbytes / (us * 1e-6) / ROOF, nbytes / 1e6, us_copy, us / us_copy)
        if rect:
            L = int(lens[0])
            tables = (lut, comp_lut, table)
            codes = range(6) if six else [frame]
            us_torch = timed(lambda k: [torch_composition(stores[k][0].view(n, L), c, tables) for c in codes], copies, max(4, loops // 4))
            line += "  | torch composition %9.1f us: %.2fx faster than it" % (us_torch, us_torch / us)
        print(line, flush=True)
    del stores


def pmc_launch(dev):
    """One warm-up launch on one store, then ONE six-frame launch on another (134 MB of characters nobody has read)."""
    n, L = 262144, 512
    lens = np.full(n, L, dtype=np.int64)
    a, b = make_store(lens, 1, dev), make_store(lens, 2, dev)
    translate.translate_packed(*a, frame="six", validate=False)
    torch.cuda.synchronize()
    translate.translate_packed(*b, frame="six", validate=False)
    torch.cuda.synchronize()
    print("store: %d characters, six frames: %d residues" % (n * L, 2 * sum((L - f) // 3 for f in range(3)) * n))


def pmc_read(directory):
    n, L = 262144, 512
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True):
        with open(path) as fh:
            rows += [r for r in csv.DictReader(fh) if "k_translate_place" in r.get("Kernel_Name", "")]
    if not rows:
        print("no k_translate_place dispatch with counters under %s" % directory)
        return
    last = max(int(r["Dispatch_Id"]) for r in rows)
    for name in sorted({r["Counter_Name"] for r in rows}):
        value = sum(float(r["Counter_Value"]) for r in rows if r["Counter_Name"] == name and int(r["Dispatch_Id"]) == last)
        print("k_translate_place, the second (cold) six-frame launch: %s = %.0f" % (name, value))
        if name == "FETCH_SIZE":  # kilobytes fetched from memory by the L2s
            print("   = %.1f MB against %.1f MB of source characters: %.2f reads of the source" % (value * 1024 / 1e6, n * L / 1e6, value * 1024 / (n * L)))


def main():
    if "--pmc-read" in sys.argv:
        return pmc_read(sys.argv[sys.argv.index("--pmc-read") + 1])
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    if "--pmc" in sys.argv:
        return pmc_launch(dev)
    quick = "--quick" in sys.argv
    rng = np.random.default_rng(16)
    print("cold regime: every launch of a loop reads a store copy the caches do not hold (copies cycle over > %d MiB)" % (COLD_BYTES >> 20))
    shape("1M reads x 150", np.full(1 << 20, 150, dtype=np.int64), [0, "six"], True, quick, dev)
    shape("262144 x 512", np.full(262144, 512, dtype=np.int64), [0, 4, "six"], True, quick, dev)
    shape("4096 contigs 2000-200000", rng.integers(2000, 200001, 4096), ["six"], False, quick, dev)


if __name__ == "__main__":
    main()
