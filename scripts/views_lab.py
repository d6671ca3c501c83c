#!/usr/bin/env python3
"""Views of a resident store (bsq_crop_packed_device): what cropping buys the shuffled loader, and what the crop kernel costs alone.

(a) loader step: FlatFileDataset.batches(4096) over a synthetic store, shuffled, int64 tokens and (B, C, P) float32 one-hot, cropped
    against not cropped -- crop=1024 on a long-tail store (most sequences 100-500 residues, a few of 35 000), crop=1000 on a store
    whose longest sequence is 1000 (the same width).  us per batch (host + device, the epoch's wall time over its batches) and bytes of the batch's encoded output.
(b) the crop kernel alone (raw ABI, back-to-back launches, event time): n x 1024-character windows of 2000-residue sequences, forward
    (revcomp_frac 0) and reverse-complemented (1), against bsq_gather_packed_device of n 1024-residue sequences (the same output
    bytes).  Bytes = read + write of the characters (2 n 1024) + the offsets; fraction of 8 TB/s.

    python scripts/views_lab.py [--quick]     (--quick: fewer repetitions, for a run under rocprofv3 --kernel-trace --stats)
"""
import ctypes
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bioseq_amd import Tokenizer, capi  # noqa: E402
from bioseq_amd.flatfile import FlatFile, write_flatfile  # noqa: E402
from bioseq_amd.loaders import FlatFileDataset  # noqa: E402

ROOF = 8e12  # bytes / s, the MI355X HBM3E peak


def store(path, n, lo, hi, outliers, rng):
    lens = rng.integers(lo, hi + 1, n)
    lens[rng.choice(n, outliers, replace=False)] = 35000
    pool = np.frombuffer(b"ACGT", np.uint8)
    seqs = [rng.choice(pool, int(L)).tobytes() for L in lens]
    return FlatFile(write_flatfile(seqs, path))


def loader(quick, tmp):
    rng = np.random.default_rng(1)
    dev = torch.device("cuda:0")
    tok = Tokenizer("DNA", True, True, True)
    # (the short store is cropped at its own longest sequence: the same width, so the step compares like for like)
    stores = {"long-tail (16384 seqs, 8 of 35000)": (store(os.path.join(tmp, "tail.ff"), 16384, 100, 500, 8, rng), 1024),
              "short (16384 seqs, longest 1000)": (store(os.path.join(tmp, "short.ff"), 16384, 100, 1000, 0, rng), 1000)}
    epochs = 2 if quick else 6
    for name, (ff, window) in stores.items():
        ff.to_device(dev)
        for cnn in (False, True):
            for crop in (None, window):
                ds = FlatFileDataset(ff, tok, device=dev, cnn=cnn, crop=crop, token_dtype="q")
                nbytes = 0
                for b in ds.batches(4096):  # warm-up epoch (allocator, first launches)
                    nbytes = b.numel() * b.element_size()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                nb = 0
                for _ in range(epochs):
                    for b in ds.batches(4096):
                        nb += 1
                torch.cuda.synchronize()
                us = (time.perf_counter() - t0) / nb * 1e6
                print("(a) %-36s %-10s crop=%-5s width %5d: %8.1f us per 4096-batch, %9.1f MB written per batch" %
                      (name, "(B,C,P) f32" if cnn else "int64 tok", crop, ds.max_seq_len, us, nbytes / 1e6), flush=True)


def kernel(quick):
    dev = torch.device("cuda:0")
    lib = capi.load()
    loops = 20 if quick else 200
    stream = ctypes.c_void_p(capi.raw_stream(dev))

    def timed(fn):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(loops):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / loops * 1e3

    W = 1024
    for n in (4096, 65536):
        rng = np.random.default_rng(n)
        nstore = max(n, 4096)
        long_ch = torch.from_numpy(rng.choice(np.frombuffer(b"ACGTN", np.uint8), nstore * 2000)).to(dev)
        long_of = torch.arange(0, (nstore + 1) * 2000, 2000, dtype=torch.int64, device=dev)
        short_ch = torch.from_numpy(rng.choice(np.frombuffer(b"ACGTN", np.uint8), nstore * W)).to(dev)
        short_of = torch.arange(0, (nstore + 1) * W, W, dtype=torch.int64, device=dev)
        idx = torch.randperm(nstore, device=dev)[:n].contiguous()
        out = torch.empty(n * W, dtype=torch.uint8, device=dev)
        out_of = torch.empty(n + 1, dtype=torch.int64, device=dev)
        nbytes = 2 * n * W + 8 * (n + 1) + 8 * n + 16 * n  # characters read + written, offsets written, index + source offsets read
        g = timed(lambda: lib.bsq_gather_packed_device(short_ch.data_ptr(), short_of.data_ptr(), nstore, idx.data_ptr(), n, out.data_ptr(),
                                                       n * W, out_of.data_ptr(), None, stream))
        print("(b) n=%6d x %d  gather_device (1024-residue rows)   %8.1f us  %.3f of 8 TB/s" % (n, W, g, nbytes / (g * 1e-6) / ROOF), flush=True)
        for frac in (0.0, 1.0):
            c = capi.Crop(W, capi.CROP_RANDOM, frac, 7, 0)
            t = timed(lambda: lib.bsq_crop_packed_device(long_ch.data_ptr(), long_of.data_ptr(), nstore, idx.data_ptr(), n, ctypes.byref(c),
                                                         out.data_ptr(), n * W, out_of.data_ptr(), None, None, None, stream))
            print("(b) n=%6d x %d  crop revcomp_frac=%.0f (2000-residue rows) %8.1f us  %.3f of 8 TB/s  (%.2fx the gather)" %
                  (n, W, frac, t, nbytes / (t * 1e-6) / ROOF, t / g), flush=True)


def main():
    quick = "--quick" in sys.argv
    torch.cuda.set_device(0)
    kernel(quick)
    with tempfile.TemporaryDirectory() as tmp:
        loader(quick, tmp)


if __name__ == "__main__":
    main()
