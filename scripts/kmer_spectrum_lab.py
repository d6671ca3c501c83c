#!/usr/bin/env python3
"""k-mer spectra of packed batches (bsq_kmer_spectrum_device): both kernel forms against the roof and against the torch composition a
user writes without the call, taken in the same run:

    ids = kmer_tokenize_packed(int64, PAD = V + 1)  ->  + row * V  ->  mask ids < V  ->  scatter_add_ of ones into a zeroed (B, V) float32
    matrix (both strands: a second scatter_add_ through the table of reverse-complement ids)

which is asserted to produce the same tensor at the timed size; the first rows are also compared with the numpy twin
(tests/kmer_spectrum_twin.py).  Seeded synthetic data (1 % unmapped characters), float32 counts:

    1 048 576 DNA4 reads x 150, k = 4 and 6        262 144 DNA4 reads x 512, k = 6
    65 536 protein-like rows of 50 .. 1024 residues (AMINO20), k = 2 and 3
    4 096 contigs of 2 000 .. 200 000 characters (DNA4), k = 4, both strands

For each shape: form 1 (a wave per row) and form 2 (a workgroup per row) where both apply, the form the library picks from
total_chars, the same launch on a poly-A batch of the same offsets (every lane on one LDS bin: the worst case of the atomics), and the
launch with normalize = 1.  cold: the calls cycle over distinct batches and outputs of more than 512 MiB together.  Device events around
>= 0.25 s of work per figure after a warm-up.  Bytes = characters + offsets + the (B, V) output, against 8 TB/s.

    python scripts/kmer_spectrum_lab.py [--quick]     (--quick: a sixteenth of the rows and short timings)
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kmer_spectrum_twin as twin  # noqa: E402
from bioseq_amd import Tokenizer, kmers  # noqa: E402

ROOF = 8e12
DNA = np.frombuffer(b"ACGT" * 25 + b"N", np.uint8)
AMINO = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY" * 5 + b"X", np.uint8)


def batch(seed, lens, pool):
    rng = np.random.default_rng(seed)
    offs = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return rng.choice(pool, int(offs[-1])).astype(np.uint8), offs


def timed(fn, seconds):
    for _ in range(3):
        fn(0)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(4):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    reps = max(4, int(seconds / max(a.elapsed_time(b) / 4e3, 1e-6)))
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us


def composition(padded, dch, dof, k, V, maxlen, both, rc):
    B = dof.numel() - 1
    ids = kmers.kmer_tokenize_packed(padded, dch, dof, k, max(1, maxlen - k + 1), "q", True, validate=False)
    keep = ids < V
    rows = (torch.arange(B, device=ids.device) * V)[:, None]
    out = torch.zeros(B * V, dtype=torch.float32, device=ids.device)
    idx = (ids + rows)[keep]
    ones = torch.ones(idx.numel(), dtype=torch.float32, device=ids.device)
    out.scatter_add_(0, idx, ones)
    if both:
        out.scatter_add_(0, (rc[ids.clamp(max=V - 1)] + rows)[keep], ones)
    return out.view(B, V)


def main():
    quick = "--quick" in sys.argv
    seconds = 0.05 if quick else 0.25
    shrink = 16 if quick else 1
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    rng = np.random.default_rng(1)
    shapes = [
        ("reads 150", "DNA4", 4, False, np.full(1048576 // shrink, 150, np.int64), DNA),
        ("reads 150", "DNA4", 6, False, np.full(1048576 // shrink, 150, np.int64), DNA),
        ("reads 512", "DNA4", 6, False, np.full(262144 // shrink, 512, np.int64), DNA),
        ("proteins", "AMINO20", 2, False, rng.integers(50, 1025, 65536 // shrink).astype(np.int64), AMINO),
        ("proteins", "AMINO20", 3, False, rng.integers(50, 1025, 65536 // shrink).astype(np.int64), AMINO),
        ("contigs", "DNA4", 4, True, rng.integers(2000, 200001, 4096 // shrink).astype(np.int64), DNA),
    ]
    print("# scripts/kmer_spectrum_lab.py: float32 counts, stride 1; us per call (device events, cold), fraction of 8 TB/s on characters + "
          "offsets + output", flush=True)
    lib = kmers._lib
    for label, key, k, both, lens, pool in shapes:
        tok, padded = Tokenizer(key, False, False, False), Tokenizer(key, False, False, True)
        desc, km = kmers.capi.desc_of(tok), kmers.capi.Kmer(k, 1)
        V, B, maxlen = kmers.kmer_spectrum_width(tok, k), lens.size, int(lens.max())
        host = [batch(100 + i, lens, pool) for i in range(2)]
        total = int(host[0][1][-1])
        nbytes = total + (B + 1) * 8 + B * V * 4
        nsets = max(2, -(-(600 << 20) // (total + B * V * 4)) + 1)
        sets = [(torch.from_numpy(host[i % 2][0]).to(dev), torch.from_numpy(host[i % 2][1]).to(dev)) for i in range(nsets)]
        poly = [(torch.full_like(c, ord("A")), o) for c, o in sets]
        outs = [torch.empty((B, V), dtype=torch.float32, device=dev) for _ in range(nsets)]
        rc = torch.from_numpy(twin.rc_ids(V, k)).to(dev) if both else None
        stream = ctypes.c_void_p(kmers.capi.raw_stream(dev))
        lut = np.frombuffer(bytes(desc.lut), dtype=np.int8)

        def call(i, form, data=sets, normalize=0):
            c, o = data[i % nsets]
            opt = kmers.capi.KmerSpectrum(int(both), normalize, form, 0, total)
            lib.bsq_kmer_spectrum_device(ctypes.byref(desc), c.data_ptr(), o.data_ptr(), B, ctypes.byref(km), ctypes.byref(opt), 4,
                                         outs[i % nsets].data_ptr(), stream)

        comp = composition(padded, *sets[0], k, V, maxlen, both, rc)
        chosen = kmers.kmer_spectrum_kernel_name(tok, k, B, "f", both_strands=both, total_chars=total)
        head = min(B, 512)
        want = twin.spectrum(lut, desc.nchars, host[0][0], host[0][1][:head + 1], k, 1, 4, both, False)
        for form in ((1, 2) if V <= 1024 else (2,)):
            got = kmers.kmer_spectrum_packed(tok, *sets[0], k, "f", both_strands=both, form=form, validate=False)
            assert torch.equal(got, comp), "the call and the torch composition differ"
            assert got[:head].cpu().numpy().tobytes() == want.tobytes(), "the call and the numpy twin differ"
            del got
            name = kmers.kmer_spectrum_kernel_name(tok, k, B, "f", both_strands=both, form=form)
            t = timed(lambda i: call(i, form), seconds)
            tp = timed(lambda i: call(i, form, poly), seconds)
            tn = timed(lambda i: call(i, form, normalize=1), seconds)
            print("%-9s %-7s k=%d V=%5d B=%7d mean L %6.0f %s | %-28s%s %9.1f us %.3f of roof | poly-A %9.1f us = %5.2fx | frequencies %9.1f us"
                  % (label, key, k, V, B, total / B, "both" if both else "one ", name, "*" if name == chosen else " ", t,
                     nbytes / (t * 1e-6) / ROOF, tp, tp / t, tn), flush=True)
        del comp
        tc = timed(lambda i: composition(padded, *sets[i % nsets], k, V, maxlen, both, rc), seconds)
        best = timed(lambda i: call(i, 0), seconds)
        print("%-9s %-7s k=%d V=%5d   the library's choice (*) %9.1f us | torch composition %10.1f us = %6.1fx | results equal" %
              (label, key, k, V, best, tc, tc / best), flush=True)
        del sets, poly, outs
        torch.cuda.empty_cache()
    # the dispatch threshold (kBlockChars of bsq_kmer_spectrum_dev.h): the two forms on rows of one length
    print("# DNA4, k = 4 (V = 256), one strand, 128 Mi characters in rows of L: form 1 (wave per row) against form 2 (workgroup per row)", flush=True)
    tok = Tokenizer("DNA4", False, False, False)
    desc, km = kmers.capi.desc_of(tok), kmers.capi.Kmer(4, 1)
    stream = ctypes.c_void_p(kmers.capi.raw_stream(dev))
    for L, B in [(L, (128 << 20) // L // shrink) for L in (256, 512, 1024, 2048, 4096, 8192, 16384, 65536)] + \
                [(L, B) for L in (1024, 4096, 16384) for B in (64, 512, 4096)]:  # then few rows: the block form has four times the waves
        c, o = batch(7, np.full(B, L, np.int64), DNA)
        nsets = max(2, -(-(600 << 20) // (B * L + B * 1024)) + 1)
        sets = [(torch.from_numpy(c).to(dev), torch.from_numpy(o).to(dev)) for _ in range(nsets)]
        outs = [torch.empty((B, 256), dtype=torch.float32, device=dev) for _ in range(nsets)]

        def call(i, form):
            opt = kmers.capi.KmerSpectrum(0, 0, form, 0, B * L)
            lib.bsq_kmer_spectrum_device(ctypes.byref(desc), sets[i % nsets][0].data_ptr(), sets[i % nsets][1].data_ptr(), B, ctypes.byref(km),
                                         ctypes.byref(opt), 4, outs[i % nsets].data_ptr(), stream)

        call(0, 1), call(1, 2)
        assert torch.equal(outs[0], outs[1])
        tw, tb = timed(lambda i: call(i, 1), seconds), timed(lambda i: call(i, 2), seconds)
        print("L=%6d B=%7d | wave %8.1f us %.3f of roof | block %8.1f us %.3f of roof | wave / block %.2f | the library takes the %s form" %
              (L, B, tw, (B * L + B * 1032) / (tw * 1e-6) / ROOF, tb, (B * L + B * 1032) / (tb * 1e-6) / ROOF, tw / tb,
               "wave" if kmers.kmer_spectrum_kernel_name(tok, 4, B, "f", total_chars=B * L).endswith("wave") else "block"), flush=True)
        del sets, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
