#!/usr/bin/env python3
"""MinHash sketches of packed batches (bsq_minhash_device) and the all-pairs sketch comparison (bsq_sketch_compare_device): both sketch
forms against the roof, against kmer_spectrum_packed on the same batch for scale, against the torch composition a user writes without
the call, and the comparison against the chunked torch broadcast.  Seeded synthetic data (1 % unmapped characters), int32 sketches.

    sketch    1 048 576 DNA4 reads x 150, 262 144 x 512, 4 096 contigs of 2 000 .. 200 000 (k = 21, canonical);
              65 536 protein-like rows of 50 .. 1024 residues (AMINO20, k = 7); S = 128 and 1024.  Form 1 (a wave per row), form 2 (a
              workgroup per row), the form the library picks (*), and kmer_spectrum_packed (f32 counts) at the legal k whose width is
              nearest S.  Bytes = characters + offsets + the (B, S) output, against 8 TB/s.
    compose   DNA4 reads x 150 at k = 12, S = 1024, where the composition exists: kmer_tokenize_packed (int64 ids) -> mix64 in int64
              tensor arithmetic -> bucket, value -> scatter_reduce(amin) into a (B, S) matrix of EMPTY; asserted equal to the call.
    compare   sketch_compare against (a[i0:i1, None, :] == b[None, :, :]) ... .sum(-1) in row chunks of at most 1 GiB of booleans;
              asserted equal.
    forms     the dispatch threshold: DNA4, k = 21, canonical, S = 1024 -- 128 Mi characters in rows of L, then few rows: form 1 against
              form 2 (the grid bsq_kmer_spectrum_dev.h records for the spectrum).

cold: the calls cycle over distinct batches and outputs of more than 512 MiB together.  Device events around >= 0.25 s of work per
figure after a warm-up.  The first rows of every sketch are compared with the numpy twin (tests/minhash_twin.py).

    python scripts/minhash_lab.py sketch|compose|compare|forms [--quick]     (--quick: a sixteenth of the rows and short timings)
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import minhash_twin as twin  # noqa: E402
from bioseq_amd import Tokenizer, capi, kmers, sketch  # noqa: E402

ROOF = 8e12
DNA = np.frombuffer(b"ACGT" * 25 + b"N", np.uint8)
AMINO = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY" * 5 + b"X", np.uint8)
QUICK = "--quick" in sys.argv
SECONDS = 0.05 if QUICK else 0.25
SHRINK = 16 if QUICK else 1
lib = sketch._lib


def batch(seed, lens, pool):
    rng = np.random.default_rng(seed)
    offs = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return rng.choice(pool, int(offs[-1])).astype(np.uint8), offs


def timed(fn, seconds=SECONDS):
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


def lut_of(desc):
    return np.frombuffer(bytes(desc.lut), dtype=np.int8)


def part_sketch(dev):
    rng = np.random.default_rng(1)
    shapes = [
        ("reads 150", "DNA4", 21, True, np.full(1048576 // SHRINK, 150, np.int64), DNA),
        ("reads 512", "DNA4", 21, True, np.full(262144 // SHRINK, 512, np.int64), DNA),
        ("proteins", "AMINO20", 7, False, rng.integers(50, 1025, 65536 // SHRINK).astype(np.int64), AMINO),
        ("contigs", "DNA4", 21, True, rng.integers(2000, 200001, 4096 // SHRINK).astype(np.int64), DNA),
    ]
    print("# sketch: int32, seed 0; us per call (device events, cold), fraction of 8 TB/s on characters + offsets + output", flush=True)
    stream = ctypes.c_void_p(capi.raw_stream(dev))
    for label, key, k, canonical, lens, pool in shapes:
        tok = Tokenizer(key, False, False, False)
        desc = capi.desc_of(tok)
        B = lens.size
        host = [batch(100 + i, lens, pool) for i in range(2)]
        total = int(host[0][1][-1])
        for S in (128, 1024):
            nbytes = total + (B + 1) * 8 + B * S * 4
            nsets = max(2, -(-(600 << 20) // (total + B * S * 4)) + 1)
            sets = [(torch.from_numpy(host[i % 2][0]).to(dev), torch.from_numpy(host[i % 2][1]).to(dev)) for i in range(nsets)]
            outs = [torch.empty((B, S), dtype=torch.int32, device=dev) for _ in range(nsets)]

            def call(i, form):
                c, o = sets[i % nsets]
                m = capi.MinHash(k, S, int(canonical), form, 0, total, 0)
                lib.bsq_minhash_device(ctypes.byref(desc), c.data_ptr(), o.data_ptr(), B, ctypes.byref(m), 2, outs[i % nsets].data_ptr(), stream)

            head = min(B, 256)
            want = twin.sketch(lut_of(desc), desc.nchars, host[0][0], host[0][1][:head + 1], k, S, 2, canonical)
            chosen = sketch.minhash_kernel_name(tok, k, B, S, canonical=canonical, total_chars=total)
            for form in (1, 2):
                got = sketch.minhash_packed(tok, *sets[0], k, S, canonical=canonical, form=form, validate=False)
                assert got[:head].cpu().numpy().tobytes() == want.tobytes(), "the call and the numpy twin differ"
                del got
                name = sketch.minhash_kernel_name(tok, k, B, S, canonical=canonical, form=form)
                t = timed(lambda i: call(i, form))
                print("%-9s %-7s k=%2d %s S=%4d B=%7d mean L %6.0f | %-22s%s %9.1f us %.3f of roof %6.2f G windows/s"
                      % (label, key, k, "canonical" if canonical else "plain    ", S, B, total / B, name, "*" if name == chosen else " ", t,
                         nbytes / (t * 1e-6) / ROOF, max(total - B * (k - 1), 0) / (t * 1e-6) / 1e9), flush=True)
            # for scale: the spectrum of the same batch at the legal k whose width is nearest S
            A = desc.nchars
            ks = min((kk for kk in range(2, 8) if A ** kk <= 1 << 14), key=lambda kk: abs(A ** kk - S))
            V = A ** ks
            spec = [torch.empty((B, V), dtype=torch.float32, device=dev) for _ in range(nsets)]
            km, opt = capi.Kmer(ks, 1), capi.KmerSpectrum(0, 0, 0, 0, total)

            def spectrum(i):
                c, o = sets[i % nsets]
                lib.bsq_kmer_spectrum_device(ctypes.byref(desc), c.data_ptr(), o.data_ptr(), B, ctypes.byref(km), ctypes.byref(opt), 4,
                                             spec[i % nsets].data_ptr(), stream)

            ts = timed(spectrum)
            tb = timed(lambda i: call(i, 0))
            print("%-9s %-7s        the library's choice (*) %9.1f us | kmer_spectrum_packed k=%d V=%5d f32 %9.1f us = %5.2fx the sketch"
                  % (label, key, tb, ks, V, ts, ts / tb), flush=True)
            del sets, outs, spec
            torch.cuda.empty_cache()


def mix64_torch(z):
    """splitmix64's finalizer on int64 tensors: products wrap, the shifts are made logical by masking"""
    def shr(x, n):
        return (x >> n) & ((1 << (64 - n)) - 1)
    z = (z ^ shr(z, 30)) * (0xBF58476D1CE4E5B9 - (1 << 64))  # (the constants as int64)
    z = (z ^ shr(z, 27)) * (0x94D049BB133111EB - (1 << 64))
    return z ^ shr(z, 31)


def composition(padded, dch, dof, k, V, S, maxlen, salt):
    B = dof.numel() - 1
    ids = kmers.kmer_tokenize_packed(padded, dch, dof, k, max(1, maxlen - k + 1), "q", True, validate=False)
    keep = ids < V
    h = mix64_torch(ids ^ salt)
    bucket = (((h >> 32) & 0xFFFFFFFF) * S) >> 32
    value = (h & 0xFFFFFFFF).clamp(max=0xFFFFFFFE)
    idx = (bucket + (torch.arange(B, device=ids.device) * S)[:, None])[keep]
    out = torch.full((B * S,), 0xFFFFFFFF, dtype=torch.int64, device=ids.device)
    out.scatter_reduce_(0, idx, value[keep], "amin")
    return out.view(B, S)


def part_compose(dev):
    k, S = 12, 1024
    tok, padded = Tokenizer("DNA4", False, False, False), Tokenizer("DNA4", False, False, True)
    lens = np.full(1048576 // SHRINK // 4, 150, np.int64)
    B = lens.size
    host = [batch(200 + i, lens, DNA) for i in range(2)]
    total = int(host[0][1][-1])
    nsets = max(2, -(-(600 << 20) // (total + B * S * 8)) + 1)
    sets = [(torch.from_numpy(host[i % 2][0]).to(dev), torch.from_numpy(host[i % 2][1]).to(dev)) for i in range(nsets)]
    salt = twin.salt(0)
    salt = salt - (1 << 64) if salt >= 1 << 63 else salt
    comp = composition(padded, *sets[0], k, 4 ** k, S, 150, salt)
    got = sketch.minhash_packed(tok, *sets[0], k, S, "q", validate=False)
    assert torch.equal(torch.where(got < 0, torch.full_like(got, 0xFFFFFFFF), got), comp), "the call and the torch composition differ"
    del comp, got
    tc = timed(lambda i: composition(padded, *sets[i % nsets], k, 4 ** k, S, 150, salt))
    tk = timed(lambda i: sketch.minhash_packed(tok, *sets[i % nsets], k, S, "q", validate=False))
    print("# compose: DNA4 reads x 150, B = %d, k = 12, plain, S = 1024, int64 elements\nminhash_packed %9.1f us | kmer_tokenize_packed + "
          "int64 mix64 + scatter_reduce(amin) %10.1f us = %6.1fx | results equal" % (B, tk, tc, tc / tk), flush=True)


def part_compare(dev):
    print("# compare: int32 sketches of random DNA4 rows of 600 characters, k = 21, canonical; match and either", flush=True)
    tok = Tokenizer("DNA4", False, False, False)
    for Ba, Bb, S, with_torch in ((1024, 1024, 1024, True), (4096, 4096, 128, True), (8192, 8192, 1024, False), (65536 // SHRINK, 1024, 1024, False)):
        c, o = batch(300 + S, np.full(max(Ba, Bb), 600, np.int64), DNA)
        c[:600 * 16] = c[600 * 16:600 * 32]  # (sixteen duplicated rows: not every pair scores 0)
        sk = sketch.minhash_packed(tok, torch.from_numpy(c).to(dev), torch.from_numpy(o).to(dev), 21, S, canonical=True)
        a, b = sk[:Ba].contiguous(), sk[:Bb].contiguous()
        t = timed(lambda i: sketch.sketch_compare(a, b))
        line = "Ba=%6d Bb=%5d S=%5d | k_sketch_compare %9.1f us  %7.1f G bucket pairs/s" % (Ba, Bb, S, t, Ba * Bb * S / (t * 1e-6) / 1e9)
        if with_torch:
            rows = max(1, (1 << 30) // (Bb * S))

            def broadcast(_):
                ms, es = [], []
                for i0 in range(0, Ba, rows):
                    x = a[i0:i0 + rows, None, :]
                    ms.append(((x == b[None]) & (x != -1)).sum(-1, dtype=torch.int32))
                    es.append(((x != -1) | (b[None] != -1)).sum(-1, dtype=torch.int32))
                return torch.cat(ms), torch.cat(es)

            m, e = sketch.sketch_compare(a, b)
            tm, te = broadcast(0)
            assert torch.equal(m, tm) and torch.equal(e, te) and int(m[0, 16]) > 0, "the call and the torch broadcast differ"
            del m, e, tm, te
            tt = timed(broadcast)
            line += " | torch broadcast in chunks of %d rows %10.1f us = %6.1fx | results equal" % (rows, tt, tt / t)
        print(line, flush=True)
        del sk, a, b
        torch.cuda.empty_cache()


def part_forms(dev):
    print("# forms: DNA4, k = 21, canonical, S = 1024, int32: form 1 (wave per row) against form 2 (workgroup per row)", flush=True)
    tok = Tokenizer("DNA4", False, False, False)
    desc = capi.desc_of(tok)
    stream = ctypes.c_void_p(capi.raw_stream(dev))
    S = 1024
    for L, B in [(L, (128 << 20) // L // SHRINK) for L in (256, 512, 1024, 2048, 4096, 8192, 16384, 65536)] + \
                [(L, B) for L in (1024, 4096, 16384) for B in (64, 512, 4096)]:  # then few rows: the block form has four times the waves
        c, o = batch(7, np.full(B, L, np.int64), DNA)
        nsets = max(2, -(-(600 << 20) // (B * L + B * S * 4)) + 1)
        sets = [(torch.from_numpy(c).to(dev), torch.from_numpy(o).to(dev)) for _ in range(nsets)]
        outs = [torch.empty((B, S), dtype=torch.int32, device=dev) for _ in range(nsets)]

        def call(i, form):
            m = capi.MinHash(21, S, 1, form, 0, B * L, 0)
            lib.bsq_minhash_device(ctypes.byref(desc), sets[i % nsets][0].data_ptr(), sets[i % nsets][1].data_ptr(), B, ctypes.byref(m), 2,
                                   outs[i % nsets].data_ptr(), stream)

        call(0, 1), call(1, 2)
        assert torch.equal(outs[0], outs[1])
        tw, tb = timed(lambda i: call(i, 1)), timed(lambda i: call(i, 2))
        nbytes = B * L + B * (8 + S * 4)
        print("L=%6d B=%7d | wave %8.1f us %.3f of roof | block %8.1f us %.3f of roof | wave / block %.2f | the library takes the %s form" %
              (L, B, tw, nbytes / (tw * 1e-6) / ROOF, tb, nbytes / (tb * 1e-6) / ROOF, tw / tb,
               "wave" if sketch.minhash_kernel_name(tok, 21, B, S, canonical=True, total_chars=B * L).endswith("wave") else "block"), flush=True)
        del sets, outs
        torch.cuda.empty_cache()


def main():
    parts = {"sketch": part_sketch, "compose": part_compose, "compare": part_compare, "forms": part_forms}
    chosen = [a for a in sys.argv[1:] if a in parts]
    if not chosen:
        sys.exit(__doc__)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    for name in chosen:
        parts[name](dev)


if __name__ == "__main__":
    main()
