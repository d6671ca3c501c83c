#!/usr/bin/env python3
"""k-mer ids of packed batches (bsq_kmer_tokenize_device) against two yardsticks taken in the same run, alternating with the new call:

(1) `tok.tokenize_packed` of the same batch, padlen and element type -- existing code moving the same output bytes;
(2) the torch composition a user writes without the call: single-residue tokens (DNA5, so that N is visible) -> unfold -> weighted
    sum -> where for UNK -> where for the positions behind a row's last window, cast to the element type.

Seeded synthetic DNA reads (1 % N), plain DNA4 tokenizer with PAD; k = 6, stride 1 and 6; int16 and int64; 262 144 reads of 512 and
1 048 576 reads of 160 characters.  padlen = the read length for stride 1 and the windows rounded up to 16 for stride 6 (the token
yardstick then clamps its rows to that padlen: it reads fewer characters and writes the same bytes).  Every result is first compared
with the numpy twin (tests/kmer_twin.py) through a 64-bit fold at the timed size, and the composition with the call's result.
cold: the calls cycle over distinct batches and outputs of more than 512 MiB together; looped: one batch, one output.  Device events
around >= 0.5 s of work per line after a warm-up.  Bytes = characters + offsets + output, against 8 TB/s.

    python scripts/kmer_lab.py [--quick]     (--quick: short timings and no twin, for a run under rocprofv3 --kernel-trace --stats)
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kmer_twin as twin  # noqa: E402
from bioseq_amd import Tokenizer, kmers  # noqa: E402

ROOF = 8e12
K = 6
SIZE = {"h": 2, "q": 8}


def reads(seed, B, L):
    rng = np.random.default_rng(seed)
    chars = rng.choice(np.frombuffer(b"ACGT" * 25 + b"N", np.uint8), B * L).astype(np.uint8)
    offs = np.arange(B + 1, dtype=np.int64) * L
    return chars, offs


def fold(a, first):
    idx = np.arange(first, first + a.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int((a.reshape(-1).astype(np.int64).astype(np.uint64) * (idx * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1))).sum(dtype=np.uint64))


def twin_fold(lut, chars, offs, s, P, step=16384):
    B, total = len(offs) - 1, 0
    for b0 in range(0, B, step):
        o = offs[b0:b0 + step + 1]
        total += fold(twin.rows_fast(lut, 4, chars[o[0]:o[-1]], o - o[0], K, s, P, 0, 0, 1), b0 * P)
    return total & (2 ** 64 - 1)


def device_fold(t, step=16384):
    P, total = t.shape[1], 0
    for b0 in range(0, t.shape[0], step):
        total += fold(t[b0:b0 + step].cpu().numpy(), b0 * P)
    return total & (2 ** 64 - 1)


def composition(tok5, dch, dof, L, s, P, tdt, pad_id, unk_id):
    t = tok5.tokenize_packed(dch, dof, L, "q", True, validate=False)
    w = t.unfold(1, K, s)
    weights = 4 ** torch.arange(K - 1, -1, -1, device=t.device)
    ids = (w * weights).sum(-1)
    ids = torch.where((w == 4).any(-1), unk_id, ids)
    lens = dof[1:] - dof[:-1]
    n = torch.where(lens < K, 0, torch.div(lens - K, s, rounding_mode="floor") + 1)
    ids = torch.where(torch.arange(ids.shape[1], device=t.device)[None, :] < n[:, None], ids, pad_id)
    out = torch.full((ids.shape[0], P), pad_id, dtype=tdt, device=t.device)
    out[:, :ids.shape[1]] = ids[:, :P]
    return out


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


def main():
    quick = "--quick" in sys.argv
    seconds = 0.05 if quick else 0.25  # per block; two blocks per timing, alternating
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    tok, tok5 = Tokenizer("DNA4", False, False, True), Tokenizer("DNA5", False, False, True)
    lut = np.frombuffer(bytes(kmers.capi.desc_of(tok).lut), dtype=np.int8)
    sp = kmers.kmer_special_ids(tok, K)
    print("# scripts/kmer_lab.py: DNA4 + PAD, k = %d; us per call (device events), fraction of 8 TB/s on characters + offsets + output" % K)
    for B, L in ((262144, 512), (1048576, 160)):
        host = [reads(100 + i, B, L) for i in range(1 if quick else 2)]
        for s in (1, 6):
            P = L if s == 1 else (kmers.kmer_count(K, L, s) + 15) // 16 * 16
            want = None if quick else twin_fold(lut, host[0][0], host[0][1], s, P)
            for dc in ("h", "q"):
                tdt = torch.int16 if dc == "h" else torch.int64
                out_bytes = B * P * SIZE[dc]
                nbytes = B * L + (B + 1) * 8 + out_bytes
                nsets = max(2, -(-(600 << 20) // (B * L + out_bytes)) + 1)
                batches = []
                for i in range(nsets):
                    c, o = host[i % len(host)]
                    batches.append((torch.from_numpy(c).to(dev), torch.from_numpy(o).to(dev)))
                outs = [torch.empty((B, P), dtype=tdt, device=dev) for _ in range(nsets)]
                name = kmers.kmer_kernel_name(tok, K, B, P, dc, True, stride=s)
                got = kmers.kmer_tokenize_packed(tok, *batches[0], K, P, dc, stride=s, validate=False)
                gen = kmers.kmer_tokenize_packed(tok, *batches[0], K, P, dc, False, stride=s, validate=False)
                comp = composition(tok5, *batches[0], L, s, P, tdt, sp["pad"], sp["unk"])
                ok = torch.equal(got, comp) and torch.equal(got, gen.t())
                if want is not None:
                    ok = ok and device_fold(got) == want
                del got, gen, comp
                lib, desc, km = kmers._lib, kmers.capi.desc_of(tok), kmers.capi.Kmer(K, s)
                dt = kmers.capi.dtype_of(dc)[0]
                stream = ctypes.c_void_p(kmers.capi.raw_stream(dev))

                def kmer_call(i, sets=nsets, bf=1):
                    c, o = batches[i % sets]
                    lib.bsq_kmer_tokenize_device(ctypes.byref(desc), c.data_ptr(), o.data_ptr(), B, P, bf, ctypes.byref(km), dt,
                                                 outs[i % sets].data_ptr(), stream)

                def tok_call(i, sets=nsets):
                    c, o = batches[i % sets]
                    lib.bsq_tokenize_device(ctypes.byref(desc), c.data_ptr(), o.data_ptr(), B, P, 1, dt, outs[i % sets].data_ptr(), stream)

                for mode, sets in (("cold", nsets), ("looped", 1)):
                    tk = tt = 0.0
                    for _ in range(2):  # alternate the new call and the yardstick
                        tk += timed(lambda i: kmer_call(i, sets), seconds) / 2
                        tt += timed(lambda i: tok_call(i, sets), seconds) / 2
                    tg = timed(lambda i: kmer_call(i, sets, 0), seconds)
                    tc = timed(lambda i: composition(tok5, *batches[i % sets], L, s, P, tdt, sp["pad"], sp["unk"]), seconds)
                    print("B=%7d L=%3d stride %d padlen %3d %s %-6s %-14s %8.1f us %.3f of roof | tokenize_packed %8.1f us %.3f -> ratio %.2f | "
                          "k_kmer_generic (P,B) %8.1f us | torch composition %9.1f us = %5.1fx | %s" %
                          (B, L, s, P, "int16" if dc == "h" else "int64", mode, name, tk, nbytes / (tk * 1e-6) / ROOF, tt,
                           (min(P, L) * B + (B + 1) * 8 + out_bytes) / (tt * 1e-6) / ROOF, tk / tt, tg, tc, tc / tk,
                           "results equal" if ok else "RESULTS DIFFER"), flush=True)
                del batches, outs
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
