#!/usr/bin/env python3
"""Span-masked k-mer masked-LM batches (bsq_kmer_mlm_tokenize_device) against three yardsticks run in the same process on the same inputs:

(a) `bsq_kmer_tokenize_device` of the same shape and input type, plus a plain write of the label matrix at (a)'s own byte rate (the
    way the packed masked-LM encode was judged): what the two outputs cost without a draw;
(b) the padded `bsq_mlm_tokenize_device` at the same padlen and element types: the hash-cost comparison (4 - 5 selection hashes per
    lane there, up to nine here);
(c) the torch composition over `kmer_tokenize_packed`'s output that yields the same distribution: anchors by `rand`, dilation by
    `max_pool1d`, `where`, `randint`.

DNA4 + PAD, k = 6, span = ceil(k / stride), frac 0.15; 262 144 reads of 512 and 1 048 576 reads of 160 characters (1 % N); stride 1
(padlen = the read length) and stride 6 (the windows rounded up to 16); input / label types int64 / int64, int16 / int64, int16 / int16.
Every result is first compared with the library's CPU twin on the first 4096 rows and with the generic kernel on all of them.  The
calls cycle over distinct batches and outputs of more than 512 MiB together (cold); device events around >= 0.25 s of work per line
after a warm-up, the new call and (a) alternating.  Bytes = characters + offsets + both outputs, against 8 TB/s.

    python scripts/kmer_mlm_lab.py [--quick] [--out FILE]      (default FILE: profiles/r13/kmer_mlm_lab.txt)
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bioseq_amd import Tokenizer, capi, kmers  # noqa: E402

ROOF = 8e12
K, FRAC = 6, 0.15
SIZE = {"h": 2, "q": 8}
NAME = {"h": "int16", "q": "int64"}


def reads(seed, B, L):
    rng = np.random.default_rng(seed)
    chars = rng.choice(np.frombuffer(b"ACGT" * 25 + b"N", np.uint8), B * L).astype(np.uint8)
    return chars, np.arange(B + 1, dtype=np.int64) * L


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


def composition(tok, dch, dof, s, P, dc, ldt, span, p, V, mask_token):
    ids = kmers.kmer_tokenize_packed(tok, dch, dof, K, P, dc, stride=s, validate=False)
    anch = (torch.rand(ids.shape, device=ids.device) < p).float()
    cov = torch.nn.functional.max_pool1d(torch.nn.functional.pad(anch[:, None, :], (span - 1, 0)), span, 1)[:, 0, :] > 0
    sel = cov & (ids < V)
    labels = torch.where(sel, ids.to(ldt), -100)
    r = torch.rand(ids.shape, device=ids.device)
    rnd = torch.randint(0, V, ids.shape, device=ids.device, dtype=ids.dtype)
    inputs = torch.where(sel & (r < 0.8), mask_token, torch.where(sel & (r < 0.9), rnd, ids))
    return inputs, labels


def main():
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r13", "kmer_mlm_lab.txt")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    log = open(out_path, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    seconds = 0.05 if quick else 0.25
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    tok = Tokenizer("DNA4", False, False, True)
    lib, desc = kmers._lib, capi.desc_of(tok)
    V = 4 ** K
    vocab = kmers.kmer_vocab_size(tok, K)
    say("# scripts/kmer_mlm_lab.py: DNA4 + PAD, k = %d, span = ceil(k / stride), frac %.2f; us per call (device events, cold: distinct "
        "batches and outputs), fraction of 8 TB/s on characters + offsets + both outputs" % (K, FRAC))
    say("# (a) bsq_kmer_tokenize_device + the label matrix written at (a)'s byte rate; (b) padded bsq_mlm_tokenize_device, same padlen and "
        "types; (c) torch composition over kmer_tokenize_packed; ratios = yardstick / this call (> 1: this call is faster)")
    for B, L in ((262144, 512), (1048576, 160)):
        host = reads(100, B, L)
        for s in (1, 6):
            span = -(-K // s)
            p = kmers.span_anchor_prob(FRAC, span)
            P = L if s == 1 else (kmers.kmer_count(K, L, s) + 15) // 16 * 16
            km = capi.Kmer(K, s)
            for dc, ldc in (("q", "q"), ("h", "q"), ("h", "h")):
                dt, tdt = capi.dtype_of(dc)
                ldt, ltdt = capi.dtype_of(ldc)
                in_bytes, lab_bytes = B * P * SIZE[dc], B * P * SIZE[ldc]
                src_bytes = B * L + (B + 1) * 8
                nbytes = src_bytes + in_bytes + lab_bytes
                nsets = max(2, -(-(600 << 20) // (B * L + in_bytes + lab_bytes)) + 1)
                dch, dof = torch.from_numpy(host[0]).to(dev), torch.from_numpy(host[1]).to(dev)
                batches = [(dch if i == 0 else dch.clone(), dof) for i in range(nsets)]
                ins = [torch.empty((B, P), dtype=tdt, device=dev) for _ in range(nsets)]
                labs = [torch.empty((B, P), dtype=ltdt, device=dev) for _ in range(nsets)]
                name = kmers.kmer_mlm_kernel_name(tok, K, B, P, dc, True, stride=s, label_destchar=ldc)
                kw = dict(stride=s, frac=FRAC, seed=7, label_destchar=ldc)
                gi, gl = kmers.kmer_mlm_tokenize_packed(tok, dch, dof, K, P, dc, True, validate=False, **kw)
                xi, xl = kmers.kmer_mlm_tokenize_packed(tok, dch, dof, K, P, dc, False, validate=False, **kw)
                hi, hl = kmers.kmer_mlm_tokenize_host(tok, host[0][:4096 * L], host[1][:4097], K, P, dc, True, **kw)
                ok = (torch.equal(gi, xi.t()) and torch.equal(gl, xl.t()) and gi[:4096].cpu().numpy().tobytes() == hi.tobytes()
                      and gl[:4096].cpu().numpy().tobytes() == hl.tobytes())
                share = float((gl != -100).float().mean()) * P / max(kmers.kmer_count(K, L, s), 1)
                ci, cl = composition(tok, dch, dof, s, P, dc, ltdt, span, p, V, vocab)
                cshare = float((cl != -100).float().mean()) * P / max(kmers.kmer_count(K, L, s), 1)
                del gi, gl, xi, xl, ci, cl
                m = capi.KmerMlm(p, 0.8, 0.1, span, vocab, -100, 7, 0)
                mm = capi.Mlm(FRAC, 0.8, 0.1, 4, -100, 7, 0)
                stream = ctypes.c_void_p(capi.raw_stream(dev))

                def new_call(i):
                    c, o = batches[i % nsets]
                    lib.bsq_kmer_mlm_tokenize_device(ctypes.byref(desc), c.data_ptr(), o.data_ptr(), B, P, 1, ctypes.byref(km), ctypes.byref(m), dt,
                                                     ins[i % nsets].data_ptr(), ldt, labs[i % nsets].data_ptr(), stream)

                def kmer_call(i):
                    c, o = batches[i % nsets]
                    lib.bsq_kmer_tokenize_device(ctypes.byref(desc), c.data_ptr(), o.data_ptr(), B, P, 1, ctypes.byref(km), dt, ins[i % nsets].data_ptr(), stream)

                def mlm_call(i):
                    c, o = batches[i % nsets]
                    lib.bsq_mlm_tokenize_device(ctypes.byref(desc), c.data_ptr(), o.data_ptr(), B, P, 1, ctypes.byref(mm), dt, ins[i % nsets].data_ptr(),
                                                ldt, labs[i % nsets].data_ptr(), stream)

                tn = ta = 0.0
                for _ in range(2):  # alternate the new call and yardstick (a)
                    tn += timed(new_call, seconds) / 2
                    ta += timed(kmer_call, seconds) / 2
                tb = timed(mlm_call, seconds)
                tc = timed(lambda i: composition(tok, *batches[i % nsets], s, P, dc, ltdt, span, p, V, vocab), seconds)
                ta_full = ta * (1.0 + lab_bytes / float(src_bytes + in_bytes))  # + the labels at (a)'s byte rate
                say("B=%7d L=%3d stride %d span %d padlen %3d %s/%s %-18s %8.1f us %.3f of roof | (a) kmer %8.1f us + labels = %8.1f us -> %.2f | "
                    "(b) mlm_tokenize %8.1f us -> %.2f | (c) torch %9.1f us -> %5.1fx | selected %.3f (torch %.3f) | %s" %
                    (B, L, s, span, P, NAME[dc], NAME[ldc], name, tn, nbytes / (tn * 1e-6) / ROOF, ta, ta_full, ta_full / tn, tb, tb / tn, tc, tc / tn,
                     share, cshare, "results equal" if ok else "RESULTS DIFFER"))
                del batches, ins, labs
                torch.cuda.empty_cache()
    log.close()


if __name__ == "__main__":
    main()
