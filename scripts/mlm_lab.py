#!/usr/bin/env python3
"""Masked-LM token batches at the cfg5 shape (262 144 x 512, AMINO20, (B, P)): `masking.mlm_tokenize_packed`'s one launch against the
torch composition a user has without it (tokenize_packed, then torch.rand-based selection / replacement / torch.where for the labels).

Algorithmic bytes = sum(L) + 8 (B + 1) + B P (sizeof(input) + sizeof(label)).  "looped": the mean of back-to-back calls (events);
"cold": the median of single calls after a 1 GiB write has pushed the batch and the outputs out of the caches.

    python scripts/mlm_lab.py [--quick]     (--quick: fewer repetitions, for a run under rocprofv3 --kernel-trace --stats)
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bioseq_amd import Tokenizer, capi, masking, synth  # noqa: E402

ROOF = 8e12  # bytes / s, the MI355X HBM3E peak


def main():
    quick = "--quick" in sys.argv
    loops, colds = (5, 3) if quick else (50, 15)
    dev = torch.device("cuda:0")
    c = synth.CONFIGS["cfg5"]
    chars, offs = synth.synth_packed(c["seed"], c["n"], c["lo"], c["hi"], c["letters"])
    B, P = c["n"], c["padlen"]
    dch, dof = torch.from_numpy(chars).to(dev), torch.from_numpy(offs).to(dev)
    tok = Tokenizer("AMINO20")
    desc = capi.make_desc("AMINO20")
    lib = capi.load()
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    sizes = {"b": 1, "q": 8}
    codes = {"b": capi.I8, "q": capi.U64}
    mtok = tok.alphabet_size()

    def timed(fn, n):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1e3

    def cold(fn, n):
        ts = []
        for _ in range(n):
            flush.fill_(1)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return sorted(ts)[len(ts) // 2]

    results = []
    for ic, lc in (("b", "b"), ("b", "q"), ("q", "q")):
        algo = int(offs[-1]) + 8 * (B + 1) + B * P * (sizes[ic] + sizes[lc])
        inp = torch.empty((B, P), dtype=torch.int8 if ic == "b" else torch.int64, device=dev)
        lab = torch.empty((B, P), dtype=torch.int8 if lc == "b" else torch.int64, device=dev)
        m = capi.Mlm(0.15, 0.8, 0.1, mtok, -100, 1234, 0)
        stream = capi.raw_stream(dev)

        def kernel():
            capi.check(lib.bsq_mlm_tokenize_device(ctypes.byref(desc), dch.data_ptr(), dof.data_ptr(), B, P, 1, ctypes.byref(m), codes[ic],
                                                   inp.data_ptr(), codes[lc], lab.data_ptr(), ctypes.c_void_p(stream)))

        def api():
            masking.mlm_tokenize_packed(tok, dch, dof, P, ic, True, label_dtype=lc, seed=1234, validate=False)

        lens = (dof[1:] - dof[:-1]).view(B, 1)
        pos = torch.arange(P, device=dev).view(1, P)
        tdt = torch.int8 if ic == "b" else torch.int64

        def composition():
            plain = tok.tokenize_packed(dch, dof, P, ic, True, validate=False)
            sel = (torch.rand((B, P), device=dev) < 0.15) & (pos < lens)
            r = torch.rand((B, P), device=dev)
            rnd = torch.randint(0, 20, (B, P), device=dev, dtype=tdt)
            x = torch.where(sel & (r < 0.8), torch.tensor(mtok, dtype=tdt, device=dev), torch.where(sel & (r < 0.9), rnd, plain))
            y = torch.where(sel, plain.to(lab.dtype), torch.tensor(-100, dtype=lab.dtype, device=dev))
            return x, y

        row = {"case": "inputs %s / labels %s" % ({"b": "int8", "q": "int64"}[ic], {"b": "int8", "q": "int64"}[lc]), "algo_bytes": algo}
        for name, fn in (("kernel", kernel), ("mlm_tokenize_packed", api), ("torch_composition", composition)):
            lo_us, co_us = timed(fn, loops), cold(fn, colds)
            row[name] = {"looped_us": round(lo_us, 1), "cold_us": round(co_us, 1),
                         "looped_frac_of_8TBs": round(algo / (lo_us * 1e-6) / ROOF, 3), "cold_frac_of_8TBs": round(algo / (co_us * 1e-6) / ROOF, 3)}
        row["speedup_vs_composition_looped"] = round(row["torch_composition"]["looped_us"] / row["kernel"]["looped_us"], 2)
        results.append(row)
        print(json.dumps(row), flush=True)
        del inp, lab
    # the plain int8 token matrix of the same batch, for scale
    out = torch.empty((B, P), dtype=torch.int8, device=dev)
    dt = ctypes.c_int(capi.I8)

    def plain():
        capi.check(lib.bsq_tokenize_device(ctypes.byref(desc), dch.data_ptr(), dof.data_ptr(), B, P, 1, dt, out.data_ptr(), ctypes.c_void_p(capi.raw_stream(dev))))
    algo = int(offs[-1]) + 8 * (B + 1) + B * P
    lo_us, co_us = timed(plain, loops), cold(plain, colds)
    print(json.dumps({"case": "plain int8 tokens (bsq_tokenize_device)", "algo_bytes": algo, "looped_us": round(lo_us, 1), "cold_us": round(co_us, 1),
                      "looped_frac_of_8TBs": round(algo / (lo_us * 1e-6) / ROOF, 3), "cold_frac_of_8TBs": round(algo / (co_us * 1e-6) / ROOF, 3)}), flush=True)


if __name__ == "__main__":
    main()
