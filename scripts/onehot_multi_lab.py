"""n one-hot batches as ONE bsq_onehot_device_multi call against n single calls (bsq_onehot_device / bsq_onehot_bcl_device) back to back on
one stream, timed with HIP events: looped (the same buffers every iteration) and cold (cycling over > 512 MiB of distinct inputs and outputs),
each repeated --reps times in the same process -- the spread of the repeats is the yardstick.  Prints us per batch and the fraction of
8 TB/s on output bytes.  Usage: python scripts/onehot_multi_lab.py [--iters 50] [--reps 3]"""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bioseq_amd import capi, synth  # noqa: E402

SHAPES = [  # (label, key, (eos, bos, pad), B, P, dtype, layout, n)
    ("1024x256 DNA f32", "DNA", (0, 0, 0), 1024, 256, "F32", 0, 8),
    ("4096x512 AMINO20 f32", "AMINO20", (0, 0, 0), 4096, 512, "F32", 0, 4),
    ("8192x1024 AMINO20 f32 (cfg3 shard)", "AMINO20", (0, 0, 0), 8192, 1024, "F32", 0, 4),
    ("131072x160 DNA4+BEP f32 (cfg4f shard)", "DNA4", (1, 1, 1), 131072, 160, "F32", 0, 4),
    ("262144x160 DNA4+BEP int8 (rows1<nibbles>)", "DNA4", (1, 1, 1), 262144, 160, "I8", 0, 4),
    ("4096x512 SEB8 f32 (B,C,P) cnn batch", "SEB8", (0, 0, 0), 4096, 512, "F32", 1, 4),
]


def make_set(key, B, P, n, seed, dev):
    alpha = "ACGT" if key.startswith("DNA") else synth.AA
    out = []
    for i in range(n):
        lens = synth.synth_lengths(seed + i, B, P // 2, P - 2)
        offs = np.zeros(B + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        rng = np.random.default_rng(seed + i)
        letters = np.frombuffer(alpha.encode(), np.uint8)
        chars = letters[rng.integers(0, letters.size, int(offs[-1]))]
        out.append((torch.from_numpy(chars).to(dev), torch.from_numpy(offs).to(dev)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    lib = capi.load()
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(s.cuda_stream)
    print("shape | family | n | mode | multi us/batch (reps) | single us/batch (reps) | multi frac | single frac")
    for label, key, fl, B, P, code, layout, n in SHAPES:
        desc = capi.make_desc(key, *map(bool, fl))
        C = lib.bsq_alphabet_size(ctypes.byref(desc))
        t = getattr(capi, code)
        sz = int(lib.bsq_dtype_size(t))
        out_bytes = B * C * P * sz
        nsets = max(1, -(-(512 << 20) // (n * out_bytes)) + 1)
        sets = []
        for k in range(nsets):
            inp = make_set(key, B, P, n, 1000 * k, dev)
            outs = [torch.empty(out_bytes, dtype=torch.uint8, device=dev) for _ in range(n)]
            arr = (capi.OnehotBatch * n)()
            for i, ((c, o), y) in enumerate(zip(inp, outs)):
                arr[i].chars, arr[i].offsets, arr[i].mask, arr[i].B, arr[i].out = c.data_ptr(), o.data_ptr(), None, B, y.data_ptr()
            sets.append((inp, outs, arr))
        fam = (ctypes.c_int32 * n)()
        lib.bsq_onehot_multi_plan(ctypes.byref(desc), n, sets[0][2], P, layout, t, fam)
        single = lib.bsq_onehot_device if layout == 0 else lib.bsq_onehot_bcl_device

        def run(k, multi):
            arr = sets[k % nsets][2]
            if multi:
                capi.check(lib.bsq_onehot_device_multi(ctypes.byref(desc), n, arr, P, layout, t, sp))
            else:
                for i in range(n):
                    capi.check(single(ctypes.byref(desc), arr[i].chars, arr[i].offsets, None, B, P, t, arr[i].out, sp))

        for mode in ("loop", "cold"):
            res = {True: [], False: []}
            for _ in range(a.reps):
                for multi in (True, False):
                    for k in range(3):
                        run(k, multi)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for k in range(a.iters):
                        run(k if mode == "cold" else 0, multi)
                    e1.record(s)
                    e1.synchronize()
                    res[multi].append(e0.elapsed_time(e1) * 1e3 / a.iters / n)
            m, sg = np.median(res[True]), np.median(res[False])
            print("%s | %s | %d | %s | %.1f (%s) | %.1f (%s) | %.3f | %.3f" % (
                label, ",".join(str(f) for f in sorted(set(fam))), n, mode, m, " ".join("%.1f" % x for x in res[True]), sg,
                " ".join("%.1f" % x for x in res[False]), out_bytes / (m * 1e-6) / 8e12, out_bytes / (sg * 1e-6) / 8e12), flush=True)
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
