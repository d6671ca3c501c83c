#!/usr/bin/env python3
"""BPE training on the device (`bpe.bpe_train_packed`, bsq_bpe_train_*_device) as whole calls, at the shapes the BPE labs use:

    reads     1 048 576 reads of 150 DNA4 characters, 4096 merges                   max_chars 1024: k_bpe_train_pass<wave>
    dna512    262 144 rows of 512 DNA4 characters, 4096 merges                      max_chars 1024: k_bpe_train_pass<wave>
    protein   65 536 AMINO20 rows of 50 .. 1024 residues, 8000 merges               max_chars 1024: k_bpe_train_pass<wave>
    long      4 096 rows of 8192 DNA4 characters, 4096 merges                       max_chars 8192: k_bpe_train_pass<block>

Rows of uniform letters, seeded.  Per shape:
  * the whole call (workspace allocation, begin, every step, the 8-byte read-backs, the head's read-back), wall clock around a
    synchronised call, the calls alternating between two stores of the same row lengths: the median of the rounds and their spread;
  * one run through the C ABI with device events behind step 64 and in front of the last 64 steps: the time per merge over the first 64
    and the last 64 merges (the corpus shrinks, the pair table grows), and the live symbols at the end, read from the workspace;
  * the bytes a pass moves at least -- 2 per live symbol, 12 per row -- against 8 TB/s;
  * the library's CPU twin on one thread on the same store at n_merges = 64, by time per merge, its merges asserted equal to the
    device's first 64;
  * numpy `bpe_train_host` on a 1/64 sample at 16 merges (a sort of the sample per merge), its merges asserted equal to the device's and
    the twin's on that sample;
  * where the `tokenizers` package is importable, its BpeTrainer on the 1/64 sample for information (its tie rule differs: no equality).
The pass / pick split is not taken here (events cannot separate interleaved launches): it comes from a kernel-trace run of this script.

    python scripts/bpe_train_lab.py reads|dna512|protein|long [--quick] [--once] [--out FILE]
    (--quick: an eighth of the rows, a quarter of the merges; --once: one whole call and nothing else, for a kernel trace)
"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bioseq_amd import Tokenizer, bpe, capi  # noqa: E402

QUICK = "--quick" in sys.argv
ONCE = "--once" in sys.argv
ROUNDS = 2
lib = bpe._lib
AMINO = "ACDEFGHIKLMNPQRSTVWY"
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r30", "bpe_train_lab.txt")


def emit(line):
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as fh:
        fh.write(line + "\n")


def store(rng, lengths, letters):
    """(chars, offsets) of random rows of these lengths"""
    offs = np.zeros(lengths.size + 1, np.int64)
    np.cumsum(lengths, out=offs[1:])
    return np.frombuffer(letters.encode(), np.uint8)[rng.integers(0, len(letters), int(offs[-1]), dtype=np.uint8)], offs


def whole_call(tok, dset, n_merges, max_chars):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v, info = bpe.bpe_train_packed(tok, dset[0], dset[1], n_merges, max_chars=max_chars, return_info=True)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, v, info


def staged_run(tok, dset, n_merges, max_chars, dev):
    """One run through the C ABI, no read-back before its end: (ms of the first 64 steps, ms of the last 64, ms in all, records, live
    symbols at the end)."""
    desc = capi.desc_of(tok)
    chars, offs = dset
    B, total = offs.numel() - 1, chars.numel()
    cfg = capi.BpeTrain(max_chars, 0, n_merges, 0, 0)
    work = torch.empty((lib.bsq_bpe_train_workspace_bytes(ctypes.byref(desc), B, total, ctypes.byref(cfg)) + 7) // 8, dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(capi.raw_stream(dev))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    capi.check(lib.bsq_bpe_train_begin_device(ctypes.byref(desc), chars.data_ptr(), offs.data_ptr(), B, total, ctypes.byref(cfg), work.data_ptr(), stream))
    cuts = [0, 64, n_merges - 64, n_merges]
    ev[0].record()
    for k in range(3):
        capi.check(lib.bsq_bpe_train_steps_device(ctypes.byref(desc), offs.data_ptr(), B, total, ctypes.byref(cfg), work.data_ptr(), cuts[k],
                                                  cuts[k + 1] - cuts[k], stream))
        ev[k + 1].record()
    torch.cuda.synchronize()
    head = work[:2 + n_merges].cpu().numpy()
    assert head[1] == 0, "the pair table overflowed"
    lens = work[2 + n_merges:2 + n_merges + (B + 1) // 2].cpu().numpy().view(np.int32)[:B]
    return ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3]), ev[0].elapsed_time(ev[3]), head[2:].view(np.uint64), int(lens.sum())


def hf_train(texts, n_merges, letters):
    try:
        import tokenizers
    except ImportError:
        return None
    os.environ.setdefault("RAYON_NUM_THREADS", "16")
    tk = tokenizers.Tokenizer(tokenizers.models.BPE(unk_token="<UNK>"))
    trainer = tokenizers.trainers.BpeTrainer(vocab_size=len(letters) + 1 + n_merges, special_tokens=["<UNK>"], initial_alphabet=list(letters),
                                             show_progress=False)
    t0 = time.perf_counter()
    tk.train_from_iterator(texts, trainer)
    return time.perf_counter() - t0


def part(dev, name, key, letters, n_rows, lo, hi, n_merges, max_chars):
    tok = Tokenizer(key, False, False, False)
    n, n_merges = n_rows // (8 if QUICK else 1), n_merges // (4 if QUICK else 1)
    sets = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        sets.append(store(rng, rng.integers(lo, hi + 1, n), letters))
    dsets = [[torch.from_numpy(x).to(dev) for x in s] for s in sets]
    total = int(sets[0][1][-1])
    whole_call(tok, dsets[1], 64, max_chars)  # warm-up: the runtime's first launches, the allocator's first blocks
    if ONCE:
        sec, v, info = whole_call(tok, dsets[0], n_merges, max_chars)
        emit("%-8s --once: %d merges in %.3f s" % (name, v.M, sec))
        return
    times, vocabs = [], []
    for r in range(2 * ROUNDS):
        sec, v, info = whole_call(tok, dsets[r & 1], n_merges, max_chars)
        times.append(sec)
        vocabs.append(v)
    assert all(np.array_equal(vocabs[r].merges, vocabs[r & 1].merges) for r in range(2 * ROUNDS)), "a call differs from itself"
    v, med = vocabs[0], float(np.median(times))
    first, last, all_ms, records, live_end = staged_run(tok, dsets[0], n_merges, max_chars, dev)
    staged_m, _ = bpe._decode_records(records)
    assert np.array_equal(staged_m, v.merges), "the staged run and the whole call differ"
    pass_bytes = lambda live: 2 * live + 12 * n
    emit("%-8s %s %d rows, %.1f M characters, %d merges asked, %d made, %s, table %d slots | whole call: median of %d %.3f s (min %.3f, max %.3f; "
         "%.3f ms per merge) | events, no read-backs: %.3f s; first 64 merges %.3f ms each, last 64 %.3f ms each | live symbols at the end %.1f M "
         "(%.2f of the start) | a pass moves at least %.0f MB at the start, %.0f MB at the end: %.3f / %.3f ms at 8 TB/s"
         % (name, key, n, total / 1e6, n_merges, v.M, info["kernel"], info["table_slots"], len(times), med, min(times), max(times), med / max(v.M, 1) * 1e3,
            all_ms / 1e3, first / 64, last / 64, live_end / 1e6, live_end / max(total, 1), pass_bytes(total) / 1e6, pass_bytes(live_end) / 1e6,
            pass_bytes(total) / 8e12 * 1e3, pass_bytes(live_end) / 8e12 * 1e3))
    # the CPU twin, one thread, the same store, 64 merges
    t0 = time.perf_counter()
    tw = bpe.bpe_train_packed(tok, sets[0][0], sets[0][1], 64, max_chars=max_chars)
    t_twin = time.perf_counter() - t0
    assert np.array_equal(tw.merges, v.merges[:tw.M]) and tw.M == min(64, v.M), "the twin and the device differ"
    emit("%-8s CPU twin, one thread, the same store, 64 merges: %.2f s, %.1f ms per merge | device first 64: %.3f ms per merge: %.0f x | "
         "device whole call per merge: %.0f x" % (name, t_twin, t_twin / 64 * 1e3, first / 64, t_twin / 64 * 1e3 / (first / 64),
                                                   t_twin / 64 / (med / max(v.M, 1))))
    # numpy on a 1/64 sample, 16 merges
    pick = np.arange(0, n, 64)
    rows = [sets[0][0][sets[0][1][k]:sets[0][1][k + 1]] for k in pick]
    sch = np.concatenate(rows)
    sof = np.zeros(pick.size + 1, np.int64)
    np.cumsum([r.size for r in rows], out=sof[1:])
    t0 = time.perf_counter()
    ref = bpe.bpe_train_host(tok, sch, sof, 16)
    t_np = time.perf_counter() - t0
    t0 = time.perf_counter()
    tws = bpe.bpe_train_packed(tok, sch, sof, 16, max_chars=max_chars)
    t_tws = time.perf_counter() - t0
    dsample = [torch.from_numpy(sch).to(dev), torch.from_numpy(sof).to(dev)]
    whole_call(tok, dsample, 16, max_chars)
    t_dev, vs, _ = whole_call(tok, dsample, 16, max_chars)
    assert np.array_equal(ref.merges, vs.merges) and np.array_equal(ref.merges, tws.merges), "numpy, the twin and the device differ on the sample"
    line = ("%-8s 1/64 sample (%d rows, %.2f M characters), 16 merges: numpy bpe_train_host %.2f s (%.1f ms per merge), twin %.3f s, device whole call "
            "%.4f s; merges equal" % (name, pick.size, sch.size / 1e6, t_np, t_np / 16 * 1e3, t_tws, t_dev))
    t_hf = hf_train([bytes(r).decode() for r in rows], min(n_merges, 1024), letters)
    line += " | tokenizers: not importable" if t_hf is None else " | tokenizers BpeTrainer, the sample, %d merges: %.2f s (its own tie rule)" % (min(n_merges, 1024), t_hf)
    emit(line)


def main():
    parts = {"reads": ("DNA4", "ACGT", 1048576, 150, 150, 4096, 1024),
             "dna512": ("DNA4", "ACGT", 262144, 512, 512, 4096, 1024),
             "protein": ("AMINO20", AMINO, 65536, 50, 1024, 8000, 1024),
             "long": ("DNA4", "ACGT", 4096, 8192, 8192, 4096, 8192)}
    chosen = [a for a in sys.argv[1:] if a in parts]
    if not chosen:
        sys.exit(__doc__)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    for name in chosen:
        part(dev, name, *parts[name])


if __name__ == "__main__":
    main()
