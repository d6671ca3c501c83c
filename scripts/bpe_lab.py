#!/usr/bin/env python3
"""BPE ids of packed batches (bsq_bpe_tokenize_device) as whole calls: rows and characters per second at the shapes the two forms are
for, the steps a row takes, and two CPU yardsticks on a sample of the same rows -- the library's host twin on one thread and, where
the `tokenizers` package is importable, Hugging Face's `encode_batch` on 16 threads (strings prepared outside the timing).

    dna512    262 144 rows of 512 DNA4 characters, 4096 merges                      max_chars 1024: k_bpe_wave
    reads     1 048 576 reads of 150 DNA4 characters, 4096 merges                   max_chars 1024: k_bpe_wave
    protein   65 536 AMINO20 rows of 50 .. 1024 residues, 8000 merges               max_chars 1024: k_bpe_wave
    long      4 096 rows of 8192 DNA4 characters, 4096 merges                       max_chars 8192: k_bpe_block
    each followed by the poly-A batch of its shape (every candidate mask one run: the worst case of the selection)

The merges are trained by `bpe_train_host` on a seeded sample of the same distribution (rows of the part's lengths, uniform letters).
Steps: the distinct ranks a row applies (one step of the kernels each), counted by a plain Python programme on a few rows.
Timing: device events around >= 0.25 s of work (at least 4 calls) after a warm-up, the calls alternating between two sets of inputs and
outputs, so a call finds none of its inputs in cache from the call before at the larger shapes; nothing here was timed with a
profiler attached.  Before timing, the device's tokens and lengths of the sample are asserted equal to the host twin's.

    python scripts/bpe_lab.py dna512|reads|protein|long [--quick]     (--quick: an eighth of the rows, a quarter of the merges)
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
SECONDS = 0.05 if QUICK else 0.25
SHRINK = 8 if QUICK else 1
lib = bpe._lib
AMINO = "ACDEFGHIKLMNPQRSTVWY"


def store(rng, lengths, letters):
    """(chars, offsets) of random rows of these lengths"""
    offs = np.zeros(lengths.size + 1, np.int64)
    np.cumsum(lengths, out=offs[1:])
    return np.frombuffer(letters.encode(), np.uint8)[rng.integers(0, len(letters), int(offs[-1]), dtype=np.uint8)], offs


def timed(fn, seconds=SECONDS, least=4):
    fn(0), fn(1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(2):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    reps = max(least, int(seconds / max(a.elapsed_time(b) / 2e3, 1e-6)))
    reps += reps & 1
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us


def steps_of(lut, C, merges, row):
    """The steps the kernels take on one row: each applies the lowest rank present to all its occurrences, left to right."""
    V = C + len(merges)
    rank = {(int(l), int(r)): m for m, (l, r) in enumerate(merges)}
    sym = [int(lut[b]) if lut[b] >= 0 else V for b in bytes(row)]
    steps = 0
    while True:
        ranks = [rank.get(p, V) for p in zip(sym, sym[1:])]
        m = min(ranks, default=V)
        if m == V:
            return steps
        out, i = [], 0
        while i < len(sym):
            if i < len(ranks) and ranks[i] == m:
                out.append(C + m)
                i += 2
            else:
                out.append(sym[i])
                i += 1
        sym, steps = out, steps + 1


def measure(dev, name, vocab, sets, max_chars, n_steps, hf):
    """sets: two (chars, offsets) of numpy arrays with the same row lengths"""
    tok, desc = vocab.tok, vocab.desc
    B = sets[0][1].size - 1
    lens = np.diff(sets[0][1])
    P = int(lens.max())  # (room for every row even where no merge fires)
    cfg = capi.Bpe(max_chars, 0, 0)
    table = vocab.device_table(dev)
    dsets = [[torch.from_numpy(x).to(dev) for x in s] + [torch.empty((B, P), dtype=torch.int16, device=dev), torch.empty(B, dtype=torch.int32, device=dev)]
             for s in sets]
    stream = ctypes.c_void_p(capi.raw_stream(dev))

    def call(i):
        ch, of, tokens, lengths = dsets[i & 1]
        capi.check(lib.bsq_bpe_tokenize_device(ctypes.byref(desc), ch.data_ptr(), of.data_ptr(), B, P, 1, table.data_ptr(), vocab.M, ctypes.byref(cfg),
                                               capi.I16, tokens.data_ptr(), lengths.data_ptr(), stream))

    pick = np.arange(0, B, 64)
    rows = [sets[0][0][sets[0][1][k]:sets[0][1][k + 1]] for k in pick]
    sch = np.concatenate(rows)
    sof = np.zeros(pick.size + 1, np.int64)
    np.cumsum([r.size for r in rows], out=sof[1:])
    t0 = time.perf_counter()
    host_t, host_l = bpe.bpe_tokenize_host(vocab, sch, sof, P, "h", max_chars=max_chars)
    th = time.perf_counter() - t0
    call(0)
    torch.cuda.synchronize()
    assert np.array_equal(dsets[0][2].cpu().numpy()[::64], host_t) and np.array_equal(dsets[0][3].cpu().numpy()[::64], host_l) and (host_l >= 0).all(), \
        "the device and the host twin differ"
    lut = np.array(list(desc.lut), np.int64)
    steps = [steps_of(lut, desc.nchars, vocab.merges, r) for r in rows[:n_steps]]
    us = timed(call)
    chars = int(lens.sum())
    line = ("%-14s %s M %4d max_chars %4d %-11s | %8d rows, %7.1f M chars, %5.2f chars per token | %10.1f us per call, %7.2f M rows/s, %7.2f G chars/s | "
            "steps per row (%d rows): mean %.1f, max %d | host twin, one thread, %d rows: %.3f s, %.4f M rows/s: device %.0f x"
            % (name, tok.key, vocab.M, max_chars, bpe.bpe_kernel_name(max_chars=max_chars), B, chars / 1e6, chars / max(int(host_l.sum()) * 64, 1), us, B / us,
               chars / us / 1e3, len(steps), float(np.mean(steps)), max(steps), pick.size, th, pick.size / th / 1e6, (th / pick.size * B) / (us / 1e6)))
    if hf is not None:
        texts = [bytes(r).decode() for r in rows]
        hf.encode_batch(texts[:16])
        t0 = time.perf_counter()
        enc = hf.encode_batch(texts)
        tf = time.perf_counter() - t0
        same = all(bpe.bpe_decode(vocab, host_t[k, :host_l[k]]) == enc[k].tokens for k in range(0, len(texts), 16))
        line += " | tokenizers encode_batch, 16 threads, %d rows: %.3f s, %.4f M rows/s: device %.0f x, strings %s" % (
            len(texts), tf, len(texts) / tf / 1e6, (tf / len(texts) * B) / (us / 1e6), "equal" if same else "DIFFER")
    else:
        line += " | tokenizers: not importable or the table spells a string twice"
    print(line, flush=True)


def hf_of(vocab):
    try:
        import tokenizers
    except ImportError:
        return None
    strings = bpe.bpe_strings(vocab)
    if len(set(strings)) != len(strings):
        return None
    os.environ.setdefault("RAYON_NUM_THREADS", "16")
    os.environ.setdefault("TOKENIZERS_PARALLELISM", "true")
    return tokenizers.Tokenizer(tokenizers.models.BPE(vocab={s: i for i, s in enumerate(strings)},
                                                      merges=[(strings[l], strings[r]) for l, r in vocab.merges.tolist()], unk_token="<UNK>"))


def part(dev, name, key, letters, n_rows, lo, hi, n_merges, max_chars, sample_rows, n_steps):
    tok = Tokenizer(key, False, False, False)
    n = n_rows // SHRINK
    rng = np.random.default_rng(len(name))
    t0 = time.perf_counter()
    vocab = bpe.bpe_train_host(tok, *store(rng, rng.integers(lo, hi + 1, sample_rows), letters), n_merges // (4 if QUICK else 1))
    print("# %s: %d merges trained on %d rows in %.1f s" % (name, vocab.M, sample_rows, time.perf_counter() - t0), flush=True)
    hf = hf_of(vocab)
    sets, poly = [], []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        lengths = rng.integers(lo, hi + 1, n)
        sets.append(store(rng, lengths, letters))
        poly.append(store(rng, lengths, "A"))
    measure(dev, name, vocab, sets, max_chars, n_steps, hf)
    measure(dev, name + " poly-A", vocab, poly, max_chars, n_steps, hf)


def main():
    parts = {"dna512": ("DNA4", "ACGT", 262144, 512, 512, 4096, 1024, 1024, 16),
             "reads": ("DNA4", "ACGT", 1048576, 150, 150, 4096, 1024, 2048, 32),
             "protein": ("AMINO20", AMINO, 65536, 50, 1024, 8000, 1024, 384, 8),
             "long": ("DNA4", "ACGT", 4096, 8192, 8192, 4096, 8192, 64, 2)}
    chosen = [a for a in sys.argv[1:] if a in parts]
    if not chosen:
        sys.exit(__doc__)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    print("# BPE ids of packed batches: whole calls, buffers alternating; us per call", flush=True)
    for name in chosen:
        part(dev, name, *parts[name])


if __name__ == "__main__":
    main()
