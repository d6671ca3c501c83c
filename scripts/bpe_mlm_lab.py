#!/usr/bin/env python3
"""Masked-LM batches over BPE ids (bsq_bpe_mlm_tokenize_device) as whole calls, against what a user composes today, at the four shapes
and merge tables of scripts/bpe_lab.py (its seeds, its trainer, its stores):

    (a) bpe_mlm_tokenize_packed     inputs int16 + labels int64 + lengths, one launch
    (b) bpe_tokenize_packed         the plain ids, int16: the kernel the masked call extends, unchanged
    (c) (b) followed by the torch composition that yields int16 inputs and int64 labels from (b)'s output: rand, compare, where,
        randint, where -- BERT's 80 / 10 / 10 with torch's generator (its masks depend on the batch's shape and the stream)

Timing: device events around whole calls after a warm-up, the three in alternation in one process -- every round times (b), (a), (c)
and (b) again, each as a few calls alternating between two sets of inputs and outputs -- and the figure of a variant is the median of
its rounds.  The spread of (b) is (max - min) / median over all its measurements, both per round: what a difference between two
variants has to exceed to mean anything.  Nothing here was timed with a profiler attached and no counters were collected.  Before
timing, (a)'s inputs, labels and lengths of every 64th row are asserted equal to the host twin's.

    python scripts/bpe_mlm_lab.py dna512|reads|protein|long [--quick]     (--quick: an eighth of the rows, a quarter of the merges)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bpe_lab  # noqa: E402  (store, the shapes' seeds; it reads --quick from the command line as this script does)
from bioseq_amd import Tokenizer, bpe  # noqa: E402

QUICK = bpe_lab.QUICK
SHRINK = bpe_lab.SHRINK
ROUNDS = 3 if QUICK else 7
FRAC = 0.15


def per_call(fn, reps):
    """us per call of `reps` calls (even: both buffer sets take turns)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def measure(dev, name, vocab, sets, max_chars):
    B = sets[0][1].size - 1
    lens = np.diff(sets[0][1])
    P = int(lens.max())
    V = vocab.desc.nchars + vocab.M
    mask_token = bpe.bpe_vocab_size(vocab)
    dsets = [[torch.from_numpy(x).to(dev) for x in s] for s in sets]
    vocab.device_table(dev)

    def mlm(i):
        ch, of = dsets[i & 1]
        return bpe.bpe_mlm_tokenize_packed(vocab, ch, of, P, "h", frac=FRAC, seed=5, first_row=0, max_chars=max_chars)

    def plain(i):
        ch, of = dsets[i & 1]
        return bpe.bpe_tokenize_packed(vocab, ch, of, P, "h", max_chars=max_chars)

    def composed(i):
        tokens, lengths = plain(i)
        token = (torch.arange(P, device=dev)[None, :] < lengths[:, None]) & (tokens != V)
        sel = token & (torch.rand((B, P), device=dev) < FRAC)
        labels = torch.where(sel, tokens.to(torch.int64), -100)
        r = torch.rand((B, P), device=dev)
        ids = torch.randint(0, V, (B, P), dtype=torch.int16, device=dev)
        inputs = torch.where(sel & (r < 0.9), ids, tokens).masked_fill_(sel & (r < 0.8), mask_token)
        return inputs, labels, lengths

    # the sample: every 64th row against the host twin
    pick = np.arange(0, B, 64)
    rows = [sets[0][0][sets[0][1][k]:sets[0][1][k + 1]] for k in pick]
    sch = np.concatenate(rows)
    sof = np.zeros(pick.size + 1, np.int64)
    np.cumsum([r.size for r in rows], out=sof[1:])
    got = mlm(0)
    torch.cuda.synchronize()
    for k, e in zip(pick[:4], range(4)):  # rows keyed by their index in the batch: the twin takes them one by one
        hi, hl, hn = bpe.bpe_mlm_tokenize_host(vocab, sch[sof[e]:sof[e + 1]], sof[e:e + 2] - sof[e], P, "h", frac=FRAC, seed=5, first_row=int(k), max_chars=max_chars)
        assert np.array_equal(got[0][k].cpu().numpy(), hi[0]) and np.array_equal(got[1][k].cpu().numpy(), hl[0].view(np.int64)) and int(got[2][k]) == int(hn[0]), \
            "the device and the host twin differ"
    host_t, host_l = bpe.bpe_tokenize_host(vocab, sch, sof, P, "h", max_chars=max_chars)
    lab = got[1].cpu().numpy()[::64]
    on = lab != -100
    assert np.array_equal(got[2].cpu().numpy()[::64], host_l) and np.array_equal(lab[on], host_t.astype(np.int64)[on]), "labels are not the plain ids"
    n_tokens, n_sel = int(host_l.sum()), int(on.sum())
    del got

    for fn in (plain, mlm, composed):
        fn(0), fn(1)
    torch.cuda.synchronize()
    reps = max(2, int((0.02 if QUICK else 0.08) / max(per_call(plain, 2) / 1e6, 1e-6)))
    reps += reps & 1
    ta, tb, tc = [], [], []
    for _ in range(ROUNDS):
        tb.append(per_call(plain, reps))
        ta.append(per_call(mlm, reps))
        tc.append(per_call(composed, reps))
        tb.append(per_call(plain, reps))
    a, b, c = float(np.median(ta)), float(np.median(tb)), float(np.median(tc))
    spread = (max(tb) - min(tb)) / b
    token_bytes, label_bytes = B * P * 2, B * P * 8
    allowance = label_bytes / (token_bytes / b)  # the label matrix at (b)'s own store rate
    print("%-8s %s M %4d max_chars %4d %-15s | %8d rows x P %4d, sample: %.2f chars per token, %.4f of the tokens selected | "
          "(a) mlm %9.1f us  (b) plain %9.1f us  (c) plain + torch %9.1f us | (a)/(b) %.3f  (a)/(c) %.3f | spread of (b) %.3f (%d measurements, "
          "%d calls each) | (a) - (b) %8.1f us = labels' %.0f MB at %.0f GB/s; (b) + labels at (b)'s store rate %.1f us: (a) %s"
          % (name, vocab.tok.key, vocab.M, max_chars, bpe.bpe_mlm_kernel_name(max_chars=max_chars), B, P, int(lens[pick].sum()) / max(n_tokens, 1),
             n_sel / max(n_tokens, 1), a, b, c, a / b, a / c, spread, len(tb), reps, a - b, label_bytes / 1e6, label_bytes / max(a - b, 1e-3) / 1e3,
             b + allowance, "within" if a <= (b + allowance) * (1 + spread) else "EXCEEDS"), flush=True)


def part(dev, name, key, letters, n_rows, lo, hi, n_merges, max_chars, sample_rows, _n_steps):
    tok = Tokenizer(key, False, False, False)
    n = n_rows // SHRINK
    rng = np.random.default_rng(len(name))
    t0 = time.perf_counter()
    vocab = bpe.bpe_train_host(tok, *bpe_lab.store(rng, rng.integers(lo, hi + 1, sample_rows), letters), n_merges // (4 if QUICK else 1))
    print("# %s: %d merges trained on %d rows in %.1f s" % (name, vocab.M, sample_rows, time.perf_counter() - t0), flush=True)
    sets = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        sets.append(bpe_lab.store(rng, rng.integers(lo, hi + 1, n), letters))
    measure(dev, name, vocab, sets, max_chars)


def main():
    parts = {"dna512": ("DNA4", "ACGT", 262144, 512, 512, 4096, 1024, 1024, 16),
             "reads": ("DNA4", "ACGT", 1048576, 150, 150, 4096, 1024, 2048, 32),
             "protein": ("AMINO20", bpe_lab.AMINO, 65536, 50, 1024, 8000, 1024, 384, 8),
             "long": ("DNA4", "ACGT", 4096, 8192, 8192, 4096, 8192, 64, 2)}
    chosen = [a for a in sys.argv[1:] if a in parts]
    if not chosen:
        sys.exit(__doc__)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    print("# BPE masked-LM batches: whole calls in alternation, int16 inputs + int64 labels; us per call, medians of %d rounds" % ROUNDS, flush=True)
    for name in chosen:
        part(dev, name, *parts[name])


if __name__ == "__main__":
    main()
