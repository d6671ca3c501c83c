#!/usr/bin/env python3
"""Span-corruption batches (bsq_span_corrupt_device) as whole calls, against the two things a user has today:

    (a) masking.span_corrupt_packed    inputs + labels + both body lengths, one launch
    (b) masking.mlm_tokenize_packed    BERT masking of the same batch with the same element types: about the same bytes, the natural yardstick
    (c) tok.tokenize_packed followed by the torch composition that yields (a)'s four tensors: rand, a dilation by `span`, cumsums and
        scatters.  Its anchors are torch.rand's when it is timed; for the check they are the library's own anchor bits (computed here with
        numpy from the rule of include/bsq.h), and its four tensors are asserted equal to (a)'s on every 97th row.  The lab's rows hold
        mapped letters only and the tokenizer has no BOS / EOS, which spares (c) the unmapped mask and the two special positions.

Timing: device events around whole calls after a warm-up, the three in alternation in one process -- every round times (b), (a), (c) and
(b) again, each as a few calls alternating between two sets of inputs and outputs, so no call finds its inputs in a cache -- and the
figure of a variant is the median of its rounds.  The spread of (b) is (max - min) / median over all its measurements: what a difference
between two variants has to exceed to mean anything.  Nothing here was timed with a profiler attached and no counters were collected.

    python scripts/span_corrupt_lab.py prot512|protein|reads [--quick]     (--quick: an eighth of the rows)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bioseq_amd import Tokenizer, masking  # noqa: E402

QUICK = "--quick" in sys.argv
ROUNDS = 3 if QUICK else 7
FRAC = 0.15
MAX_SENTINELS = 100
PEAK = 8e12  # bytes per second
AMINO = "ACDEFGHIKLMNPQRSTVWY"


def mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def anchor_bits(rows, P, anchor_prob, seed):
    """bool (len(rows), P): anchor(a) of include/bsq.h, "span corruption", for the row keys `rows`"""
    with np.errstate(over="ignore"):
        h = mix64((np.uint64(seed) ^ np.uint64(0x5350414E43525054)) + np.uint64(0x9E3779B97F4A7C15) * (rows.astype(np.uint64) + np.uint64(1)))
        a = np.arange(P, dtype=np.uint64)
        w = mix64(h[:, None] + np.uint64(0xD1342543DE82EF95) * ((a >> np.uint64(2)) + np.uint64(1))[None, :])
        v = (w >> (np.uint64(16) * (a & np.uint64(3)))[None, :]) & np.uint64(0xFFFF)
    return v < np.uint64(int(np.floor(anchor_prob * 65536 + 0.5)))


def per_call(fn, reps):
    """us per call of `reps` calls (even: both buffer sets take turns)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def compose(tok, chars, offs, P, tdt, span, first, anchors):
    """(c): the four tensors of span_corrupt_packed(..., P, P) from tokenize_packed's rows, in torch"""
    dev = chars.device
    B = offs.numel() - 1
    tokens = tok.tokenize_packed(chars, offs, P, "q", True, validate=False)
    lens = offs[1:] - offs[:-1]
    valid = torch.arange(P, device=dev)[None, :] < lens[:, None]
    cov = anchors.clone()
    for s in range(1, span):
        cov[:, s:] |= anchors[:, :-s]
    cand = cov & valid
    start = cand.clone()
    start[:, 1:] &= ~cand[:, :-1]
    g = torch.cumsum(start, 1) - 1
    sel = cand & (g < MAX_SENTINELS)
    sstart = start & sel
    sentinel = first + g
    keep = valid & (~sel | sstart)
    in_pos = torch.cumsum(keep, 1) - 1
    inputs = torch.zeros((B, P), dtype=tdt, device=dev)
    row = torch.arange(B, device=dev)[:, None].expand(B, P)
    inputs[row[keep], in_pos[keep]] = torch.where(sstart, sentinel, tokens)[keep].to(tdt)
    tok_pos = torch.cumsum(sel, 1) - 1 + torch.cumsum(sstart, 1)
    labels = torch.full((B, P), -100, dtype=torch.int64, device=dev)
    put = sel & (tok_pos < P)
    labels[row[put], tok_pos[put]] = tokens[put]
    put = sstart & (tok_pos - 1 < P)
    labels[row[put], tok_pos[put] - 1] = sentinel[put]
    return inputs, labels, keep.sum(1).int(), (sel.sum(1) + sstart.sum(1)).int()


def measure(dev, name, key, sets, dc, span):
    tok = Tokenizer(key, False, False, False)
    first = tok.alphabet_size()
    lens = np.diff(sets[0][1])
    B, P = lens.size, int(lens.max())
    tdt = torch.int64 if dc == "q" else torch.int16
    prob = 1.0 - (1.0 - FRAC) ** (1.0 / span)
    dsets = [[torch.from_numpy(x).to(dev) for x in s] for s in sets]

    def corrupt(i):
        ch, of = dsets[i & 1]
        return masking.span_corrupt_packed(tok, ch, of, P, P, dc, frac=FRAC, span=span, seed=5, validate=False)

    def mlm(i):
        ch, of = dsets[i & 1]
        return masking.mlm_tokenize_packed(tok, ch, of, P, dc, True, frac=FRAC, seed=5, validate=False)

    def composed(i):
        ch, of = dsets[i & 1]
        return compose(tok, ch, of, P, tdt, span, first, torch.rand((B, P), device=dev) < prob)

    # the check: every 97th row, (c) with the library's anchors against (a)
    pick = np.arange(0, B, 97)
    ch, of = sets[0]
    sch = np.concatenate([ch[of[k]:of[k + 1]] for k in pick])
    sof = np.concatenate([[0], np.cumsum(lens[pick])]).astype(np.int64)
    want = [t[torch.from_numpy(pick).to(dev)] for t in corrupt(0)]
    got = compose(tok, torch.from_numpy(sch).to(dev), torch.from_numpy(sof).to(dev), P, tdt, span, first,
                  torch.from_numpy(anchor_bits(pick, P, prob, 5)).to(dev))
    torch.cuda.synchronize()
    for what, w, g in zip(("inputs", "labels", "in_len", "tgt_len"), want, got):
        assert torch.equal(w, g), "the torch composition and the kernel differ in " + what
    in_mean, tgt_mean, cut = float(want[2].float().mean()), float(want[3].float().mean()), int((want[3] > P).sum())
    del want, got

    for fn in (mlm, corrupt, composed):
        fn(0), fn(1)
    torch.cuda.synchronize()
    reps = max(2, int((0.02 if QUICK else 0.06) / max(per_call(mlm, 2) / 1e6, 1e-6)))
    reps += reps & 1
    ta, tb, tc = [], [], []
    for _ in range(ROUNDS):
        tb.append(per_call(mlm, reps))
        ta.append(per_call(corrupt, reps))
        tc.append(per_call(composed, max(2, reps // 8 * 2)))
        tb.append(per_call(mlm, reps))
    a, b, c = float(np.median(ta)), float(np.median(tb)), float(np.median(tc))
    spread = (max(tb) - min(tb)) / b
    moved = int(lens.sum()) + 8 * (B + 1) + B * P * (tdt.itemsize + 8) + 8 * B  # characters + offsets + both matrices (+ the two length vectors)
    print("%-8s %-7s %8d rows x P %4d %s/q span %d | body means: inputs %.1f, targets %.1f, %d sampled label rows cut | (a) corrupt %9.1f us  "
          "(b) mlm %9.1f us  (c) tokenize + torch %9.1f us | (a)/(b) %.3f  (a)/(c) %.3f | spread of (b) %.3f (%d measurements, %d calls each) | "
          "%.0f MB moved, %.0f GB/s = %.3f of 8 TB/s | %s"
          % (name, key, B, P, dc, span, in_mean, tgt_mean, cut, a, b, c, a / b, a / c, spread, len(tb), reps, moved / 1e6, moved / a / 1e3,
             moved / (a * 1e-6) / PEAK, "LOSES to (b)" if a > b * (1 + spread) else "within (b)" if a > b * (1 - spread) else "ahead of (b)"),
          flush=True)
    if a > c:
        print("    ^ LOSES to (c)", flush=True)


def store(rng, lens, letters):
    pool = np.frombuffer(letters.encode(), np.uint8)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return pool[rng.integers(0, pool.size, int(offs[-1]))], offs


def main():
    parts = {"prot512": ("AMINO20", AMINO, 262144, 512, 512), "protein": ("AMINO20", AMINO, 65536, 50, 1024), "reads": ("DNA4", "ACGT", 1048576, 150, 150)}
    chosen = [a for a in sys.argv[1:] if a in parts]
    if not chosen:
        sys.exit(__doc__)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    print("# span-corruption batches: whole calls in alternation; us per call, medians of %d rounds; frac %.2f, max_sentinels %d, P_tgt = P_in = P"
          % (ROUNDS, FRAC, MAX_SENTINELS), flush=True)
    for name in chosen:
        key, letters, n_rows, lo, hi = parts[name]
        sets = []
        for seed in (1, 2):
            rng = np.random.default_rng(seed)
            sets.append(store(rng, rng.integers(lo, hi + 1, n_rows // (8 if QUICK else 1)), letters))
        for dc in ("q", "h"):
            for span in (3, 1):
                measure(dev, name, key, sets, dc, span)


if __name__ == "__main__":
    main()
