"""Packed masked-LM lab: the one launch of packing.pack_mlm_tokenize_packed (bsq_pack_mlm_tokenize_device) against its yardsticks on
the same batches, all timed in the same session:
  (a) the plain packed encode bsq_pack_tokenize_device (one matrix less, no draw);
  (b) the padded masked batch bsq_mlm_tokenize_device at the same width (one sequence per row);
  (c) the torch composition that yields the same four tensors from the plain packed encode's output: rand / where over the matrices
      (another random stream: the count of label positions is compared, not the bits).
Writes profiles/r12/pack_mlm_lab.txt (argument: another path).  Times in microseconds: `med` the median of event-timed single launches,
`sus` the mean of a back-to-back window of launches between two events (at least ~0.3 s of work).  The last columns are the new launch's
algorithmic bytes (outputs written + characters and offsets read) over its sustained time as a fraction of 8 TB/s, and the time a plain
write of the label matrix would take at the rate (a) achieves.  Run it under `rocprofv3 --kernel-trace --stats` for the kernel table."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bioseq_amd  # noqa: E402
from bioseq_amd import capi, packing, synth  # noqa: E402

L = capi.load()

AA = "ACDEFGHIKLMNPQRSTVWY"
FRAC = 0.15


def lognormal_lengths(seed, n, mean=336.0, sigma=0.75, hi=1022):
    rng = np.random.default_rng(seed)
    mu = np.log(mean) - sigma * sigma / 2
    return np.clip(rng.lognormal(mu, sigma, n), 20, hi).astype(np.int64)


def batch(lens, letters, seed):
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    chars = np.frombuffer(letters.encode(), np.uint8)[rng.integers(0, len(letters), int(offs[-1]))]
    return torch.from_numpy(chars).cuda(), torch.from_numpy(offs).cuda()


def timed(fn, reps=15, warm=3, window_s=0.3):
    """(median of event-timed single calls, mean of one back-to-back window), microseconds."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0)
    med = float(np.median(out))
    n = int(min(2000, max(10, window_s * 1e6 / max(med, 1.0))))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return med, a.elapsed_time(b) * 1000.0 / n


def torch_composition(tok, tokens, seg, nchars, mask_token, gen):
    """Masked inputs and labels from the plain packed encode's tokens (segment_ids and position_ids are its own): BERT's 80/10/10."""
    special = (seg == 0) | (tokens >= nchars)  # PAD gaps, BOS / EOS / PAD ids
    r = torch.rand(tokens.shape, device=tokens.device, generator=gen)
    sel = (r < FRAC) & ~special
    labels = torch.where(sel, tokens, -100)
    c = torch.rand(tokens.shape, device=tokens.device, generator=gen)
    rnd = torch.randint(0, nchars, tokens.shape, device=tokens.device, generator=gen)
    inputs = torch.where(sel & (c < 0.8), mask_token, torch.where(sel & (c < 0.9), rnd, tokens))
    return inputs, labels


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "r12", "pack_mlm_lab.txt")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    quick = os.environ.get("PACK_MLM_LAB_QUICK") == "1"  # the rocprofv3 run: every kernel a few times, nothing else
    shapes = [("AMINO20 log-normal", "AMINO20", AA, lognormal_lengths(1, 65536), 1024, "qq"), ("AMINO20 log-normal", "AMINO20", AA, lognormal_lengths(1, 65536), 2048, "qq"),
              ("AMINO20 log-normal", "AMINO20", AA, lognormal_lengths(2, 262144), 1024, "qq"), ("AMINO20 log-normal", "AMINO20", AA, lognormal_lengths(2, 262144), 2048, "qq"),
              ("DNA reads 140-160", "DNA4", "ACGT", synth.synth_lengths(3, 1 << 20, 140, 160), 1024, "qq"),
              ("AMINO20 log-normal", "AMINO20", AA, lognormal_lengths(2, 262144), 1024, "bq")]
    lines = ["# packed masked-LM batches: inputs + int64 labels + int32 segment_ids + int32 position_ids, BOS + EOS + PAD, frac 0.15, 80/10/10; times in us",
             "# %-20s %8s %5s %-8s %-3s %8s | %9s %9s | %9s %9s %6s | %9s %9s | %9s %6s %6s | %7s %9s" % (
                 "shape", "B", "P", "mode", "in", "rows", "new med", "new sus", "(a) med", "(a) sus", "new/a", "(b) med", "(b) sus", "(c) sus", "c/new", "count", "of8TB/s", "lab-write")]
    for name, key, letters, lens, P, pair in shapes:
        tok = bioseq_amd.Tokenizer(key, True, True, True)
        d = capi.desc_of(tok)
        nchars = int(d.nchars)
        chars, offs = batch(lens, letters, 9)
        B = len(lens)
        in_dt, in_t = capi.dtype_of(pair[0])
        isz = torch.empty(0, dtype=in_t).element_size()
        m = capi.Mlm(FRAC, 0.8, 0.1, tok.alphabet_size(), -100, 12345, 0)
        stream = ctypes.c_void_p(capi.raw_stream())
        for mode in ("nextfit", "stream"):
            starts, n_rows, _ = packing.pack_plan(tok, chars, offs, P, mode=mode, validate=False)
            R = int(n_rows)
            o_in = torch.empty((R, P), dtype=in_t, device="cuda")
            o_lab = torch.empty((R, P), dtype=torch.int64, device="cuda")
            o_seg, o_pos = (torch.empty((R, P), dtype=torch.int32, device="cuda") for _ in range(2))

            def new():
                capi.check(L.bsq_pack_mlm_tokenize_device(ctypes.byref(d), chars.data_ptr(), offs.data_ptr(), B, starts.data_ptr(), R, P, ctypes.byref(m),
                                                          in_dt, o_in.data_ptr(), capi.U64, o_lab.data_ptr(), o_seg.data_ptr(), o_pos.data_ptr(), stream))

            def plain():
                capi.check(L.bsq_pack_tokenize_device(ctypes.byref(d), chars.data_ptr(), offs.data_ptr(), B, starts.data_ptr(), R, P, in_dt,
                                                      o_in.data_ptr(), o_seg.data_ptr(), o_pos.data_ptr(), stream))

            if quick:
                for _ in range(3):
                    new(), plain()
                torch.cuda.synchronize()
                continue
            t_new = timed(new)
            t_a = timed(plain)
            p_in = torch.empty((B, P), dtype=in_t, device="cuda")
            p_lab = torch.empty((B, P), dtype=torch.int64, device="cuda")
            t_b = timed(lambda: capi.check(L.bsq_mlm_tokenize_device(ctypes.byref(d), chars.data_ptr(), offs.data_ptr(), B, P, 1, ctypes.byref(m), in_dt,
                                                                     p_in.data_ptr(), capi.U64, p_lab.data_ptr(), stream)))
            del p_in, p_lab
            gen = torch.Generator(device="cuda").manual_seed(1)
            tokens64 = torch.empty((R, P), dtype=torch.int64, device="cuda")

            def composed():
                capi.check(L.bsq_pack_tokenize_device(ctypes.byref(d), chars.data_ptr(), offs.data_ptr(), B, starts.data_ptr(), R, P, capi.U64,
                                                      tokens64.data_ptr(), o_seg.data_ptr(), o_pos.data_ptr(), stream))
                return torch_composition(tok, tokens64, o_seg, nchars, tok.alphabet_size(), gen)

            t_c = timed(composed, reps=3, warm=1, window_s=0.1)
            n_c = int((composed()[1] != -100).sum())
            new()
            n_new = int((o_lab != -100).sum())
            del tokens64
            out_bytes = R * P * (isz + 8 + 8)
            nbytes = out_bytes + int(lens.sum()) + 8 * (B + 1) * 2
            a_bytes = R * P * (isz + 8) + int(lens.sum()) + 8 * (B + 1) * 2
            lab_write = R * P * 8 / (a_bytes / t_a[1])  # us: the label matrix at the byte rate (a) achieves
            lines.append("  %-20s %8d %5d %-8s %-3s %8d | %9.1f %9.1f | %9.1f %9.1f %6.2f | %9.1f %9.1f | %9.1f %6.2f %6.3f | %7.2f %9.1f"
                         % (name, B, P, mode, pair, R, t_new[0], t_new[1], t_a[0], t_a[1], t_new[1] / t_a[1], t_b[0], t_b[1], t_c[1], t_c[1] / t_new[1],
                            n_new / max(n_c, 1), nbytes / (t_new[1] * 1e-6) / 8e12, lab_write))
            print(lines[-1], flush=True)
            del o_in, o_lab, o_seg, o_pos
            torch.cuda.empty_cache()
    if quick:
        return
    lines.append("# new: bsq_pack_mlm_tokenize_device alone on outputs allocated beforehand; (a): bsq_pack_tokenize_device, inputs' type, same plan;")
    lines.append("# (b): bsq_mlm_tokenize_device (B, P) of the same batch; (c): bsq_pack_tokenize_device int64 + the torch composition; count: label")
    lines.append("# positions of the new launch over those of (c) (another random stream: near 1, not 1); lab-write: us a plain write of the label matrix")
    lines.append("# takes at the byte rate (a) achieves -- new sus should be near (a) sus + lab-write")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
