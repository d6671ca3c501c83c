"""Sequence packing lab: fill, plan time and encode time of packing.pack_tokenize_packed against its yardsticks on the same batches --
the padded `tokenize_packed` at the same width and the torch composition that yields the same three tensors (padded tokens, a
boolean-mask gather, a scatter, repeat_interleave for the ids; it is handed the library's plan, torch has no building block for it).
Writes profiles/r11/pack_lab.txt (argument: another path).  Times are medians of event-timed repeats, in microseconds; the last
column is the encode's algorithmic bytes (outputs written + characters and offsets read) over its time, as a fraction of 8 TB/s.
Run it under `rocprofv3 --kernel-trace --stats` for the kernel table that goes beside the record."""
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


def lognormal_lengths(seed, n, mean=336.0, sigma=0.75, hi=1022):
    rng = np.random.default_rng(seed)
    mu = np.log(mean) - sigma * sigma / 2
    return np.clip(rng.lognormal(mu, sigma, n), 20, hi).astype(np.int64)


def batch(lens, letters, seed):
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    chars = np.frombuffer(letters.encode(), np.uint8)[rng.integers(0, len(letters), int(offs[-1]))]
    return torch.from_numpy(chars).cuda(), torch.from_numpy(offs).cuda()


def timed(fn, reps=20, warm=3):
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
    return float(np.median(out))


def torch_composition(tok, chars, offs, P, starts, R, width):
    """The same three tensors from a padded encode: gather the live positions, scatter them to their packed places."""
    B = offs.numel() - 1
    w = offs[1:] - offs[:-1] + int(tok.includes_bos()) + int(tok.includes_eos())
    padded = tok.tokenize_packed(chars, offs, width, "q", True, validate=False)
    j = torch.arange(width, device=chars.device)[None, :]
    live = j < w[:, None]
    at = (starts[:-1, None] + j)[live]
    tokens = torch.full((R * P,), tok.pad() if tok.is_padded() else 0, dtype=torch.int64, device=chars.device)
    tokens[at] = padded[live]
    pos = torch.zeros(R * P, dtype=torch.int32, device=chars.device)
    pos[at] = j.expand(B, width)[live].to(torch.int32)
    seq = torch.repeat_interleave(torch.arange(B, device=chars.device), w)
    cover = torch.full((R * P,), -1, dtype=torch.int64, device=chars.device)
    cover[at] = seq
    c2 = cover.view(R, P)
    seg = torch.where(c2 >= 0, 1 + c2 - c2[:, :1], 0).to(torch.int32)
    return tokens.view(R, P), seg, pos.view(R, P)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "r11", "pack_lab.txt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    shapes = [("AMINO20 log-normal", "AMINO20", AA, lognormal_lengths(1, 65536), 1024), ("AMINO20 log-normal", "AMINO20", AA, lognormal_lengths(1, 65536), 2048),
              ("AMINO20 log-normal", "AMINO20", AA, lognormal_lengths(2, 262144), 1024), ("AMINO20 log-normal", "AMINO20", AA, lognormal_lengths(2, 262144), 2048),
              ("DNA reads 140-160", "DNA4", "ACGT", synth.synth_lengths(3, 1 << 20, 140, 160), 1024)]
    lines = ["# sequence packing, int64 tokens + int32 segment_ids + int32 position_ids, BOS + EOS + PAD; times in us (median of 20)",
             "# %-20s %8s %5s %-8s %6s %6s %8s %9s %9s %9s %9s %9s %7s" % ("shape", "B", "P", "mode", "fill1", "fill", "rows", "plan", "encode", "call", "padded", "torch", "of8TB/s")]
    for name, key, letters, lens, P in shapes:
        tok = bioseq_amd.Tokenizer(key, True, True, True)
        chars, offs = batch(lens, letters, 9)
        B = len(lens)
        ntok = int(lens.sum()) + 2 * B
        width = min(P, 1024)  # every run fits 1024 positions: the padded yardstick at width P for P = 1024, and its cheaper self for 2048
        for mode in ("nextfit", "stream"):
            desc_args = dict(mode=mode, validate=False)
            starts, n_rows, _ = packing.pack_plan(tok, chars, offs, P, **desc_args)
            R = int(n_rows)
            t_plan = timed(lambda: packing.pack_plan(tok, chars, offs, P, **desc_args))
            t_call = timed(lambda: packing.pack_tokenize_packed(tok, chars, offs, P, "q", rows=R, **desc_args))
            # the encode launch and the padded yardstick alone: the raw entry points on outputs allocated beforehand
            d = capi.desc_of(tok)
            o_tok = torch.empty((R, P), dtype=torch.int64, device="cuda")
            o_seg, o_pos = (torch.empty((R, P), dtype=torch.int32, device="cuda") for _ in range(2))
            o_pad = torch.empty((B, P), dtype=torch.int64, device="cuda")
            stream = ctypes.c_void_p(capi.raw_stream())
            t_enc = timed(lambda: capi.check(L.bsq_pack_tokenize_device(ctypes.byref(d), chars.data_ptr(), offs.data_ptr(), B, starts.data_ptr(), R, P,
                                                                        capi.U64, o_tok.data_ptr(), o_seg.data_ptr(), o_pos.data_ptr(), stream)))
            t_pad = timed(lambda: capi.check(L.bsq_tokenize_device(ctypes.byref(d), chars.data_ptr(), offs.data_ptr(), B, P, 1, capi.U64,
                                                                   o_pad.data_ptr(), stream)))
            del o_pad
            t_torch = timed(lambda: torch_composition(tok, chars, offs, P, starts, R, width), reps=5, warm=1)
            ref = torch_composition(tok, chars, offs, P, starts, R, width)
            got = packing.pack_tokenize_packed(tok, chars, offs, P, "q", rows=R, **desc_args)
            assert torch.equal(got.tokens, ref[0]) and torch.equal(got.segment_ids, ref[1]) and torch.equal(got.position_ids, ref[2])
            nbytes = R * P * 16 + int(lens.sum()) + 8 * (B + 1) * 2
            lines.append("  %-20s %8d %5d %-8s %6.2f %6.2f %8d %9.1f %9.1f %9.1f %9.1f %9.1f %7.2f"
                         % (name, B, P, mode, ntok / (B * P), ntok / (R * P), R, t_plan, t_enc, t_call, t_pad, t_torch, nbytes / (t_enc * 1e-6) / 8e12))
            print(lines[-1], flush=True)
    lines.append("# fill1: one sequence per row at that width; plan: packing.pack_plan; encode: bsq_pack_tokenize_device alone on outputs allocated beforehand;")
    lines.append("# call: packing.pack_tokenize_packed with rows given (plan + encode + allocations); padded: bsq_tokenize_device int64 (B, P) of the same")
    lines.append("# batch, alone, on an output allocated beforehand; torch: the composition above, handed the plan")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
