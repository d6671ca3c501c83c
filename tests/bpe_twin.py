"""An independent Python programme of the BPE rule of include/bsq.h ("BPE ids of a packed batch") in its ONE-MERGE-AT-A-TIME form:
while some adjacent pair is a merge, the occurrence of lowest rank, leftmost among equals, is replaced.  Deliberately not the step
form the kernels and the library's CPU twin run (all occurrences of the lowest rank at once, run parity when l == r).  Plus the
generators the BPE tests share: rows, batches and legal merge tables."""
import numpy as np

DTYPES = {"b": np.int8, "h": np.int16, "i": np.int32, "q": np.uint64, "f": np.float32, "d": np.float64}
KNOWN_MERGES = [("A", "A"), ("C", "G"), ("AA", "A"), ("CG", "T"), ("AA", "AA"), ("T", "T")]
KNOWN = [(b"AAAAAAA", [8, 6]), (b"AAAAA", [4, 6]), (b"ACGTACGT", [0, 7, 0, 7]), (b"AAACGTNAAAA", [6, 7, 10, 8]), (b"TTTTT", [9, 9, 3]),
         (b"CGCGT", [5, 7]), (b"N", [10]), (b"", [])]


def pack(rows):
    """rows (bytes or uint8 arrays) -> (chars uint8, offsets int64)"""
    rows = [np.frombuffer(r, np.uint8) if isinstance(r, (bytes, bytearray)) else np.asarray(r, np.uint8) for r in rows]
    offs = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    return (np.concatenate(rows) if rows else np.zeros(0, np.uint8)).astype(np.uint8), offs


def row_ids(lut, C, merges, row):
    """The ids of one row: lut the 256 class ids (< 0: unmapped), merges an (M, 2) array."""
    V = C + len(merges)
    rank = {(int(l), int(r)): m for m, (l, r) in enumerate(merges)}
    sym = [int(lut[b]) if lut[b] >= 0 else V for b in bytes(row)]
    while True:
        best = None
        for i in range(len(sym) - 1):
            m = rank.get((sym[i], sym[i + 1]))
            if m is not None and (best is None or m < best[0]):
                best = (m, i)
        if best is None:
            return sym
        sym[best[1]:best[1] + 2] = [C + best[0]]


def tokenize(lut, C, merges, flags, chars, offs, P, destchar="q", batch_first=True, max_chars=8192):
    """(tokens, lengths) as the header states them; flags = (eos, bos, padchar) as the Tokenizer constructor orders them."""
    eos, bos, padchar = (int(bool(f)) for f in flags)
    V = C + len(merges)
    bos_id, eos_id, pad_id = V + 1, V + 1 + bos, V + 1 + bos + eos
    B = len(offs) - 1
    tokens = np.zeros((B, P), np.int64)
    lengths = np.zeros(B, np.int32)
    for b in range(B):
        L = max(int(offs[b + 1] - offs[b]), 0)
        if L > max_chars:
            ids, lengths[b] = [], -1
        else:
            ids = row_ids(lut, C, merges, chars[offs[b]:offs[b] + L])
            lengths[b] = len(ids)
        ids = ids[:max(P - bos - eos, 0)]
        row = ([bos_id] if bos else []) + ids + ([eos_id] if eos else [])
        row = (row + [pad_id if padchar else 0] * P)[:P]
        tokens[b] = row
    tokens = tokens if batch_first else tokens.T
    return np.ascontiguousarray(tokens.astype(DTYPES[destchar])), lengths


def random_row(rng, n, letters, unmapped=0.0):
    row = np.frombuffer(letters.encode(), np.uint8)[rng.integers(0, len(letters), n)].copy()
    if unmapped:
        row[rng.random(n) < unmapped] = ord("N") if "N" not in letters else ord("-")
    return row


def low_complexity_row(rng, n, letters):
    """Runs and short repeats: where equal neighbours make the run parity matter."""
    out = []
    while len(out) < n:
        unit = [ord(letters[int(i)]) for i in rng.integers(0, len(letters), int(rng.integers(1, 4)))]
        out += unit * int(rng.integers(1, 40))
    return np.array(out[:n], np.uint8)


def random_table(rng, C, M, small=0.7):
    """A random LEGAL table: merge m names ids below C + m (mostly small ones, so merges fire on random rows), all pairs distinct."""
    seen, out = set(), []
    while len(out) < M:
        hi = C + len(out)
        lo = min(hi, C + 8)
        l, r = (int(rng.integers(0, lo if rng.random() < small else hi)) for _ in range(2))
        if (l, r) not in seen:
            seen.add((l, r))
            out.append((l, r))
    return np.array(out, np.int64).reshape(-1, 2)


def fuzz_rows(rng, letters, count, max_len=160):
    rows = []
    for k in range(count):
        n = int(rng.integers(0, max_len + 1))
        rows.append(low_complexity_row(rng, n, letters) if k % 3 == 0 else random_row(rng, n, letters, 0.03 if k % 3 == 1 else 0.0))
    return rows
