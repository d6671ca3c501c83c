"""Independent numpy twin of the edit distance of row pairs (include/bsq.h, "edit distance of row pairs"): the plain row-by-row
dynamic programme over class strings, the integer identity rule and a seeded generator of pairs.  Nothing here is shared with the
bit-vector code of the library (csrc/bsq_edit_dev.h): a row of the table is made from the row above it,

    cur[j] = min(prev[j] + 1, prev[j - 1] + (x != y[j - 1]))      deletion, match / substitution
    cur[j] = min(cur[j], cur[j - 1] + 1)                          the insertion chain, as one running minimum of cur - arange

so the cost is one vector operation per character of the first string.
"""
import numpy as np

TOO_LONG, BAD_INDEX = -1, -2


def classes(lut, nchars, row):
    """The class string of a row of bytes: lut[byte] where that is >= 0, else nchars."""
    c = np.asarray(lut, np.int64)[np.asarray(row, np.uint8)]
    return np.where(c >= 0, c, nchars)


def levenshtein(x, y):
    """Unit-cost global edit distance of two integer arrays."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    if x.size > y.size:  # (fewer, longer vector operations)
        x, y = y, x
    ar = np.arange(y.size + 1, dtype=np.int64)
    prev = ar.copy()
    for i in range(x.size):
        cur = np.empty_like(prev)
        cur[0] = i + 1
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (y != x[i]))
        prev = np.minimum.accumulate(cur - ar) + ar
    return int(prev[-1])


def edit_pairs(lut, nchars, chars_a, offsets_a, chars_b, offsets_b, row, col, max_len=4096):
    """dist (int32) of the listed pairs by the rule: -2 for an index out of range, -1 where the shorter side exceeds max_len."""
    chars_a, chars_b = np.asarray(chars_a, np.uint8), np.asarray(chars_b, np.uint8)
    Ba, Bb = len(offsets_a) - 1, len(offsets_b) - 1
    out = np.empty(len(row), np.int32)
    for k, (i, j) in enumerate(zip(row, col)):
        if not (0 <= i < Ba and 0 <= j < Bb):
            out[k] = BAD_INDEX
            continue
        x, y = chars_a[offsets_a[i]:offsets_a[i + 1]], chars_b[offsets_b[j]:offsets_b[j + 1]]
        if min(x.size, y.size) > max_len:
            out[k] = TOO_LONG
            continue
        out[k] = levenshtein(classes(lut, nchars, x), classes(lut, nchars, y))
    return out


def identity_threshold(min_identity):
    return int(float(min_identity) * 65536 + 0.5)


def passes(dist, la, lb, min_identity):
    """The integer identity rule on Python integers, entry by entry."""
    T = identity_threshold(min_identity)
    return np.array([int(d) >= 0 and int(d) * 65536 <= (65536 - T) * max(int(a), int(b)) for d, a, b in zip(dist, la, lb)], bool)


def pack(rows):
    """(chars, offsets) of a list of uint8 arrays."""
    offsets = np.zeros(len(rows) + 1, np.int64)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    chars = np.concatenate([np.asarray(r, np.uint8) for r in rows]) if offsets[-1] else np.zeros(0, np.uint8)
    return chars, offsets


def random_row(rng, n, letters):
    return np.frombuffer(letters.encode(), np.uint8)[rng.integers(0, len(letters), size=n)]


def mutate(rng, x, letters, rate):
    """A copy of x with substitutions, insertions and deletions, each at `rate` per character."""
    alphabet = np.frombuffer(letters.encode(), np.uint8)
    out = []
    for c in x:
        u = rng.random()
        if u < rate:  # deletion
            continue
        if u < 2 * rate:  # substitution by another letter
            c = alphabet[(letters.index(chr(c)) + 1 + rng.integers(0, len(letters) - 1)) % len(letters)]
        out.append(c)
        if rng.random() < rate:  # insertion behind it
            out.append(alphabet[rng.integers(0, len(letters))])
    return np.array(out, np.uint8)


def fit(rng, x, n, letters):
    """x cut or filled with random letters to exactly n characters."""
    return x[:n] if x.size >= n else np.concatenate([x, random_row(rng, n - x.size, letters)])


def related_pair(rng, m, n, letters, rate=None):
    """(short, long) of exactly m and n characters, the long one a mutated copy of the short one (rates 1 - 5 %), filled behind."""
    rate = rng.uniform(0.01, 0.05) if rate is None else rate
    x = random_row(rng, m, letters)
    return x, fit(rng, mutate(rng, x, letters, rate), n, letters)


def cases(seed, letters, lengths=(0, 1, 2, 7, 63, 64, 65, 100, 129, 200)):
    """Seeded pairs of the three kinds -- unrelated random rows, mutated copies, shifted poly-A rows -- as a list of (x, y)."""
    rng = np.random.default_rng(seed)
    out = []
    for m in lengths:
        for n in (m, m + 1, m + 37, 2 * m + 3):
            out.append((random_row(rng, m, letters), random_row(rng, n, letters)))
            out.append(related_pair(rng, m, n, letters))
        a = np.full(m, ord("A"), np.uint8)
        out.append((a, np.concatenate([random_row(rng, 3, letters), a])))  # poly-A, shifted by three
        out.append((np.concatenate([a, random_row(rng, 2, letters)]), np.concatenate([random_row(rng, 1, letters), a])))
    return out


def store_of(pairs):
    """Two stores and the pair list of a list of (x, y): row k of A against row k of B."""
    ca, oa = pack([p[0] for p in pairs])
    cb, ob = pack([p[1] for p in pairs])
    idx = np.arange(len(pairs), dtype=np.int64)
    return ca, oa, cb, ob, idx, idx.copy()
