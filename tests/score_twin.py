"""Independent numpy twin of the scored alignment of row pairs (include/bsq.h, "scored alignment of row pairs"): Gotoh's algorithm over
class strings, row by row, and once more cell by cell for small inputs.  Nothing here is shared with the library's cell
(csrc/bsq_score_dev.h).  A row of the table is made from the row above it,

    F[j]  = max(F_above[j], H_above[j] - o) - e                      the gap that runs down the loop string
    Ht[j] = max(H_above[j - 1] + S[u_i][v_j], F[j])   (and 0, local)  everything but the gap along the row
    E[j]  = max over k < j of (Ht[k] + k e) - o - j e                 the gap along the row, one running maximum (valid for o >= 0:
    H[j]  = max(Ht[j], E[j])                                          a gap never opens out of a gap's own end at a gain)

so the cost is a dozen vector operations per character of the loop string, which is the shorter one.  The ends follow the tie rule in
A / B terms whichever string is looped over: the smallest end_a, then the smallest end_b, among the cells that reach the maximum.
"""
import numpy as np

from edit_twin import classes, fit, mutate, pack, random_row, related_pair, store_of  # noqa: F401  (re-exported for the tests)

TOO_LONG, BAD_INDEX = -2**31 + 1, -2**31 + 2
NEG = -(1 << 29)
MAX_LONG = 1 << 20


def gotoh(xa, yb, S, o, e, mode):
    """(score, end_a, end_b, cells that reach the score) of class strings xa (A) and yb (B); S[class of A][class of B]; mode "local" or
    "global".  In global mode the ends are the lengths and the count is 1."""
    xa, yb, S = np.asarray(xa, np.int64), np.asarray(yb, np.int64), np.asarray(S, np.int32)
    local = mode == "local"
    a_loop = xa.size <= yb.size
    u, v = (xa, yb) if a_loop else (yb, xa)
    prof = (S[:, v] if a_loop else S.T[:, v]).astype(np.int32)  # prof[class of the loop string's character][j]
    n = v.size
    ar = np.arange(n + 1, dtype=np.int32)
    are, back = ar * e, o + ar[1:] * e
    H = np.zeros(n + 1, np.int32) if local else np.where(ar == 0, 0, -(o + ar * e)).astype(np.int32)
    F = np.full(n + 1, NEG, np.int32)
    Ht, run, tmp = np.empty(n + 1, np.int32), np.empty(n + 1, np.int32), np.empty(n + 1, np.int32)
    best, end_u, end_v, count = 0, 0, 0, 0
    for i in range(1, u.size + 1):
        np.subtract(H, o, out=tmp)
        np.maximum(F, tmp, out=F)
        F -= e
        Ht[0] = 0 if local else -(o + i * e)
        np.add(H[:-1], prof[u[i - 1]], out=Ht[1:])
        np.maximum(Ht[1:], F[1:], out=Ht[1:])
        if local:
            np.maximum(Ht, 0, out=Ht)
        np.add(Ht, are, out=run)
        np.maximum.accumulate(run, out=run)
        np.subtract(run[:-1], back, out=tmp[1:])
        H, Ht = Ht, H  # (the row above is not read again)
        np.maximum(H[1:], tmp[1:], out=H[1:])
        if local and n:
            top = int(H[1:].max())
            if top > 0 and top >= best:
                at = int(H[1:].argmax()) + 1  # the first column that reaches the row's maximum
                hits = int(np.count_nonzero(H[1:] == top))
                if top > best:
                    best, end_u, end_v, count = top, i, at, hits
                else:
                    count += hits
                    if not a_loop and at < end_v:  # (looping over B: a later row wins only by a smaller end_a)
                        end_u, end_v = i, at
    if local:
        return (best, end_u, end_v, count) if a_loop else (best, end_v, end_u, count)
    return int(H[n]), xa.size, yb.size, 1


def gotoh_cells(xa, yb, S, o, e, mode):
    """The same by the recurrence as written, cell by cell over full tables (small inputs)."""
    local = mode == "local"
    la, lb = len(xa), len(yb)
    H = [[0] * (lb + 1) for _ in range(la + 1)]
    E = [[NEG] * (lb + 1) for _ in range(la + 1)]
    F = [[NEG] * (lb + 1) for _ in range(la + 1)]
    if not local:
        for i in range(1, la + 1):
            H[i][0] = -(o + i * e)
        for j in range(1, lb + 1):
            H[0][j] = -(o + j * e)
    best, ends, count = 0, (0, 0), 0
    for i in range(1, la + 1):
        for j in range(1, lb + 1):
            E[i][j] = max(E[i][j - 1], H[i][j - 1] - o) - e
            F[i][j] = max(F[i - 1][j], H[i - 1][j] - o) - e
            h = max(H[i - 1][j - 1] + int(S[xa[i - 1]][yb[j - 1]]), E[i][j], F[i][j])
            H[i][j] = h = max(h, 0) if local else h
            if local and h > 0:
                if h > best:
                    best, ends, count = h, (i, j), 1
                elif h == best:
                    count += 1
                    ends = min(ends, (i, j))
    if local:
        return best, ends[0], ends[1], count
    return H[la][lb], la, lb, 1


def score_pairs(lut, nchars, chars_a, offsets_a, chars_b, offsets_b, row, col, S, o, e, mode, max_len=4096, one=gotoh):
    """(score int32, ends int32 (n, 2)) of the listed pairs by the rule, codes included."""
    chars_a, chars_b = np.asarray(chars_a, np.uint8), np.asarray(chars_b, np.uint8)
    Ba, Bb = len(offsets_a) - 1, len(offsets_b) - 1
    score, ends = np.empty(len(row), np.int32), np.full((len(row), 2), -1, np.int32)
    for k, (i, j) in enumerate(zip(row, col)):
        if not (0 <= i < Ba and 0 <= j < Bb):
            score[k] = BAD_INDEX
            continue
        x, y = chars_a[offsets_a[i]:offsets_a[i + 1]], chars_b[offsets_b[j]:offsets_b[j + 1]]
        if min(x.size, y.size) > max_len or max(x.size, y.size) > MAX_LONG:
            score[k] = TOO_LONG
            continue
        score[k], ends[k, 0], ends[k, 1], _ = one(classes(lut, nchars, x), classes(lut, nchars, y), S, o, e, mode)
    return score, ends


def self_scores(lut, nchars, chars, offsets, S):
    """The sum of S[c][c] over every row's classes, as Python sums."""
    diag = np.diagonal(np.asarray(S)).astype(np.int64)
    return np.array([int(diag[classes(lut, nchars, np.asarray(chars, np.uint8)[offsets[i]:offsets[i + 1]])].sum()) for i in range(len(offsets) - 1)], np.int64)


def keeps(score, self_a, self_b, min_ratio, min_score=1):
    """The verification rule on Python integers, entry by entry."""
    T = int(float(min_ratio) * 65536 + 0.5)
    return np.array([int(s) > -2**30 and int(s) >= min_score and min(int(a), int(b)) > 0 and int(s) * 65536 >= T * min(int(a), int(b))
                     for s, a, b in zip(score, self_a, self_b)], bool)


def delete_run(x, at, length):
    """x without `length` characters from position `at`."""
    return np.concatenate([x[:at], x[at + length:]])
