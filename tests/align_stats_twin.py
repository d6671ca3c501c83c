"""Independent twin of the alignment statistics of row pairs (include/bsq.h, "alignment statistics of row pairs"): the rule as written,
cell by cell over full tables of class strings, every state a (value, (start_a, start_b, matches, diag)) pair in A / B terms.  Nothing
here is shared with the library's cell or packing (csrc/bsq_align_stats_dev.h): no packed words, no pattern / text orientation, Python
integers throughout.  The same rule once more as a numpy sweep over anti-diagonals (`align_stats_diag`), a few hundred times cheaper, for
pairs of full length; the tests pin it to the cell-by-cell programme.  Also the rule of `verify_align_pairs` on Python integers (`keeps`).
"""
import numpy as np

from edit_twin import classes, fit, mutate, pack, random_row, related_pair, store_of  # noqa: F401  (re-exported for the tests)

TOO_LONG, BAD_INDEX = -2**31 + 1, -2**31 + 2
MAX_LEN = 2048
MAX_LONG = 1 << 20
NEG = -(1 << 60)
ZERO = (0, 0, 0, 0)


def align_stats(xa, yb, S, o, e, mode):
    """(score, (start_a, start_b, end_a, end_b, matches, columns)) of class strings xa (A) and yb (B); S[class of A][class of B]."""
    local = mode == "local"
    xa, yb = [int(c) for c in xa], [int(c) for c in yb]
    la, lb = len(xa), len(yb)
    if la == 0 or lb == 0:
        if local:
            return 0, (0, 0, 0, 0, 0, 0)
        return (0 if la + lb == 0 else -(o + (la + lb) * e)), (0, 0, la, lb, 0, la + lb)
    S = [[int(v) for v in r] for r in np.asarray(S)]
    H = [[None] * (lb + 1) for _ in range(la + 1)]
    E = [[None] * (lb + 1) for _ in range(la + 1)]
    F = [[None] * (lb + 1) for _ in range(la + 1)]
    for i in range(la + 1):
        H[i][0] = (0, (i, 0, 0, 0)) if local else ((0 if i == 0 else -(o + i * e)), ZERO)
        E[i][0] = (NEG, ZERO)
    for j in range(lb + 1):
        H[0][j] = (0, (0, j, 0, 0)) if local else ((0 if j == 0 else -(o + j * e)), ZERO)
        F[0][j] = (NEG, ZERO)
    best, cell = 0, None
    for i in range(1, la + 1):
        x = xa[i - 1]
        Hi, Hup, Ei, Fi, Fup, Sx = H[i], H[i - 1], E[i], F[i], F[i - 1], S[x]
        for j in range(1, lb + 1):
            hv, ht = Hi[j - 1]
            ev, et = Ei[j - 1]
            en = (hv - o - e, ht) if hv - o >= ev else (ev - e, et)  # opening wins the tie
            hv, ht = Hup[j]
            fv, ft = Fup[j]
            fn = (hv - o - e, ht) if hv - o >= fv else (fv - e, ft)
            dv, dt = Hup[j - 1]
            y = yb[j - 1]
            d = dv + Sx[y]
            top = max(d, en[0], fn[0])
            if local and top <= 0:
                h = (0, (i, j, 0, 0))
            elif d == top:  # the diagonal, then E, then F
                h = (d, (dt[0], dt[1], dt[2] + (1 if x == y else 0), dt[3] + 1))
            elif en[0] == top:
                h = (top, en[1])
            else:
                h = (top, fn[1])
            Ei[j], Fi[j], Hi[j] = en, fn, h
            if local and h[0] > best:  # (row-major order: the smallest end_a, then the smallest end_b)
                best, cell = h[0], (i, j)
    if local:
        if best == 0:
            return 0, (0, 0, 0, 0, 0, 0)
        i, j = cell
    else:
        i, j = la, lb
    v, (sa, sb, matches, diag) = H[i][j]
    return v, (sa, sb, i, j, matches, (i - sa) + (j - sb) - diag)


def align_stats_diag(xa, yb, S, o, e, mode):
    """(score, (start_a, start_b, end_a, end_b, matches, columns), cells that reach the score) by the same rule as `align_stats`, one
    anti-diagonal d = i + j at a time: the cells (i, d - i) of a diagonal need nothing of each other, only (i, j - 1) and (i - 1, j) of the
    diagonal before and (i - 1, j - 1) of the one before that, so a diagonal is a few dozen numpy operations on int64 arrays indexed by
    i, the boundary cells (0, d) and (d, 0) among them, and three generations of arrays are all that is kept.  A state is a value and a
    (4, la + 1) array of (start_a, start_b, matches, diag) in A / B terms.  In global mode the count is 1; 0 where the local score is 0."""
    local = mode == "local"
    xa, yb, S = np.asarray(xa, np.int64), np.asarray(yb, np.int64), np.asarray(S, np.int64)
    la, lb = xa.size, yb.size
    if la == 0 or lb == 0:
        if local:
            return 0, (0, 0, 0, 0, 0, 0), 0
        return (0 if la + lb == 0 else -(o + (la + lb) * e)), (0, 0, la, lb, 0, la + lb), 1
    yr = yb[::-1].copy()  # (yb[d - i - 1] for i = lo .. hi is yr[lb - d + lo : lb - d + hi + 1])
    rows = np.arange(la + 1, dtype=np.int64)
    gen = [{"H": np.zeros(la + 1, np.int64), "E": np.full(la + 1, NEG, np.int64), "F": np.full(la + 1, NEG, np.int64),
            "HT": np.zeros((4, la + 1), np.int64), "ET": np.zeros((4, la + 1), np.int64), "FT": np.zeros((4, la + 1), np.int64)} for _ in range(3)]

    def edge(g, d):  # the boundary cells of diagonal d: (0, d) and (d, 0)
        for i, j in ((0, d), (d, 0)):
            if i <= la and j <= lb:
                g["H"][i] = 0 if local or d == 0 else -(o + d * e)
                g["HT"][:, i] = (i, j, 0, 0) if local else ZERO
                g["E"][i] = g["F"][i] = NEG
                g["ET"][:, i] = g["FT"][:, i] = 0

    edge(gen[0], 0)
    edge(gen[1], 1)
    best, cell, tup, count = 0, None, None, 0
    for d in range(2, la + lb + 1):
        p2, p1, g = gen[(d - 2) % 3], gen[(d - 1) % 3], gen[d % 3]
        lo, hi = max(1, d - lb), min(la, d - 1)
        at, up = slice(lo, hi + 1), slice(lo - 1, hi)  # row i of a diagonal, row i - 1
        open_e = p1["H"][at] - o >= p1["E"][at]  # opening wins the tie
        en = np.where(open_e, p1["H"][at] - o, p1["E"][at]) - e
        enT = np.where(open_e, p1["HT"][:, at], p1["ET"][:, at])
        open_f = p1["H"][up] - o >= p1["F"][up]
        fn = np.where(open_f, p1["H"][up] - o, p1["F"][up]) - e
        fnT = np.where(open_f, p1["HT"][:, up], p1["FT"][:, up])
        x, y = xa[lo - 1:hi], yr[lb - d + lo:lb - d + hi + 1]
        dg = p2["H"][up] + S[x, y]
        dgT = p2["HT"][:, up].copy()
        dgT[2] += x == y
        dgT[3] += 1
        top = np.maximum(dg, np.maximum(en, fn))
        by_d = dg == top  # the diagonal, then E, then F
        by_e = ~by_d & (en == top)
        hT = np.where(by_d, dgT, np.where(by_e, enT, fnT))
        if local:
            reset = top <= 0
            top = np.where(reset, 0, top)
            hT = np.where(reset, np.stack([rows[at], d - rows[at], rows[at] * 0, rows[at] * 0]), hT)
        g["H"][at], g["E"][at], g["F"][at] = top, en, fn
        g["HT"][:, at], g["ET"][:, at], g["FT"][:, at] = hT, enT, fnT
        edge(g, d)
        if local:
            most = int(top.max())
            if most > 0 and most >= best:
                hits = np.flatnonzero(top == most)
                first = (lo + int(hits[0]), d - lo - int(hits[0]))  # the smallest end_a of this diagonal's
                if most > best:
                    best, cell, tup, count = most, first, hT[:, hits[0]].tolist(), hits.size
                else:
                    count += hits.size
                    if first < cell:  # the smallest end_a, then the smallest end_b
                        cell, tup = first, hT[:, hits[0]].tolist()
    if local:
        if best == 0:
            return 0, (0, 0, 0, 0, 0, 0), 0
        (i, j), v = cell, best
    else:
        g = gen[(la + lb) % 3]
        i, j, v, tup, count = la, lb, int(g["H"][la]), g["HT"][:, la].tolist(), 1
    sa, sb, matches, diag = tup
    return v, (sa, sb, i, j, matches, (i - sa) + (j - sb) - diag), count


def stats_pairs(lut, nchars, chars_a, offsets_a, chars_b, offsets_b, row, col, S, o, e, mode, max_len=MAX_LEN, one=align_stats, counts=None):
    """(score int32, stats int32 (n, 6)) of the listed pairs by the rule, codes included; `one`: the programme (align_stats or
    align_stats_diag).  counts: a list that receives, pair by pair, the programme's count of best cells (None where it gives none)."""
    chars_a, chars_b = np.asarray(chars_a, np.uint8), np.asarray(chars_b, np.uint8)
    Ba, Bb = len(offsets_a) - 1, len(offsets_b) - 1
    score, stats = np.empty(len(row), np.int32), np.full((len(row), 6), -1, np.int32)
    for k, (i, j) in enumerate(zip(row, col)):
        if counts is not None:
            counts.append(None)
        if not (0 <= i < Ba and 0 <= j < Bb):
            score[k] = BAD_INDEX
            continue
        x, y = chars_a[offsets_a[i]:offsets_a[i + 1]], chars_b[offsets_b[j]:offsets_b[j + 1]]
        if min(x.size, y.size) > max_len or max(x.size, y.size) > MAX_LONG:
            score[k] = TOO_LONG
            continue
        got = one(classes(lut, nchars, x), classes(lut, nchars, y), S, o, e, mode)
        score[k], stats[k] = got[:2]
        if counts is not None and len(got) > 2:
            counts[-1] = got[2]
    return score, stats


def keeps(score, stats, la, lb, min_identity=0.9, min_coverage=0.8, identity_over="columns", coverage="both", min_score=1):
    """The rule of verify_align_pairs on Python integers, entry by entry."""
    Ti, Tc = int(float(min_identity) * 65536 + 0.5), int(float(min_coverage) * 65536 + 0.5)
    out = []
    for s, st, a, b in zip(score, stats, la, lb):
        s, a, b = int(s), int(a), int(b)
        sa, sb, ea, eb, matches, columns = (int(v) for v in st)
        D = columns if identity_over == "columns" else min(a, b)
        ok = s > -2**30 and s >= min_score and D > 0 and matches * 65536 >= Ti * D
        cov_a, cov_b = (ea - sa) * 65536 >= Tc * a, (eb - sb) * 65536 >= Tc * b
        shorter, longer = (cov_a, cov_b) if a <= b else (cov_b, cov_a)
        out.append(ok and {"both": cov_a and cov_b, "a": cov_a, "b": cov_b, "shorter": shorter, "longer": longer}[coverage])
    return np.array(out, bool)
