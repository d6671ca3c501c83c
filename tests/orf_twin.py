"""numpy twin of ORF extraction, written from the rule of include/bsq.h ("open reading frames"); shared by tests/test_orfs_host.py and
tests/test_orfs_gpu.py.  It does not call the library.

`orfs_of_row` is the rule word for word on one row; `find` is the same rule over a whole batch without a Python loop (the rows
beyond 2^20 need it), and `segments` counts what the min_len filter accepted and rejected."""
import numpy as np

import translate_twin


def orfs_of_row(row, stop=ord("*"), start=-1, min_len=30):
    """[(s, length)] of one row, by the header's words: every terminator (a stop, then the row's end), its segment, its s."""
    row = np.asarray(row, dtype=np.uint8)
    m = row.size
    out = []
    p = -1  # the previous stop
    for e in [int(x) for x in np.nonzero(row == stop)[0]] + [m]:
        first = p + 1
        if start < 0:
            s = first
        else:
            hits = np.nonzero(row[first:e] == start)[0]
            s = first + int(hits[0]) if hits.size else None
        if s is not None and e - s >= min_len:
            out.append((s, e - s))
        p = e
    return out


def _segments(chars, offsets, stop, start):
    """(row, s, e) int64 arrays of every segment of the batch that has an s (start < 0: all of them), unsorted."""
    chars = np.asarray(chars, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.int64)
    n = offsets.size - 1
    total = int(offsets[-1])
    chars = chars[:total]
    stops = np.nonzero(chars == stop)[0].astype(np.int64)
    # a segment begins at every row's first position and behind every stop; it belongs to the row of that stop
    row_of_stop = np.searchsorted(offsets, stops, side="right") - 1
    first = np.concatenate([offsets[:-1], stops + 1])
    row = np.concatenate([np.arange(n, dtype=np.int64), row_of_stop])
    nxt = np.searchsorted(stops, first, side="left")
    end = offsets[row + 1].copy()
    has = nxt < stops.size
    end[has] = np.minimum(end[has], stops[nxt[has]])
    end = np.maximum(end, first)  # (an empty row: its one segment is empty)
    if start < 0:
        return row, first - offsets[row], end - offsets[row]
    marks = np.nonzero(chars == start)[0].astype(np.int64)
    k = np.searchsorted(marks, first, side="left")
    ok = k < marks.size
    s = np.full(first.size, -1, dtype=np.int64)
    s[ok] = marks[k[ok]]
    ok &= s < end
    return row[ok], s[ok] - offsets[row[ok]], end[ok] - offsets[row[ok]]


def find(chars, offsets, stop=ord("*"), start=-1, min_len=30):
    """(row, start, length, orf_offsets, residues) of a batch, ORFs in (row, start) order."""
    offsets = np.asarray(offsets, dtype=np.int64)
    n = offsets.size - 1
    row, s, e = _segments(chars, offsets, stop, start)
    keep = e - s >= min_len
    row, s, e = row[keep], s[keep], e[keep]
    order = np.lexsort((s, row))
    row, s, length = row[order], s[order], (e - s)[order]
    orf_offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n)[:n], out=orf_offsets[1:])
    return row, s, length, orf_offsets, int(length.sum())


def segments(chars, offsets, stop=ord("*"), start=-1, min_len=30):
    """(accepted, rejected): the non-empty candidates [s, e) the min_len filter kept and dropped."""
    _, s, e = _segments(chars, offsets, stop, start)
    size = e - s
    return int((size >= min_len).sum()), int(((size > 0) & (size < min_len)).sum())


def slices(chars, offsets, row, start, length):
    """The ORFs as a packed batch (chars, offsets) cut out of the rows."""
    offsets = np.asarray(offsets, dtype=np.int64)
    out_offs = np.zeros(len(row) + 1, dtype=np.int64)
    np.cumsum(length, out=out_offs[1:])
    pieces = [np.asarray(chars[offsets[r] + s:offsets[r] + s + n], dtype=np.uint8) for r, s, n in zip(row, start, length)]
    return (np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)), out_offs


PIECE = 64    # residues the library's walk takes at a time (csrc/bsq_orf_dev.h), and
ROUND = 256   # ... the pieces a lane has in flight together (csrc/bsq_orf.hip)
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000]


def hand_rows(min_len, seed=0):
    """The hand-made rows of the ORF tests as a packed batch (chars, offsets): filler A, stop *, start M.  Every edge
    of the rule and of the walk's pieces, for this min_len: see the comments."""
    ml = int(min_len)
    A, rows = b"A", []
    rng = np.random.default_rng(seed)
    for n in LENGTHS:
        rows.append(A * n)                                   # no stop: one ORF, the row, if long enough
        if n:
            rows.append(b"*" + A * (n - 1))                  # a stop at position 0
            rows.append(A * (n - 1) + b"*")                  # a stop at the last position
            rows.append(b"M" * n)
            r = rng.choice(np.frombuffer(b"AAAAAAAAAAAAAAAAAAAAAAAACDEFGHIKLMMMX**", np.uint8), n)
            rows.append(r.tobytes())                         # noise: a stop every ~20 residues, an M every ~13
    rows += [b"*", b"**", b"***", b"*" * 64, b"*" * 65, b"*" * 300]                      # nothing but stops: zero ORFs
    rows += [A * 40 + b"**" + A * 40, A * 40 + b"***" + A * 40, A * 62 + b"***" + A * 70]  # two and three stops in a row
    rows += [b"*" + A * ml + b"*" + A * (ml - 1) + b"*" + A * ml,                        # segments of exactly min_len and min_len - 1,
             A * (ml - 1) + b"*" + A * (ml - 1), A * ml + b"*" + A * ml]                 # ... at the row's edges too
    rows += [A * 10 + b"*" + A * (2 * PIECE + 4) + b"*" + A * 3,                         # an ORF whose stops lie two pieces apart
             A * 5 + b"*" + A * (2 * ROUND + 7) + b"*" + A * 90]
    for at in (PIECE, ROUND, 3 * PIECE, 2 * ROUND):                                      # a stop as the last byte of a piece, the first of
        for stops in ((at - 1,), (at,), (at - 1, at)):                                   # the next, and both
            r = bytearray(A * (at + 50))
            for s in stops:
                r[s] = ord("*")
            rows.append(bytes(r))
    # start mode
    rows += [b"*" + A * (ml + 5) + b"*" + A * (ml + 5),                                  # no M in a segment
             b"*M" + A * (ml + 2) + b"*", b"*" + A * (ml + 2) + b"M*", b"M" + A * ml, A * ml + b"M",   # M first / last of a segment
             b"*AA" + b"M" + A * (ml - 1) + b"*", b"*AA" + b"M" + A * max(ml - 2, 0) + b"*",           # M min_len and min_len - 1 in front
             A * 2 + b"M" + A * (ml - 1), A * 2 + b"M" + A * max(ml - 2, 0),                           # ... of the stop / the row's end
             b"*" + A * (ml + 3) + b"M" + A * ml + b"*" + A * (ml + 3) + b"M" + A * max(ml - 2, 0) + b"*",  # an M behind a long stretch without one
             A * 5 + b"M" + A * 700 + b"*", A * 5 + b"M" + A * 700 + b"M" + A * 50]                    # an M carried across many pieces
    for piece in (PIECE, ROUND):                                                         # the deciding M in the piece before the stop's
        k = min(ml // 2, piece - 1)
        r = bytearray(A * (piece + ml + 20))
        r[piece - 1 - k] = ord("M")
        r[piece - 1 - k + ml] = ord("*")
        rows.append(bytes(r))
        r[piece - 1 - k + ml], r[piece - 1 - k + ml - 1] = ord("A"), ord("*")            # ... one residue too close
        rows.append(bytes(r))
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    return np.frombuffer(b"".join(rows), dtype=np.uint8).copy(), offs


def spans(L, code, start, length):
    """[a, b) on the forward strand of the nucleotides an ORF of a frame-`code` row of a source of L characters was read from."""
    f = code % 3
    if code < 3:
        return f + 3 * start, f + 3 * (start + length)
    return L - f - 3 * (start + length), L - f - 3 * start


def dna_store(rng, lens):
    """Rows drawn like tests/test_translate_gpu.py::_store: bases, one character in sixteen from a pool of other bytes."""
    lens = np.asarray(lens, dtype=np.int64)
    total = int(lens.sum())
    chars = rng.choice(np.frombuffer(b"ACGTACGTACGTacgt", np.uint8), total).astype(np.uint8)
    other = rng.random(total) < 1.0 / 16
    chars[other] = rng.choice(np.frombuffer(b"ACGTNacgtnRYKMBVDHSWxX*-.\x00\xff\x80@[`{Uu", np.uint8), int(other.sum()))
    offs = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return chars, offs


def batch_mix():
    """The translated batch of the mix cases: 300 rows of 90 .. 1500 uniform A, C, G, T in six frames (the numpy translation twin)."""
    rng = np.random.default_rng(18)
    lens = rng.integers(90, 1501, 300)
    offs = np.zeros(301, np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(offs[-1])).astype(np.uint8)
    p_chars, p_offs, _ = translate_twin.translate(chars, offs, frame=translate_twin.SIX)
    return p_chars, p_offs
