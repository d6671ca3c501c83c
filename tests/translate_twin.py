"""numpy twin of codon translation, written from the rule of include/bsq.h ("codon translation"); shared by
tests/test_translate_host.py and tests/test_translate_gpu.py.  It does not call the library."""
import numpy as np

STANDARD = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
NCBI = "TCAG"  # base numbers of the table's order
SIX = 6


def codon(triple):
    """Table entry of a codon written in letters, e.g. "TGA"."""
    b = [NCBI.index(x) for x in triple]
    return 16 * b[0] + 4 * b[1] + b[2]


def table(table_id=1):
    t = np.frombuffer(STANDARD.encode(), dtype=np.uint8).copy()
    changes = {1: {}, 11: {}, 4: {"TGA": "W"}, 2: {"TGA": "W", "ATA": "M", "AGA": "*", "AGG": "*"}}[table_id]
    for k, v in changes.items():
        t[codon(k)] = ord(v)
    return t


def _base_numbers():
    b = np.full(256, -1, dtype=np.int64)
    for letters, number in (("Tt", 0), ("Uu", 0), ("Cc", 1), ("Aa", 2), ("Gg", 3)):
        for x in letters:
            b[ord(x)] = number
    return b


BASE = _base_numbers()
COMP_BASE = np.array([2, 3, 0, 1], dtype=np.int64)  # T <-> A, C <-> G in NCBI numbers


def length(L, code):
    return max(0, int(L) - code % 3) // 3


def translate_row(row, code, tab, unknown=ord("X")):
    """Residues (uint8) of one source row under frame code 0 .. 5."""
    row = np.asarray(row, dtype=np.uint8)
    f = code % 3
    m = length(row.size, code)
    if m == 0:
        return np.zeros(0, dtype=np.uint8)
    if code < 3:
        b = BASE[row[f:f + 3 * m]].reshape(m, 3)
    else:
        back = row[::-1][f:f + 3 * m]  # s[q], s[q - 1], s[q - 2] with q = L - 1 - f - 3k
        b = BASE[back]
        b = np.where(b >= 0, COMP_BASE[np.maximum(b, 0)], -1).reshape(m, 3)
    ok = (b >= 0).all(axis=1)
    idx = np.where(ok, 16 * b[:, 0] + 4 * b[:, 1] + b[:, 2], 0)
    return np.where(ok, np.asarray(tab, dtype=np.uint8)[idx], unknown).astype(np.uint8)


def translate(chars, offsets, index=None, frame=0, frames=None, tab=None, unknown=ord("X"), capacity=None, cache=None):
    """(chars, offsets, status) of the call: frame 0 .. 5 or SIX for every row, or `frames` one code per row; a bad index or a code > 5
    is an empty row; status by the header's rule (-1, the smallest bad source row, or n_out + the first output row that did not fit).
    chars are cut at `capacity` (None: everything fits).  cache: a dict the caller keeps for ONE (store, table, unknown): a row is
    translated once per frame code however often the index list repeats it."""
    chars = np.asarray(chars, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.int64)
    tab = table(1) if tab is None else tab
    n_store = offsets.size - 1
    idx = np.arange(n_store, dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
    n = idx.size
    pieces, bad = [], []
    cache = {} if cache is None else cache
    for i in range(n):
        codes = range(6) if frame == SIX and frames is None else [int(frames[i]) if frames is not None else frame]
        for c in codes:
            j = int(idx[i])
            if c > 5 or j < 0 or j >= n_store:
                bad.append(i)
                pieces.append(np.zeros(0, dtype=np.uint8))
            else:
                if (j, c) not in cache:
                    cache[(j, c)] = translate_row(chars[offsets[j]:offsets[j + 1]], c, tab, unknown)
                pieces.append(cache[(j, c)])
    n_out = len(pieces)
    out_offs = np.zeros(n_out + 1, dtype=np.int64)
    np.cumsum([p.size for p in pieces], out=out_offs[1:])
    out = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.uint8)
    status = [min(bad)] if bad else []
    if capacity is not None and out_offs[-1] > capacity:
        status.append(n_out + int(np.nonzero(out_offs[1:] > capacity)[0][0]))
        out = out[:capacity]
    return out.astype(np.uint8), out_offs, (min(status) if status else -1)
