"""Plain numpy / Python twins of three of the oldest device paths, shared by tests/test_decode_twin_host.py (which pins them to the
reference fixtures and to the host code) and the GPU tests that judge the kernels with them: the offsets gate
(`bsq_validate_packed_device` / `bsq_validate_lengths_device`), `decode_tokens` and the argmax in front of `decode_logits`.
Written from include/bsq.h and the reference's tokenize.h:83-183, not from the kernels.  No torch."""
import numpy as np

OK, ERR_INVALID_ARG, ERR_DTYPE, ERR_SEQ_TOO_LONG = 0, 2, 3, 4  # bsq_status (include/bsq.h); the host test pins them to capi's


def validate(offsets, B, room, nchars):
    """(status, first_bad) of the gate over offsets[0..B]; `room` = P - bos - eos.  Malformed (only looked for when nchars >= 0):
    the smallest of {i: offsets[i] > offsets[i + 1]}, 0 if offsets[0] < 0, B if offsets[B] > nchars.  Too long: the first i with
    offsets[i + 1] - offsets[i] > room.  Malformed wins."""
    o = np.asarray(offsets, dtype=np.int64)[:B + 1]
    assert o.shape == (B + 1,)
    lens = o[1:] - o[:-1]
    if nchars >= 0:
        bad = [int(i) for i in np.flatnonzero(lens < 0)[:1]]
        if o[0] < 0:
            bad.append(0)
        if o[B] > nchars:
            bad.append(B)
        if bad:
            return ERR_INVALID_ARG, min(bad)
    long = np.flatnonzero(lens > room)
    if long.size:
        return ERR_SEQ_TOO_LONG, int(long[0])
    return OK, -1


def table(lut):
    """The reference's `Tokenizer.lut()` dump (alphabets.json: keys are decimal strings, negative ones included) with int keys."""
    return {int(k): v for k, v in lut.items()}


def table_from_chars(char_ids, bos=None, eos=None, pad=None):
    """The same table, pieces as BYTES, from a character -> id list (alphabets.json `luts`) by the rule of tokenize.h:83-99: the first
    character of every id, then <BOS>, <EOS>, <PAD> in this order.  For BYTES, whose pieces >= 0x80 no JSON string carries."""
    lut = {}
    for i, v in enumerate(char_ids):
        lut.setdefault(int(v), bytes([i]))
    for k, piece in ((bos, b"<BOS>"), (eos, b"<EOS>"), (pad, b"<PAD>")):
        if k is not None:
            lut[int(k)] = piece
    return lut


def golden_bytes_table(alphabets, key, flags):
    """`table_from_chars` of a key x flags ("eos bos pad" digits, e.g. "111") of tests/golden/alphabets.json."""
    m = alphabets["meta"][key][flags]
    return table_from_chars(alphabets["luts"][key], m["bos"] if m["includes_bos"] else None, m["eos"] if m["includes_eos"] else None,
                            m["pad"] if m["is_padded"] else None)


def golden_table(alphabets, key, flags):
    """The reference's own dump of a key x flags; for BYTES, which has none (its pieces >= 0x80 are no text), the table from its
    character list with every byte as the character of that code."""
    m = alphabets["meta"][key][flags]
    if "lut" in m:
        return m["lut"]
    return {k: v.decode("latin-1") for k, v in golden_bytes_table(alphabets, key, flags).items()}


def as_lookup_keys(tokens):
    """Every item as the reference reads it (tokenize.h:107-124, 145-146): loaded UNSIGNED by its item size, narrowed to uint32,
    and looked up as int32.  Returns (uint32 array, int32 array) of the tokens' shape; any strides."""
    a = np.asarray(tokens)
    if a.dtype.itemsize not in (1, 2, 4, 8) or a.dtype.kind not in "iub":
        raise RuntimeError("Unexpected itemsize: expected 1, 2, 4, or 8. Found %d" % a.dtype.itemsize)
    u = a.view("u%d" % a.dtype.itemsize)
    u32 = np.ascontiguousarray((u.astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    return u32, u32.view(np.int32)


def decode(lut, tokens):
    """`decode_tokens`: 1-D -> one text, 2-D -> a list of texts, row by row; str or bytes as the table's pieces are.  The first item
    in row-major order that the table lacks raises RuntimeError("Unexpected/invalid token N"), N the uint32 value."""
    lut = table(lut)
    a = np.asarray(tokens)
    if a.ndim not in (1, 2):
        raise ValueError("Currently supported: 1 or 2 dimensions for decoding tokens.")
    u32, i32 = as_lookup_keys(a)
    keys = np.array(sorted(lut), dtype=np.int32)
    pieces = np.empty(len(keys), dtype=object)
    pieces[:] = [lut[int(k)] for k in keys]
    at = np.minimum(np.searchsorted(keys, i32), len(keys) - 1)
    miss = np.flatnonzero((keys[at] != i32).ravel())  # (ravel of a C-ordered array: row-major)
    if miss.size:
        raise RuntimeError("Unexpected/invalid token %d" % int(u32.ravel()[miss[0]]))
    empty = pieces[0][:0]
    got = pieces[at]
    if a.ndim == 1:
        return empty.join(got.tolist())
    return [empty.join(row) for row in got.tolist()]


def argmax(logits_as_float64):
    """Per row of an (n, C) float64 matrix: the first NaN if the row has one, otherwise the first maximum (torch.argmax's rule).
    -0.0 and +0.0 are equal.  int64[n]."""
    x = np.asarray(logits_as_float64)
    assert x.dtype == np.float64 and x.ndim == 2 and x.shape[1] >= 1
    nan = np.isnan(x)
    below = np.where(nan, -np.inf, x)
    first_max = (below == below.max(axis=1, keepdims=True)).argmax(axis=1)  # (argmax of booleans: the first True)
    return np.where(nan.any(axis=1), nan.argmax(axis=1), first_max).astype(np.int64)
