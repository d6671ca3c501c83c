"""bsq_onehot_device_multi / bsq_onehot_multi_plan without a device: the symbols, which batches the plan fuses (for fabricated, never
dereferenced pointer values) and the argument errors, which the multi call reports before any HIP call."""
import ctypes
import os

import pytest

from bioseq_amd import capi

BASE = 1 << 40  # a 4-KiB aligned fake device address: the plan reads pointer values, never what they point at


def _lib():
    return capi.load()


def _desc(key, bos=False, eos=False, pad=False):
    return capi.make_desc(key, eos, bos, pad)


def _table(shapes, misalign=0):
    """shapes: list of (B, masked)"""
    n = len(shapes)
    arr = (capi.OnehotBatch * max(n, 1))()
    for i, (B, masked) in enumerate(shapes):
        arr[i].chars = BASE
        arr[i].offsets = BASE
        arr[i].mask = BASE if masked else None
        arr[i].B = B
        arr[i].out = BASE + (i << 34) + misalign
    return arr


def _plan(desc, shapes, P, layout, t, misalign=0):
    n = len(shapes)
    fam = (ctypes.c_int32 * max(n, 1))()
    r = _lib().bsq_onehot_multi_plan(ctypes.byref(desc), n, _table(shapes, misalign), P, layout, t, fam)
    return r, list(fam)[:n]


def test_symbols_declared_and_exported():
    names = capi.declared_symbols()
    L = _lib()
    for s in ("bsq_onehot_device_multi", "bsq_onehot_multi_plan"):
        assert s in names
        assert hasattr(L, s)
    text = open(capi.HEADER_PATH).read()
    assert "bsq_onehot_batch" in text


def test_chunk_owner_batches_share_one_launch():
    assert _plan(_desc("AMINO20"), [(8192, 0)] * 4, 1024, 0, capi.F32) == (1, [1] * 4)
    assert _plan(_desc("DNA"), [(1024, 0)] * 8, 256, 0, capi.F32) == (1, [1] * 8)
    # masks do not change the chunk-owner kernel
    assert _plan(_desc("AMINO20"), [(8192, 1), (8192, 0), (4096, 1)], 1024, 0, capi.F32) == (1, [1] * 3)


def test_one_piece_two_pass_batches_share_two_launches():
    assert _plan(_desc("DNA4", True, True, True), [(131072, 0)] * 4, 160, 0, capi.F32) == (2, [2] * 4)
    assert _plan(_desc("DNA4", True, True, True), [(262144, 0)] * 4, 160, 0, capi.I8) == (2, [2] * 4)


def test_channels_first_chunk_stream_shares_one_launch():
    # the cnn loader's batch: k_tokenize_chunks<HOT> in its plain form, family 3, masked or not
    assert _plan(_desc("SEB8"), [(4096, 0)] * 4, 512, 1, capi.F32) == (1, [3] * 4)
    assert _plan(_desc("SEB8"), [(4096, 1), (100, 0), (3, 1)], 512, 1, capi.I8) == (1, [3] * 3)
    # outputs that are only element-aligned, or P % (16 / sizeof(T)) != 0: the ragged form -- single calls
    assert _plan(_desc("SEB8"), [(4096, 0)] * 4, 512, 1, capi.F32, misalign=4) == (0, [0] * 4)
    assert _plan(_desc("SEB8"), [(4096, 0)] * 4, 510, 1, capi.F32) == (0, [0] * 4)
    # a (B,C,P) batch of 256 MB and more is the two-pass form: its single call; its neighbour is then alone in its family too
    assert _plan(_desc("SEB8"), [(4096, 0), (70000, 0)], 512, 1, capi.F32) == (0, [0, 0])


def test_two_pass_keys_8_byte_elements_and_mixed_keys():
    # byte ids, 8-byte elements (k_expand_chunks<uint64_t>)
    for t in (capi.F64, capi.U64):
        assert _plan(_desc("DNA4", True, True, True), [(100000, 0), (100077, 0)], 160, 0, t) == (2, [2, 2])
    # DNA5 f32 at padlen 64: 200000 sequences keep byte ids, 2.1 M have more than 128 MB of them and take nibbles -- another key, alone in it
    r, fam = _plan(_desc("DNA5"), [(200000, 0), (2100000, 0), (200005, 0)], 64, 0, capi.F32)
    assert fam == [2, 0, 2] and r == 2


def test_mixed_group():
    # int8 DNA4 + BOS / EOS / PAD: a chunk-owner pair (small outputs), a two-pass pair (k_expand_rows1<nibbles>) and a tiled batch, which runs
    # as its single call
    d = _desc("DNA4", True, True, True)
    L = _lib()
    assert L.bsq_onehot_kernel_name(ctypes.byref(d), 4096, 160, capi.I8) == b"k_onehot_chunks"
    assert L.bsq_onehot_kernel_name(ctypes.byref(d), 65536, 160, capi.I8) == b"k_onehot_tile"
    r, fam = _plan(d, [(4096, 0), (262144, 0), (65536, 0), (4096, 0), (262144, 0)], 160, 0, capi.I8)
    assert fam == [1, 2, 0, 1, 2] and r == 3
    # the same with a masked two-pass batch (its single call) among them, f32
    r, fam = _plan(d, [(8192, 0), (131072, 0), (131072, 1), (8192, 0), (131072, 0)], 160, 0, capi.F32)
    assert fam == [1, 2, 0, 1, 2] and r == 3


def test_single_member_of_a_family_runs_alone():
    d = _desc("DNA4", True, True, True)
    r, fam = _plan(d, [(8192, 0), (131072, 0)], 160, 0, capi.F32)
    assert fam == [0, 0] and r == 0


def test_nineteen_batches_three_groups():
    assert _plan(_desc("AMINO20"), [(8192, 0)] * 19, 1024, 0, capi.F32) == (3, [1] * 19)
    # empty batches are skipped and do not count towards a group
    r, fam = _plan(_desc("AMINO20"), [(8192, 0), (0, 0)] * 8 + [(8192, 0), (8192, 0)], 1024, 0, capi.F32)
    assert r == 2 and fam[1] == 0 and fam[0] == fam[14] == fam[16] == fam[17] == 1


def test_two_pass_spills_past_the_one_piece_limit():
    # 262144 x 160 DNA4 f32: 20 MB of nibble ids each -- six fit the 128 MB of one piece, the seventh and eighth run alone
    r, fam = _plan(_desc("DNA4", True, True, True), [(262144, 0)] * 8, 160, 0, capi.F32)
    assert fam == [2] * 6 + [0, 0] and r == 2


def test_masked_two_pass_runs_alone():
    assert _plan(_desc("DNA4", True, True, True), [(131072, 1)] * 4, 160, 0, capi.F32) == (0, [0] * 4)


def test_family_agrees_with_the_single_kernel_name():
    L = _lib()
    for key, flags, B, P, t in [("AMINO20", (0, 0, 0), 8192, 1024, capi.F32), ("DNA4", (1, 1, 1), 131072, 160, capi.F32),
                                ("DNA4", (1, 1, 1), 262144, 160, capi.I8), ("DNA4", (1, 1, 1), 65536, 160, capi.I8),
                                ("DNA", (0, 0, 0), 1024, 256, capi.F32), ("AMINO20", (0, 0, 0), 2048, 512, capi.I16),
                                ("DNA5", (1, 0, 1), 16384, 512, capi.F32)]:
        d = _desc(key, *map(bool, flags))
        name = L.bsq_onehot_kernel_name(ctypes.byref(d), B, P, t).decode()
        _, fam = _plan(d, [(B, 0), (B, 0)], P, 0, t)
        if name == "k_onehot_chunks":
            want = 1
        elif name.startswith("k_tokens_pb8_fast<raw") and ("+k_expand_" in name):
            want = 2
        else:
            want = 0
        assert fam == [want, want], (key, B, P, t, name, fam)


@pytest.mark.parametrize("fn", ["plan", "run"])
def test_argument_errors(fn):
    L = _lib()
    d = _desc("DNA")
    arr = _table([(16, 0)])

    def call(n, table, layout, t):
        if fn == "plan":
            r = L.bsq_onehot_multi_plan(ctypes.byref(d), n, table, 64, layout, t, None)
            return -r if r < 0 else capi.OK
        return L.bsq_onehot_device_multi(ctypes.byref(d), n, table, 64, layout, t, None)

    assert call(-1, arr, 0, capi.F32) == capi.ERR_INVALID_ARG
    assert call(1, None, 0, capi.F32) == capi.ERR_INVALID_ARG
    assert call(1, arr, 2, capi.F32) == capi.ERR_INVALID_ARG
    assert call(1, arr, 0, 17) == capi.ERR_DTYPE
    assert call(0, None, 0, capi.F32) == capi.OK
    bad = _table([(16, 0), (-1, 0)])
    assert call(2, bad, 0, capi.F32) == capi.ERR_INVALID_ARG
    nul = _table([(16, 0), (16, 0)])
    nul[1].out = None
    assert call(2, nul, 1, capi.F32) == capi.ERR_INVALID_ARG


def test_python_surface_is_there():
    from bioseq_amd import multi
    assert callable(multi.onehot_packed_multi)
