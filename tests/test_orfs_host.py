"""CPU: ORF extraction (include/bsq.h, "open reading frames") -- the declared symbols, every argument rule, the library's host twins
bsq_orf_count_host / bsq_orf_emit_host against the numpy twin (tests/orf_twin.py) exactly, on the hand-made rows and on seeded random
batches, the nucleotide spans of ORFs, the launch names, and the new host unit once under ASan / UBSan as a stand-alone program.  No
device is needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import orf_twin as twin
import translate_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -7777
RESIDUES = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYX*", dtype=np.uint8)


def _lib():
    from bioseq_amd import capi
    return capi, capi.load()


def _raw_host(chars, offs, stop, start, min_len, max_orfs=None):
    """bsq_orf_count_host + bsq_orf_emit_host into poisoned arrays with a tail past max_orfs: (row, start, length, orf_offsets,
    residues); checks that nothing at or past max_orfs was written."""
    capi, L = _lib()
    rule = capi.Orf(stop, start, min_len)
    n = offs.size - 1
    ch = chars if chars.size else np.zeros(16, np.uint8)
    orf_offs = np.full(n + 1, POISON, dtype=np.int64)
    residues = ctypes.c_int64(POISON)
    capi.check(L.bsq_orf_count_host(ch.ctypes.data, offs.ctypes.data, n, ctypes.byref(rule), orf_offs.ctypes.data, ctypes.byref(residues)))
    cap = int(orf_offs[-1]) if max_orfs is None else max_orfs
    out = [np.full(cap + 64, POISON, dtype=np.int64) for _ in range(3)]
    capi.check(L.bsq_orf_emit_host(ch.ctypes.data, offs.ctypes.data, n, ctypes.byref(rule), orf_offs.ctypes.data, cap,
                                   out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data))
    assert all((a[cap:] == POISON).all() for a in out), "an entry at or past max_orfs was written"
    return out[0][:cap], out[1][:cap], out[2][:cap], orf_offs, residues.value


def _same(got, exp, cut=None):
    """got = (row, start, length, orf_offsets, residues) against the twin's; cut: the arrays hold the first `cut` ORFs only."""
    k = exp[0].size if cut is None else min(cut, exp[0].size)
    assert np.array_equal(got[3], exp[3]) and got[4] == exp[4]
    for a, b in zip(got[:3], exp[:3]):
        assert np.array_equal(a[:k], b[:k])
        assert (a[k:] == POISON).all()


def test_new_symbols_are_declared_and_exported():
    import bioseq_amd
    capi, L = _lib()
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_orf_count_device", "bsq_orf_emit_device", "bsq_orf_count_host", "bsq_orf_emit_host", "bsq_orf_kernel_name"):
        assert n in names and hasattr(L, n)
    assert L.bsq_abi_version() == 7
    assert ctypes.sizeof(capi.Orf) == 16 and (capi.Orf.stop.offset, capi.Orf.start.offset, capi.Orf.min_len.offset) == (0, 4, 8)
    assert "orfs" in bioseq_amd.__all__
    for n in ("find_orfs_packed", "orfs_packed", "find_orfs_host", "orfs_host", "orf_spans", "kernel_name"):
        assert n in bioseq_amd.orfs.__all__ and callable(getattr(bioseq_amd.orfs, n))


def test_known_answers():
    """Rows small enough to read: the twin and the library against answers written by hand."""
    from bioseq_amd import orfs
    rows = [b"MKT*AAMAA*M", b"", b"*", b"AAAA", b"AM*MA*"]
    chars = np.frombuffer(b"".join(rows), np.uint8)
    offs = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    cases = {(1, None): [(0, 0, 3), (0, 4, 5), (0, 10, 1), (3, 0, 4), (4, 0, 2), (4, 3, 2)],
             (3, None): [(0, 0, 3), (0, 4, 5), (3, 0, 4)],
             (1, "M"): [(0, 0, 3), (0, 6, 3), (0, 10, 1), (4, 1, 1), (4, 3, 2)],
             (3, "M"): [(0, 0, 3), (0, 6, 3)],
             (4, "M"): []}
    for (ml, start), answer in cases.items():
        t = -1 if start is None else ord(start)
        e = twin.find(chars, offs, ord("*"), t, ml)
        assert list(zip(e[0].tolist(), e[1].tolist(), e[2].tolist())) == answer, (ml, start)
        g = orfs.find_orfs_host(chars, offs, min_len=ml, start=start)
        assert list(zip(g[0].tolist(), g[1].tolist(), g[2].tolist())) == answer, (ml, start)
        assert np.array_equal(g[3], e[3]) and g[3][-1] == len(answer)
        assert [twin.orfs_of_row(np.frombuffer(r, np.uint8), ord("*"), t, ml) for r in rows] == \
               [[(s, n) for r, s, n in answer if r == i] for i in range(len(rows))]


@pytest.mark.parametrize("start", [-1, ord("M")])
@pytest.mark.parametrize("min_len", [1, 5, 30])
def test_host_twins_equal_numpy_twin_on_hand_rows(min_len, start):
    chars, offs = twin.hand_rows(min_len)
    exp = twin.find(chars, offs, ord("*"), start, min_len)
    assert exp[0].size > 20
    _same(_raw_host(chars, offs, ord("*"), start, min_len), exp)
    # the batch twin is the row rule on every row
    for i in range(offs.size - 1):
        mine = twin.orfs_of_row(chars[offs[i]:offs[i + 1]], ord("*"), start, min_len)
        k0, k1 = exp[3][i], exp[3][i + 1]
        assert mine == list(zip(exp[1][k0:k1].tolist(), exp[2][k0:k1].tolist())), i


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_twins_equal_numpy_twin_on_random_batches(seed):
    rng = np.random.default_rng(seed)
    n = 400
    lens = rng.integers(0, 400, n)
    lens[rng.integers(0, n, 20)] = 0
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = rng.choice(RESIDUES, int(offs[-1])).astype(np.uint8)
    # any byte may be the stop or the start: NUL (the value of a register nobody loaded), 0xFF, a letter
    chars[rng.random(chars.size) < 0.02] = 0
    chars[rng.random(chars.size) < 0.02] = 0xFF
    for stop, start, min_len in ((ord("*"), -1, 1), (ord("*"), ord("M"), 4), (0, 0xFF, 2), (0xFF, 0, 7), (ord("A"), ord("*"), 12), (0, -1, 30)):
        exp = twin.find(chars, offs, stop, start, min_len)
        _same(_raw_host(chars, offs, stop, start, min_len), exp)
        total = exp[0].size
        if total > 2:
            mid = int(exp[3][np.nonzero(np.diff(exp[3]) > 1)[0][0]]) + 1 if (np.diff(exp[3]) > 1).any() else total // 2
            for cap in (total - 1, mid, 0):
                _same(_raw_host(chars, offs, stop, start, min_len, max_orfs=cap), exp, cut=cap)
    # no rows at all
    got = _raw_host(chars[:0], offs[:1], ord("*"), -1, 1)
    assert got[3].tolist() == [0] and got[4] == 0


def test_argument_errors_before_any_launch():
    capi, L = _lib()
    offs = np.array([0, 5, 12, 21], np.int64)
    chars = np.full(21, ord("A"), np.uint8)
    orf_offs = np.zeros(4, np.int64)
    out = [np.zeros(8, np.int64) for _ in range(3)]
    res = np.zeros(1, np.int64)
    good = capi.Orf(ord("*"), -1, 1)

    def count(fn, rule=good, ch=chars.ctypes.data, offsets=offs.ctypes.data, n=3, oo=orf_offs.ctypes.data):
        # host pointers are never touched by the device entry: every one of these calls is refused before any HIP call
        args = [ch, offsets, n, ctypes.byref(rule) if rule is not None else None, oo, res.ctypes.data]
        return fn(*args, None) if fn is L.bsq_orf_count_device else fn(*args)

    def emit(fn, rule=good, ch=chars.ctypes.data, offsets=offs.ctypes.data, n=3, oo=orf_offs.ctypes.data, cap=8, arrays=None):
        a = [x.ctypes.data for x in out] if arrays is None else arrays
        args = [ch, offsets, n, ctypes.byref(rule) if rule is not None else None, oo, cap] + a
        return fn(*args, None) if fn is L.bsq_orf_emit_device else fn(*args)

    for call, fn in ((count, L.bsq_orf_count_device), (count, L.bsq_orf_count_host), (emit, L.bsq_orf_emit_device), (emit, L.bsq_orf_emit_host)):
        assert call(fn, capi.Orf(ord("*"), -1, 0)) == capi.ERR_INVALID_ARG          # min_len < 1
        assert call(fn, capi.Orf(ord("*"), -1, -5)) == capi.ERR_INVALID_ARG
        assert call(fn, capi.Orf(ord("*"), -2, 1)) == capi.ERR_INVALID_ARG          # start outside -1 .. 255
        assert call(fn, capi.Orf(ord("*"), 256, 1)) == capi.ERR_INVALID_ARG
        assert call(fn, capi.Orf(ord("*"), ord("*"), 1)) == capi.ERR_INVALID_ARG    # start == stop
        assert call(fn, capi.Orf(0, 0, 1)) == capi.ERR_INVALID_ARG
        assert call(fn, None) == capi.ERR_INVALID_ARG                               # null pointers
        assert call(fn, ch=None) == capi.ERR_INVALID_ARG
        assert call(fn, offsets=None) == capi.ERR_INVALID_ARG
        assert call(fn, oo=None) == capi.ERR_INVALID_ARG
        assert call(fn, n=-1) == capi.ERR_INVALID_ARG                               # negative sizes
        assert b"" != L.bsq_last_error()
    for fn in (L.bsq_orf_emit_device, L.bsq_orf_emit_host):
        assert emit(fn, cap=-1) == capi.ERR_INVALID_ARG
        for k in range(3):
            arrays = [x.ctypes.data for x in out]
            arrays[k] = None
            assert emit(fn, arrays=arrays) == capi.ERR_INVALID_ARG
    # the host twins accept what the rules allow: the residue total may be NULL, the arrays may be NULL for max_orfs == 0
    assert L.bsq_orf_count_host(chars.ctypes.data, offs.ctypes.data, 3, ctypes.byref(capi.Orf(ord("*"), 255, 1)), orf_offs.ctypes.data, None) == capi.OK
    assert orf_offs.tolist() == [0, 0, 0, 0]
    assert count(L.bsq_orf_count_host) == capi.OK and orf_offs.tolist() == [0, 1, 2, 3] and res[0] == 21
    assert emit(L.bsq_orf_emit_host, cap=0, arrays=[None, None, None]) == capi.OK
    assert emit(L.bsq_orf_emit_host) == capi.OK and out[2][:3].tolist() == [5, 7, 9]


def test_python_argument_errors_touch_no_device():
    from bioseq_amd import orfs
    chars = np.frombuffer(b"MKT*AAMAA*M", np.uint8)
    offs = np.array([0, 11], np.int64)
    for fn in (orfs.find_orfs_packed, orfs.orfs_packed, orfs.find_orfs_host, orfs.orfs_host):  # (numpy arrays: the device calls would refuse them next)
        for bad in (0, -3, 2.5):
            with pytest.raises(ValueError, match="min_len"):
                fn(chars, offs, min_len=bad)
        with pytest.raises(ValueError, match="start"):
            fn(chars, offs, start="MM")
        with pytest.raises(ValueError, match="start"):
            fn(chars, offs, start=256)
        with pytest.raises(ValueError, match="differ"):
            fn(chars, offs, start="*")
        with pytest.raises(ValueError, match="differ"):
            fn(chars, offs, stop="M", start=ord("M"))
        with pytest.raises(ValueError, match="stop"):
            fn(chars, offs, stop="")
    for fn in (orfs.find_orfs_packed, orfs.orfs_packed, orfs.find_orfs_host):
        with pytest.raises(ValueError, match="max_orfs"):
            fn(chars, offs, max_orfs=-1)
    with pytest.raises(ValueError, match="capacity"):
        orfs.orfs_packed(chars, offs, capacity=-1)
    with pytest.raises(ValueError, match="resident on the device"):
        orfs.find_orfs_packed(chars, offs)  # a host batch
    with pytest.raises(ValueError, match="resident on the device"):
        orfs.orfs_packed(chars, offs)
    with pytest.raises(ValueError, match="frame"):
        orfs.orfs_host(chars, offs, frame=7)


def test_orf_spans_and_the_host_pipeline():
    """orfs_host = translate_twin + orf_twin + slicing; the reverse complement of the interval orf_spans returns for a reverse-frame
    ORF translates back to the ORF (frame code 3 of the interval), the interval of a forward one translates to it directly."""
    from bioseq_amd import orfs
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 700, 60)
    chars, offs = twin.dna_store(rng, lens)
    for frame, start, table in (("six", None, 1), ("six", "M", 2), (4, None, 1), (rng.integers(0, 6, 60).astype(np.uint8), None, 1)):
        per_row = None if isinstance(frame, (str, int)) else frame
        code = translate_twin.SIX if isinstance(frame, str) else (0 if per_row is not None else frame)
        tab = translate_twin.table(table)
        p_chars, p_offs, _ = translate_twin.translate(chars, offs, frame=code, frames=per_row, tab=tab)
        e = twin.find(p_chars, p_offs, ord("*"), -1 if start is None else ord(start), 12)
        e_chars, e_offs = twin.slices(p_chars, p_offs, e[0], e[1], e[2])
        g_chars, g_offs, (src, fc, s, n) = orfs.orfs_host(chars, offs, frame=frame, table=table, min_len=12, start=start)
        assert e[0].size > 30
        assert np.array_equal(g_offs, e_offs) and g_chars.tobytes() == e_chars.tobytes()
        assert np.array_equal(s, e[1]) and np.array_equal(n, e[2])
        if isinstance(frame, str):
            assert np.array_equal(src, e[0] // 6) and np.array_equal(fc, e[0] % 6)
        else:
            assert np.array_equal(src, e[0]) and np.array_equal(fc, per_row[e[0]] if per_row is not None else np.full(e[0].size, frame))
        a, b = orfs.orf_spans(lens[src], fc, s, n)
        assert isinstance(frame, int) or (fc.max() >= 3 and fc.min() < 3)
        for k in range(src.size):
            row = chars[offs[src[k]]:offs[src[k] + 1]]
            assert 0 <= a[k] < b[k] <= row.size and b[k] - a[k] == 3 * n[k]
            assert (int(a[k]), int(b[k])) == twin.spans(row.size, int(fc[k]), int(s[k]), int(n[k])) == orfs.orf_spans(row.size, int(fc[k]), int(s[k]), int(n[k]))
            back = translate_twin.translate_row(row[a[k]:b[k]], 3 if fc[k] >= 3 else 0, tab)
            assert back.tobytes() == g_chars[g_offs[k]:g_offs[k + 1]].tobytes(), k


def test_batch_mix_accepts_and_rejects_segments():
    """Uniform ACGT in six frames, min_len 30: a segment reaches 30 residues with probability (61 / 64)^30 = 0.24, so the twin both
    keeps and drops at least 100 segments and neither side of the filter is vacuous (tests/test_orfs_gpu.py runs the same batch)."""
    from bioseq_amd import orfs
    p_chars, p_offs = twin.batch_mix()
    accepted, rejected = twin.segments(p_chars, p_offs, ord("*"), -1, 30)
    assert accepted >= 100 and rejected >= 100
    exp = twin.find(p_chars, p_offs, ord("*"), -1, 30)
    assert exp[0].size == accepted
    _same(_raw_host(p_chars, p_offs, ord("*"), -1, 30), exp)
    got = orfs.find_orfs_host(p_chars, p_offs)  # min_len 30, '*', no start: the defaults
    assert all(np.array_equal(a, b) for a, b in zip(got, exp[:4]))


def test_kernel_name_at_the_class_boundaries():
    from bioseq_amd import orfs
    two, three = "k_orf_count+k_orf_offsets;k_orf_emit", "k_orf_count+k_orf_scan+k_orf_offsets;k_orf_emit"
    assert orfs.kernel_name(-1) == "" and orfs.kernel_name(0) == "hipMemsetAsync"
    assert orfs.kernel_name(1) == orfs.kernel_name(4097) == orfs.kernel_name(2 ** 20 - 1) == orfs.kernel_name(2 ** 20) == two
    assert orfs.kernel_name(2 ** 20 + 1) == orfs.kernel_name(2 ** 30) == three
    assert orfs.kernel_name((2 ** 31 - 1) * 64) == three and orfs.kernel_name((2 ** 31 - 1) * 64 + 1) == ""  # a grid of 2^31 - 1 workgroups of 64 rows


def test_host_unit_under_address_and_ub_sanitizers(tmp_path):
    """bsq_orf_host.cpp with g++ -fsanitize=address,undefined in a stand-alone program (tests/native/orf_host_check.cpp: its own main,
    its own plain-loop reference, exact-size heap arrays so that a write past max_orfs or a read past a row is an error)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if not shutil.which("g++") or subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")],
                                                 capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link the ASan / UBSan runtimes here")
    if not os.path.isdir("/opt/rocm/include/hip"):
        pytest.skip("no HIP headers")
    exe = str(tmp_path / "orf_host_check")
    csrc = os.path.join(ROOT, "bioseq_amd", "csrc")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        os.path.join(ROOT, "tests", "native", "orf_host_check.cpp"), os.path.join(csrc, "bsq_orf_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ORF_HOST_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-4000:]
