"""CPU: the library's twin of the BPE training (bsq_bpe_train_host, through bioseq_amd.bpe.bpe_train_packed on numpy arrays) against the
header's known answers and, byte for byte in merges and winning counts, against the numpy rule `bpe_train_host`: DNA4 and AMINO20 samples
with and without unmapped bytes, a many-ties sample whose stop comes early, n_merges = 0, empty rows and B = 0, tokenizer flags, rows above
max_chars, the struct's size and the refusals of the C ABI, and the vocabulary's way into the tokenizer.  A stand-alone program
(tests/native/bpe_train_host_check.cpp) runs the twin once under ASan / UBSan."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import bpe_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMINO = "ACDEFGHIKLMNPQRSTVWY"
KNOWN = [([b"AAAAAAA"], [(0, 0)], [3]),
         ([b"ACGACGACG", b"CGCG"], [(1, 2), (0, 4)], [5, 3]),
         ([b"ACAC", b"GTGT"], [(0, 1), (2, 3)], [2, 2]),
         ([b"ACACAC", b"ACACAC"], [(0, 1), (4, 4), (5, 4)], [6, 2, 2]),
         ([b"AAAAANAAAA"], [(0, 0), (4, 4)], [4, 2]),
         ([b"ACGTNACGT"], [(0, 1), (2, 3), (4, 5)], [2, 2, 2]),
         ([b"AC", b"AC"], [(0, 1)], [2]),
         ([b"A" * 8192], [(0, 0)] + [(k, k) for k in range(4, 15)], [4096 >> k for k in range(12)])]


def _tok(key="DNA4", eos=False, bos=False, padchar=False):
    import bioseq_amd
    return bioseq_amd.Tokenizer(key, eos, bos, padchar)


def _numpy_counts(tok, chars, offs, merges):
    """The winning count of every merge by a plain programme of its own: rows as lists, the pairs of a row walked left to right, a pair
    of equal symbols skipped when the pair in front of it was the same pair and counted."""
    from bioseq_amd import capi
    lut = np.frombuffer(bytes(capi.desc_of(tok).lut), dtype=np.int8)
    C = capi.desc_of(tok).nchars
    rows = [[int(lut[b]) for b in bytes(chars[offs[i]:offs[i + 1]])] for i in range(len(offs) - 1)]
    out = []
    for m, (l, r) in enumerate(merges):
        count = 0
        for k, row in enumerate(rows):
            new, q, took = [], 0, 0
            while q < len(row):
                if q + 1 < len(row) and row[q] == l and row[q + 1] == r:
                    new.append(C + m)
                    q += 2
                    took += 1
                else:
                    new.append(row[q])
                    q += 1
            rows[k] = new
            count += took
        out.append(count)
    return out


def _both(tok, rows, n_merges, **kw):
    """The twin's (merges, counts) after comparing them with the numpy rule's merges and the plain programme's counts."""
    from bioseq_amd import bpe
    chars, offs = twin.pack(rows)
    v, info = bpe.bpe_train_packed(tok, chars, offs, n_merges, return_info=True, **kw)
    ref = bpe.bpe_train_host(tok, chars, offs, n_merges)
    assert v.merges.dtype == ref.merges.dtype and v.merges.tobytes() == ref.merges.tobytes(), (v.merges[:6].tolist(), ref.merges[:6].tolist())
    assert info["counts"].dtype == np.int64 and info["counts"].tolist() == _numpy_counts(tok, chars, offs, ref.merges.tolist())
    return v.merges.tolist(), info["counts"].tolist(), info


def test_known_answers():
    for rows, merges, counts in KNOWN:
        got_m, got_c, info = _both(_tok(), rows, 40)
        assert got_m == [list(m) for m in merges] and got_c == counts, (rows[0][:12], got_m, got_c)
        assert info["skipped_rows"] == 0 and info["kernel"] == "bsq_bpe_train_host"


@pytest.mark.parametrize("key,letters", [("DNA4", "ACGT"), ("AMINO20", AMINO)])
@pytest.mark.parametrize("unmapped", [0.0, 0.03])
def test_twin_against_the_numpy_rule(key, letters, unmapped):
    """About 60 rows of up to 300 characters at 200 merges, random and low-complexity, seeded."""
    rng = np.random.default_rng(len(letters) + int(unmapped * 100))
    rows = [twin.random_row(rng, int(rng.integers(0, 301)), letters, unmapped) for _ in range(40)]
    rows += [twin.low_complexity_row(rng, int(rng.integers(1, 301)), letters) for _ in range(20)]
    got_m, got_c, _ = _both(_tok(key), rows, 200)
    assert len(got_m) == 200 and got_c[-1] >= 2


def test_many_ties_and_the_early_stop():
    """30 rows of 40 characters asked for 100 merges: counts of 2 and 3 tie constantly and the stop is reached early."""
    rng = np.random.default_rng(5)
    rows = [twin.random_row(rng, 40, "ACGT") for _ in range(30)]
    got_m, got_c, _ = _both(_tok(), rows, 100)
    assert 0 < len(got_m) < 100 and got_c[-1] >= 2 and got_c.count(2) + got_c.count(3) > len(got_c) // 2


def test_no_merges_empty_rows_and_no_rows():
    from bioseq_amd import bpe
    assert _both(_tok(), [b"ACACAC"], 0)[0] == []
    assert _both(_tok(), [b"", b"", b""], 10)[0] == [] and _both(_tok(), [b"", b"ACAC", b""], 10)[0] == [[0, 1]]
    assert _both(_tok(), [b"A", b"C", b"N"], 10)[0] == []
    v, info = bpe.bpe_train_packed(_tok(), np.zeros(0, np.uint8), np.zeros(1, np.int64), 10, return_info=True)
    assert v.M == 0 and info["counts"].shape == (0,) and info["skipped_rows"] == 0


def test_tokenizer_flags_do_not_change_the_merges():
    rng = np.random.default_rng(3)
    rows = twin.fuzz_rows(rng, "ACGT", 40)
    base = _both(_tok(), rows, 80)
    for flags in ((True, False, False), (False, True, False), (True, True, True)):
        got = _both(_tok("DNA4", *flags), rows, 80)
        assert got[0] == base[0] and got[1] == base[1]


def test_rows_above_max_chars_are_skipped_and_counted():
    from bioseq_amd import bpe
    rng = np.random.default_rng(4)
    rows = [twin.random_row(rng, int(rng.integers(0, 130)), "ACGT", 0.02) for _ in range(60)]
    short = [r for r in rows if len(r) <= 64]
    v, info = bpe.bpe_train_packed(_tok(), *twin.pack(rows), 60, max_chars=64, return_info=True)
    assert info["skipped_rows"] == len(rows) - len(short) > 0
    assert v.merges.tolist() == _both(_tok(), short, 60)[0]
    with pytest.raises(ValueError, match="crop_packed"):  # max_chars=None: the longest row is looked at, and 8193 is refused
        bpe.bpe_train_packed(_tok(), *twin.pack([b"A" * 8193]), 4)
    v, info = bpe.bpe_train_packed(_tok(), *twin.pack([b"A" * 8193, b"ACAC"]), 4, max_chars=8192, return_info=True)
    assert info["skipped_rows"] == 1 and v.merges.tolist() == [[0, 1]]


def test_struct_size_symbols_and_refusals():
    from bioseq_amd import bpe, capi
    lib = capi.load()
    assert ctypes.sizeof(capi.BpeTrain) == 24 and capi.BpeTrain.table_slots.offset == 16
    names = capi.declared_symbols(capi.HEADER_PATH)
    for n in ("bsq_bpe_train_workspace_bytes", "bsq_bpe_train_table_slots", "bsq_bpe_train_lds_slots", "bsq_bpe_train_begin_device",
              "bsq_bpe_train_steps_device", "bsq_bpe_train_host", "bsq_bpe_train_kernel_name"):
        assert n in names and hasattr(lib, n), n
    assert lib.bsq_abi_version() == 7
    d = capi.desc_of(_tok())
    chars, offs = twin.pack([b"ACACAC", b"ACAC"])
    merges, counts = np.full((4, 2), -7, np.int32), np.full(4, -7, np.int64)
    made, skipped = ctypes.c_int64(-7), ctypes.c_int64(-7)

    def call(cfg, d=ctypes.byref(d), chars=chars.ctypes.data, offs=offs.ctypes.data, B=2, total=chars.size, merges=merges.ctypes.data, made=ctypes.byref(made)):
        return lib.bsq_bpe_train_host(d, chars, offs, B, total, cfg, merges, counts.ctypes.data, made, ctypes.byref(skipped))

    ok = capi.BpeTrain(8192, 0, 4, 0, 0)
    for bad in (capi.BpeTrain(0, 0, 4, 0, 0), capi.BpeTrain(8193, 0, 4, 0, 0), capi.BpeTrain(8192, 0, 4, 1, 0), capi.BpeTrain(8192, 3, 4, 0, 0),
                capi.BpeTrain(2048, 1, 4, 0, 0), capi.BpeTrain(8192, 0, -1, 0, 0), capi.BpeTrain(8192, 0, 4, 0, 8), capi.BpeTrain(8192, 0, 4, 0, 48),
                capi.BpeTrain(8192, 0, 4, 0, 1 << 29)):
        assert call(ctypes.byref(bad)) == capi.ERR_INVALID_ARG and lib.bsq_last_error()
        assert lib.bsq_bpe_train_workspace_bytes(ctypes.byref(d), 2, chars.size, ctypes.byref(bad)) == -capi.ERR_INVALID_ARG
    for kw in (dict(cfg=None), dict(d=None), dict(chars=None), dict(offs=None), dict(merges=None), dict(made=None), dict(B=-1), dict(total=-1),
               dict(total=1 << 31)):
        assert call(**{"cfg": ctypes.byref(ok), **kw}) == capi.ERR_INVALID_ARG, kw
    assert (merges == -7).all() and (counts == -7).all() and made.value == skipped.value == -7, "a refusal writes nothing"
    assert call(ctypes.byref(ok)) == capi.OK and made.value == 2 and merges[:2].tolist() == [[0, 1], [4, 4]] and counts[:2].tolist() == [5, 2]
    # the workspace: 16 + 8 n bytes of head, 4 B of lengths and 2 total of symbols (each rounded up to 8), 8 bytes per slot
    assert lib.bsq_bpe_train_table_slots(ctypes.byref(d), 2, chars.size, ctypes.byref(ok)) == 1024
    assert lib.bsq_bpe_train_workspace_bytes(ctypes.byref(d), 2, chars.size, ctypes.byref(ok)) == 16 + 8 * 4 + 8 + 24 + 8 * 1024
    big = capi.BpeTrain(8192, 0, 70000, 0, 0)  # n_merges is cut at 65536 - 4 - C, the table at 2^28 slots
    assert lib.bsq_bpe_train_table_slots(ctypes.byref(d), 1 << 20, (1 << 31) - 1, ctypes.byref(big)) == 1 << 28
    assert lib.bsq_bpe_train_workspace_bytes(ctypes.byref(d), 0, 0, ctypes.byref(big)) == 16 + 8 * (65536 - 4 - 4) + 8 * 1024
    assert lib.bsq_bpe_train_kernel_name(ctypes.byref(ok)) == b"k_bpe_train_pass<block>" and lib.bsq_bpe_train_kernel_name(ctypes.byref(capi.BpeTrain(0, 0, 4, 0, 0))) == b""
    assert bpe.bpe_train_kernel_name(1024) == "k_bpe_train_pass<wave>" and bpe.bpe_train_kernel_name(1024, 2) == "k_bpe_train_pass<block>"
    assert bpe.bpe_train_kernel_name() == "k_bpe_train_pass<block>" and lib.bsq_bpe_train_lds_slots() == 2048
    for kw in (dict(max_chars=0), dict(max_chars=8193), dict(max_chars=2048, form=1), dict(form=3), dict(table_slots=48), dict(steps_per_call=0)):
        with pytest.raises(ValueError):
            bpe.bpe_train_packed(_tok(), chars, offs, 4, **kw)
    with pytest.raises(ValueError):
        bpe.bpe_train_kernel_name(2048, 1)
    assert "bpe_train_packed" in bpe.__all__ and "bpe_train_kernel_name" in bpe.__all__ and "bpe_train_packed" in bpe.__doc__


def test_the_vocabulary_goes_into_the_tokenizer_and_the_inputs_stay():
    from bioseq_amd import bpe
    rng = np.random.default_rng(2)
    rows = twin.fuzz_rows(rng, "ACGT", 30)
    chars, offs = twin.pack(rows)
    c0, o0 = chars.copy(), offs.copy()
    v = bpe.bpe_train_packed(_tok(), chars, offs, 50)
    assert isinstance(v, bpe.BPEVocab) and v.M == 50 and chars.tobytes() == c0.tobytes() and offs.tobytes() == o0.tobytes()
    tokens, lengths = bpe.bpe_tokenize_host(v, chars, offs, 160, "i")
    lut = np.frombuffer(bytes(v.desc.lut), dtype=np.int8)
    for b, row in enumerate(rows):
        assert tokens[b, :lengths[b]].tolist() == twin.row_ids(lut, 4, v.merges, row)


def test_host_unit_under_address_and_ub_sanitizers(tmp_path):
    """Exact-size heap arrays: a read past the characters or the offsets, or a write past merges or counts, is an error; the program's
    own one-row-at-a-time programme checks the answers.  Host code only: nothing is loaded into Python, no device is needed."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if not shutil.which("g++") or subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")],
                                                 capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link the ASan / UBSan runtimes here")
    exe = str(tmp_path / "bpe_train_host_check")
    csrc = os.path.join(ROOT, "bioseq_amd", "csrc")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        os.path.join(ROOT, "tests", "native", "bpe_train_host_check.cpp"), os.path.join(csrc, "bsq_bpe_train_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "BPE_TRAIN_HOST_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-4000:]
