"""CPU: the host twins of the LSH candidates (bsq_lsh_keys_host, bsq_sketch_compare_list_host, bsq_lsh_pairs_host; bsq_lsh_host.cpp) once
under ASan / UBSan, as a stand-alone program with its own main (tests/native/lsh_host_check.cpp).  Host code only: nothing is loaded
into Python, no device is needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_unit_under_address_and_ub_sanitizers(tmp_path):
    """Exact-size heap arrays: a read past a sketch row or the list, a row looked up from an index out of range (junk entries at both
    ends of int64 in the list compare), or a write past the keys, the offsets or the pair arrays is an error; the program's own
    reference (every pair of rows tested for a shared band key, no sort) checks the answers."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if not shutil.which("g++") or subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")],
                                                 capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link the ASan / UBSan runtimes here")
    exe = str(tmp_path / "lsh_host_check")
    csrc = os.path.join(ROOT, "bioseq_amd", "csrc")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        os.path.join(ROOT, "tests", "native", "lsh_host_check.cpp"), os.path.join(csrc, "bsq_lsh_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "LSH_HOST_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-4000:]
