"""CPU: the host twin of the span-corruption batches (bsq_span_corrupt_host, bsq_span_host.cpp) once under ASan / UBSan, as a
stand-alone program with its own main (tests/native/span_corrupt_host_check.cpp).  Host code only: nothing is loaded into Python, no
device is needed.  The draw's headers take their qualifiers from the HIP runtime's header, so the ROCm include path is on the command
line."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_unit_under_address_and_ub_sanitizers(tmp_path):
    """Exact-size heap arrays: a read past the characters or the offsets, or a write past inputs, labels or the length arrays, is an
    error; the program's own loop over a row's positions checks the answers, rows of several tiles included."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if not shutil.which("g++") or subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")],
                                                 capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link the ASan / UBSan runtimes here")
    if not os.path.isdir("/opt/rocm/include/hip"):
        pytest.skip("no HIP headers")
    exe = str(tmp_path / "span_corrupt_host_check")
    csrc = os.path.join(ROOT, "bioseq_amd", "csrc")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        os.path.join(ROOT, "tests", "native", "span_corrupt_host_check.cpp"), os.path.join(csrc, "bsq_span_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SPAN_CORRUPT_HOST_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-4000:]
