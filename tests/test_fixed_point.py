"""CPU test of the fixed-point kit (csrc/pb_fixed.hpp): its host-callable part -- quantiser, range, split-add, composer,
normaliser -- against plain __int128 arithmetic, as a stand-alone program (tests/pb_fixed_check.cpp) built plainly and
under AddressSanitizer and UBSan.  The device part is exercised by the exact tests of the analyses built on it
(tests/test_gpu_series.py, test_gpu_timecorr.py, test_gpu_field.py, test_gpu_correlation.py, test_gpu_dynamics.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "particlerobotsimulations_amd", "csrc")


@pytest.mark.parametrize("flags", [["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []],
                         ids=["sanitized", "plain"])
def test_host_side_of_the_kit_against_int128(tmp_path, flags):
    exe = tmp_path / "pb_fixed_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", *flags,
                    os.path.join(ROOT, "tests", "pb_fixed_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pb_fixed_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout
