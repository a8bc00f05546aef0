"""CPU test of the arithmetic of the four-point recorder (csrc/pb_fourpoint.hpp): the overlap rule at and around the
radius, near 2^32 and at a radius of 0, the signed 128-bit add, and what one origin adds to a cell against __int128
arithmetic, as a stand-alone program (tests/pb_fourpoint_check.cpp) built plainly and under AddressSanitizer and UBSan.
The kernels call the same functions; tests/test_gpu_fourpoint.py compares what they add with tests/fourpoint_ref.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "particlerobotsimulations_amd", "csrc")


@pytest.mark.parametrize("flags", [["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []],
                         ids=["sanitized", "plain"])
def test_overlap_rule_128_bit_add_and_a_cell_against_int128(tmp_path, flags):
    exe = tmp_path / "pb_fourpoint_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", *flags,
                    os.path.join(ROOT, "tests", "pb_fourpoint_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pb_fourpoint_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout
