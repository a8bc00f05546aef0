"""CPU test of the arithmetic of the bond recorder (csrc/pb_bonds.hpp): the sort network on all 8! orders of a list and
with padding, the intersection count on every pair of subset sizes, the cage vector at |c| = 2^31 - 1 and 2^31, the
overlap rule at k qa - 1, k qa and k qa + 1 and the split of the plain squares at |dq| = 2^32 - 1, against __int128
arithmetic and brute-force sets, as a stand-alone program (tests/pb_bonds_check.cpp) built plainly and under
AddressSanitizer and UBSan.  The kernels call the same functions; tests/test_gpu_bonds.py compares what they add with
tests/bonds_ref.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "particlerobotsimulations_amd", "csrc")


@pytest.mark.parametrize("flags", [["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []],
                         ids=["sanitized", "plain"])
def test_network_intersection_cage_overlap_and_plain_split_against_int128(tmp_path, flags):
    exe = tmp_path / "pb_bonds_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", *flags,
                    os.path.join(ROOT, "tests", "pb_bonds_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pb_bonds_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout
