"""The code objects of csrc/pb_structure.hip, read as tools/summarize_profile.py prints them (no GPU needed: hipcc
cross-compiles gfx950): the two sweeps use no scratch memory, the radial sweep's LDS is its 16 KB histogram and little
else, and the registers are what profiles/structure_analysis.txt records."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_struct_hexatic", "k_struct_psi6", "k_struct_rdf"]


@pytest.fixture(scope="module")
def regs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import summarize_profile
    r = summarize_profile.code_object_registers()
    assert r, "no code objects under csrc/build: build the libraries from source (make -C particlerobotsimulations_amd/csrc)"
    return {k: tuple(int(x) for x in v) for k, v in r.items() if k.startswith("k_struct_")}


def test_structure_kernels_have_no_scratch(regs):
    assert sorted(regs) == KERNELS
    for k, (vgpr, sgpr, lds, scratch) in regs.items():
        assert scratch == 0, (k, vgpr, sgpr, lds, scratch)
        assert vgpr <= 128, (k, vgpr)  # four waves per SIMD at the least


def test_radial_sweep_lds_is_the_histogram(regs):
    vgpr, sgpr, lds, scratch = regs["k_struct_rdf"]
    assert 16384 <= lds <= 16384 + 256, lds
    assert regs["k_struct_psi6"][2] <= 1024  # the row reduction's few words


def test_registers_match_the_profile_file(regs):
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "structure_analysis.txt")):
        parts = line.split()
        if parts[:1] == ["reg"]:
            rec[" ".join(parts[1:-4])] = tuple(int(v) for v in parts[-4:])
    assert rec == regs  # the counts the profile file records are those of this build
