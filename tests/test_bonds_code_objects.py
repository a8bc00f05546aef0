"""The code objects of csrc/pb_bonds.hip, read as tools/summarize_profile.py prints them (no GPU needed: hipcc
cross-compiles gfx950): the k_bond_* kernels are the ones the file names, none uses scratch memory (a list is eight
named registers, never an indexed array), only the pairing kernel uses LDS, the 336 bytes of the workgroup's copy of a
cell that the source states, both keep at most 64 VGPRs, and the registers are what profiles/bond_dynamics.txt records."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_bond_pairs", "k_bond_snapshot"]
LDS = 42 * 8  # PB_BOND_WORDS 64-bit words


@pytest.fixture(scope="module")
def regs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import summarize_profile
    r = summarize_profile.code_object_registers()
    assert r, "no code objects under csrc/build: build the libraries from source (make -C particlerobotsimulations_amd/csrc)"
    return {k: tuple(int(x) for x in v) for k, v in r.items() if k.startswith("k_bond_")}


def test_bond_kernels_have_no_scratch(regs):
    assert sorted(regs) == KERNELS
    csrc = os.path.join(ROOT, "particlerobotsimulations_amd", "csrc")
    source = open(os.path.join(csrc, "pb_bonds.hip")).read()
    for k, (vgpr, sgpr, lds, scratch) in regs.items():
        assert "void " + k + "(" in source, k  # the kernels the file names
        assert scratch == 0, (k, vgpr, sgpr, lds, scratch)
        assert lds == (LDS if k == "k_bond_pairs" else 0), (k, lds)
        assert vgpr <= 64, (k, vgpr)  # eight waves per SIMD: the pairing kernel hides its gathers behind other waves
    assert "__shared__ unsigned long long sCell[PB_BOND_WORDS]" in source and source.count("__shared__") == 1
    assert "static_assert(PB_BOND_WORDS == 42" in open(os.path.join(csrc, "pb_bonds.hpp")).read()


def test_registers_match_the_profile_file(regs):
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "bond_dynamics.txt")):
        parts = line.split()
        if parts[:1] == ["reg"]:
            rec[" ".join(parts[1:-4])] = tuple(int(v) for v in parts[-4:])
    assert rec == regs  # the counts the profile file records are those of this build
