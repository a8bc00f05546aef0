"""The code objects of csrc/pb_strain.hip, read as tools/summarize_profile.py prints them (no GPU needed: hipcc
cross-compiles gfx950): the kernels are the ones the source names, none uses scratch memory or more than 128 VGPRs, the
fit kernel's LDS is its row reduction's few words, and the registers are what profiles/strain_analysis.txt records."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_strain_fit"]


@pytest.fixture(scope="module")
def regs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import summarize_profile
    r = summarize_profile.code_object_registers()
    assert r, "no code objects under csrc/build: build the libraries from source (make -C particlerobotsimulations_amd/csrc)"
    return {k: tuple(int(x) for x in v) for k, v in r.items() if k.startswith("k_strain_")}


def test_the_kernels_are_the_ones_the_source_names(regs):
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_strain.hip")).read()
    named = sorted(set(re.findall(r"__global__[^\n]*\bvoid (k_\w+)\(", source)))
    assert named == KERNELS == sorted(regs)
    # the scatter pass is the mark's own kernel, shared and not copied
    assert "pbDynamicsScatter(" in source and "k_dyn_scatter(" not in source.replace("//   k_dyn_scatter", "")


def test_strain_kernels_have_no_scratch(regs):
    for k, (vgpr, sgpr, lds, scratch) in regs.items():
        assert scratch == 0, (k, vgpr, sgpr, lds, scratch)
        assert vgpr <= 128, (k, vgpr)  # four waves per SIMD at the least


def test_fit_kernel_lds_is_the_row_reduction(regs):
    assert regs["k_strain_fit"][2] == 4 * 24 * 8  # four waves, 24 columns of 8 bytes


def test_registers_match_the_profile_file(regs):
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "strain_analysis.txt")):
        parts = line.split()
        if parts[:1] == ["reg"]:
            rec[" ".join(parts[1:-4])] = tuple(int(v) for v in parts[-4:])
    assert rec == regs  # the counts the profile file records are those of this build
