"""The code objects of csrc/pb_dynamics.hip, read as tools/summarize_profile.py prints them (no GPU needed: hipcc
cross-compiles gfx950): no kernel uses scratch memory or more than 128 VGPRs, the compare sweep's LDS is its row
reduction's few words, and the registers are what profiles/dynamics_analysis.txt records."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_dyn_compare", "k_dyn_count", "k_dyn_fill", "k_dyn_order", "k_dyn_scatter"]


@pytest.fixture(scope="module")
def regs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import summarize_profile
    r = summarize_profile.code_object_registers()
    assert r, "no code objects under csrc/build: build the libraries from source (make -C particlerobotsimulations_amd/csrc)"
    return {k: tuple(int(x) for x in v) for k, v in r.items() if k.startswith("k_dyn_")}


def test_dynamics_kernels_have_no_scratch(regs):
    assert sorted(regs) == KERNELS
    for k, (vgpr, sgpr, lds, scratch) in regs.items():
        assert scratch == 0, (k, vgpr, sgpr, lds, scratch)
        assert vgpr <= 128, (k, vgpr)  # four waves per SIMD at the least


def test_compare_sweep_lds_is_the_row_reduction(regs):
    assert regs["k_dyn_compare"][2] <= 1024
    for k in KERNELS:
        if k != "k_dyn_compare":
            assert regs[k][2] == 0, k


def test_registers_match_the_profile_file(regs):
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "dynamics_analysis.txt")):
        parts = line.split()
        if parts[:1] == ["reg"]:
            rec[" ".join(parts[1:-4])] = tuple(int(v) for v in parts[-4:])
    assert rec == regs  # the counts the profile file records are those of this build
