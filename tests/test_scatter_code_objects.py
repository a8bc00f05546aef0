"""The code objects of csrc/pb_scatter.hip, read as tools/summarize_profile.py prints them (no GPU needed: hipcc
cross-compiles gfx950): the k_scat_* kernels are the ones the file names, none uses scratch memory or more than 128
VGPRs, the accumulating kernel keeps the table and a tile of staged pairs in LDS, and the registers are what
profiles/intermediate_scattering.txt records."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_scat_accumulate", "k_scat_snapshot"]  # (the lag ring zeroes the table with a memset: pb_engine.hpp)
LDS = 4096 * 8 + 256 * 16  # the interleaved table and 256 staged pairs of 16 bytes (dqx, dqy, mask, 0)


@pytest.fixture(scope="module")
def regs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import summarize_profile
    r = summarize_profile.code_object_registers()
    assert r, "no code objects under csrc/build: build the libraries from source (make -C particlerobotsimulations_amd/csrc)"
    return {k: tuple(int(x) for x in v) for k, v in r.items() if k.startswith("k_scat_")}


def test_scatter_kernels_have_no_scratch(regs):
    assert sorted(regs) == KERNELS
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_scatter.hip")).read()
    for k, (vgpr, sgpr, lds, scratch) in regs.items():
        assert "void " + k + "(" in source, k  # the kernels the file names
        assert scratch == 0, (k, vgpr, sgpr, lds, scratch)
        assert vgpr <= 128, (k, vgpr)  # four waves per SIMD at the least
        assert lds == (LDS if k == "k_scat_accumulate" else 0), (k, lds)
    # one vector per lane and two 64-bit sums: nowhere near the structure factor's split accumulators
    assert regs["k_scat_accumulate"][0] <= 64


def test_registers_match_the_profile_file(regs):
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "intermediate_scattering.txt")):
        parts = line.split()
        if parts[:1] == ["reg"]:
            rec[" ".join(parts[1:-4])] = tuple(int(v) for v in parts[-4:])
    assert rec == regs  # the counts the profile file records are those of this build
