"""The code objects of csrc/pb_coherent.hip, read as tools/summarize_profile.py prints them (no GPU needed: hipcc
cross-compiles gfx950): the k_coh_* kernels are the ones the file names, none uses scratch memory or more than 128
VGPRs, the mode kernel keeps the table and a tile of staged bots in LDS and the correlating kernel none, and the
registers are what profiles/coherent_scattering.txt records."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_coh_correlate", "k_coh_modes"]  # (the slot's modes and counts are zeroed with memsets)
LDS = 4096 * 8 + 256 * 16  # the interleaved table and 256 staged bots of 16 bytes (qx, qy, mask, 0)


@pytest.fixture(scope="module")
def regs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import summarize_profile
    r = summarize_profile.code_object_registers()
    assert r, "no code objects under csrc/build: build the libraries from source (make -C particlerobotsimulations_amd/csrc)"
    return {k: tuple(int(x) for x in v) for k, v in r.items() if k.startswith("k_coh_")}


def test_coherent_kernels_have_no_scratch(regs):
    assert sorted(regs) == KERNELS
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_coherent.hip")).read()
    for k, (vgpr, sgpr, lds, scratch) in regs.items():
        assert "void " + k + "(" in source, k  # the kernels the file names
        assert scratch == 0, (k, vgpr, sgpr, lds, scratch)
        assert vgpr <= 128, (k, vgpr)  # four waves per SIMD at the least
        assert lds == (LDS if k == "k_coh_modes" else 0), (k, lds)
    # one vector per lane and two 64-bit sums, as the scattering's accumulate kernel
    assert regs["k_coh_modes"][0] <= 64


def test_registers_match_the_profile_file(regs):
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "coherent_scattering.txt")):
        parts = line.split()
        if parts[:1] == ["reg"]:
            rec[" ".join(parts[1:-4])] = tuple(int(v) for v in parts[-4:])
    assert rec == regs  # the counts the profile file records are those of this build
