"""The code objects of csrc/pb_fourpoint.hip, read as tools/summarize_profile.py prints them (no GPU needed: hipcc
cross-compiles gfx950): the k_fp_* kernels are the ones the file names, none uses scratch memory, the mode kernel keeps
at most 64 VGPRs and the table, a tile of staged pairs and the waves' counts in LDS (the compacted form, which ships),
the folding kernel at most 128 VGPRs and no LDS, and the registers are what profiles/four_point.txt records."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_fp_fold", "k_fp_modes", "k_fp_snapshot"]  # (the record's scratch is zeroed with memsets)
# the interleaved table, 256 staged pairs of 16 bytes (qx, qy, mask, 0) and, in the compacted form, a count per wave
LDS = 4096 * 8 + 256 * 16 + 4 * 4


@pytest.fixture(scope="module")
def regs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import summarize_profile
    r = summarize_profile.code_object_registers()
    assert r, "no code objects under csrc/build: build the libraries from source (make -C particlerobotsimulations_amd/csrc)"
    return {k: tuple(int(x) for x in v) for k, v in r.items() if k.startswith("k_fp_")}


def test_four_point_kernels_have_no_scratch(regs):
    assert sorted(regs) == KERNELS
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_fourpoint.hip")).read()
    for k, (vgpr, sgpr, lds, scratch) in regs.items():
        assert "void " + k + "(" in source, k  # the kernels the file names
        assert scratch == 0, (k, vgpr, sgpr, lds, scratch)
        assert lds == (LDS if k == "k_fp_modes" else 0), (k, lds)
    assert regs["k_fp_modes"][0] <= 64   # one vector per lane and two 64-bit sums, as the scattering's accumulate kernel
    assert regs["k_fp_fold"][0] <= 128   # four waves per SIMD at the least
    assert "__shared__ int2 sTab[PB_PHASOR_STEPS]" in source and "__shared__ int4 sBot[FT]" in source
    assert "__shared__ uint32_t sWave[FT / 64]" in source and "#define PB_FOURPOINT_COMPACT 1" in source  # what ships


def test_registers_match_the_profile_file(regs):
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "four_point.txt")):
        parts = line.split()
        if parts[:1] == ["reg"]:
            rec[" ".join(parts[1:-4])] = tuple(int(v) for v in parts[-4:])
    assert rec == regs  # the counts the profile file records are those of this build
