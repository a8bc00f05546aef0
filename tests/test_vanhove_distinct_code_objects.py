"""The code objects of csrc/pb_vanhove_distinct.hip, read as tools/summarize_profile.py prints them (no GPU needed: hipcc
cross-compiles gfx950): the k_vhd_* kernels are the ones the file names, none uses scratch memory or more than 128
VGPRs, the accumulating kernel keeps the edges, the histogram and the fold's words in LDS, and the registers are what
profiles/van_hove_distinct.txt records."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_vhd_accumulate", "k_vhd_snapshot"]  # (the lag ring zeroes the table with a memset: pb_engine.hpp)


def header_constant(name):
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    return int(re.search(r"#define %s (\d+)u" % name, header).group(1))


# PB_VANHOVE_MAX_BINS edges of 8 bytes (E_0 is not stored) and as many 32-bit counters, four waves of two 64-bit counts
LDS = header_constant("PB_VANHOVE_MAX_BINS") * (8 + 4) + 4 * 2 * 8


@pytest.fixture(scope="module")
def regs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import summarize_profile
    r = summarize_profile.code_object_registers()
    assert r, "no code objects under csrc/build: build the libraries from source (make -C particlerobotsimulations_amd/csrc)"
    return {k: tuple(int(x) for x in v) for k, v in r.items() if k.startswith("k_vhd_")}


def test_distinct_van_hove_kernels_have_no_scratch(regs):
    assert sorted(regs) == KERNELS
    assert LDS == 8192 + 4096 + 64
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_vanhove_distinct.hip")).read()
    for k, (vgpr, sgpr, lds, scratch) in regs.items():
        assert "void " + k + "(" in source, k  # the kernels the file names
        assert scratch == 0, (k, vgpr, sgpr, lds, scratch)
        assert vgpr <= 128, (k, vgpr)  # four waves per SIMD at the least
        assert lds == (LDS if k == "k_vhd_accumulate" else 0), (k, lds)


def test_registers_match_the_profile_file(regs):
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "van_hove_distinct.txt")):
        parts = line.split()
        if parts[:1] == ["reg"]:
            rec[" ".join(parts[1:-4])] = tuple(int(v) for v in parts[-4:])
    assert rec == regs  # the counts the profile file records are those of this build
