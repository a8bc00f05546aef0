"""The code objects of csrc/pb_timecorr.hip, read as tools/summarize_profile.py prints them (no GPU needed: hipcc
cross-compiles gfx950): the k_tc_* kernels are the two the file names, none uses scratch memory or more than 128
VGPRs, the accumulating pass' LDS is its cross-wave combine (four waves of nine 8-byte columns), and the registers are
what profiles/time_correlation.txt records."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_tc_accumulate", "k_tc_snapshot"]  # (the lag ring zeroes the table with a memset: pb_engine.hpp)


@pytest.fixture(scope="module")
def regs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import summarize_profile
    r = summarize_profile.code_object_registers()
    assert r, "no code objects under csrc/build: build the libraries from source (make -C particlerobotsimulations_amd/csrc)"
    return {k: tuple(int(x) for x in v) for k, v in r.items() if k.startswith("k_tc_")}


def test_time_correlation_kernels_have_no_scratch(regs):
    assert sorted(regs) == KERNELS
    for k, (vgpr, sgpr, lds, scratch) in regs.items():
        assert scratch == 0, (k, vgpr, sgpr, lds, scratch)
        assert vgpr <= 128, (k, vgpr)  # four waves per SIMD at the least


def test_lds_is_only_the_cross_wave_combine(regs):
    assert regs["k_tc_accumulate"][2] == 4 * 9 * 8
    assert regs["k_tc_snapshot"][2] == 0


def test_registers_match_the_profile_file(regs):
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "time_correlation.txt")):
        parts = line.split()
        if parts[:1] == ["reg"]:
            rec[" ".join(parts[1:-4])] = tuple(int(v) for v in parts[-4:])
    assert rec == regs  # the counts the profile file records are those of this build
