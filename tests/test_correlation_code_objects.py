"""The code objects of csrc/pb_correlate.hip, read as tools/summarize_profile.py prints them (no GPU needed: hipcc
cross-compiles gfx950): the two kernels use no scratch memory, the sweep's LDS stays within its 40 KB table (which is
sized at the launch, 40 bytes per bin, so the code object itself records none), and the registers are what
profiles/pair_correlation.txt records."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_corr_gather", "k_corr_sweep"]


@pytest.fixture(scope="module")
def regs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import summarize_profile
    r = summarize_profile.code_object_registers()
    assert r, "no code objects under csrc/build: build the libraries from source (make -C particlerobotsimulations_amd/csrc)"
    return {k: tuple(int(x) for x in v) for k, v in r.items() if k.startswith("k_corr_")}


def test_correlation_kernels_have_no_scratch(regs):
    assert sorted(regs) == KERNELS
    for k, (vgpr, sgpr, lds, scratch) in regs.items():
        assert scratch == 0, (k, vgpr, sgpr, lds, scratch)
        assert vgpr <= 128, (k, vgpr)  # four waves per SIMD at the least


def test_sweep_lds_is_at_most_the_table(regs):
    vgpr, sgpr, lds, scratch = regs["k_corr_sweep"]
    assert lds <= 40960 + 256, lds
    assert regs["k_corr_gather"][2] <= 1024  # the totals' few words


def test_registers_match_the_profile_file(regs):
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "pair_correlation.txt")):
        parts = line.split()
        if parts[:1] == ["reg"]:
            rec[" ".join(parts[1:-4])] = tuple(int(v) for v in parts[-4:])
    assert rec == regs  # the counts the profile file records are those of this build
