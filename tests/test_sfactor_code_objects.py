"""The code objects of csrc/pb_sfactor.hip, read as tools/summarize_profile.py prints them (no GPU needed: hipcc
cross-compiles gfx950): the k_sk_* kernels are the ones the file names, none uses scratch memory or more than 128 VGPRs,
the accumulating kernels keep the table and a tile of bots in LDS, and the registers are what
profiles/structure_factor.txt records."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_sk_accumulate<0>", "k_sk_accumulate<1>", "k_sk_accumulate<2>", "k_sk_clear"]
LDS = 4096 * 8 + 256 * 16  # the interleaved table and 256 staged bots of 16 bytes


@pytest.fixture(scope="module")
def regs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import summarize_profile
    r = summarize_profile.code_object_registers()
    assert r, "no code objects under csrc/build: build the libraries from source (make -C particlerobotsimulations_amd/csrc)"
    return {k: tuple(int(x) for x in v) for k, v in r.items() if k.startswith("k_sk_")}


def test_sk_kernels_have_no_scratch(regs):
    assert sorted(regs) == KERNELS
    for k, (vgpr, sgpr, lds, scratch) in regs.items():
        assert scratch == 0, (k, vgpr, sgpr, lds, scratch)
        assert vgpr <= 128, (k, vgpr)  # four waves per SIMD at the least
        assert lds == (0 if k == "k_sk_clear" else LDS), (k, lds)
    # the density is its own instantiation: two accumulators and no multiply, so fewer registers than the others
    assert regs["k_sk_accumulate<0>"][0] < regs["k_sk_accumulate<1>"][0] < regs["k_sk_accumulate<2>"][0]


def test_registers_match_the_profile_file(regs):
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "structure_factor.txt")):
        parts = line.split()
        if parts[:1] == ["reg"]:
            rec[" ".join(parts[1:-4])] = tuple(int(v) for v in parts[-4:])
    assert rec == regs  # the counts the profile file records are those of this build
