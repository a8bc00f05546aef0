"""CPU tests of the engine's memory owners (csrc/pb_memory.hpp): PbOwned with a malloc-backed counting trait, as a
stand-alone program (tests/pb_memory_check.cpp) under AddressSanitizer and UBSan, and the live-allocation counter's
entry point.  The GPU side -- nothing leaks on the device -- is tests/test_gpu_memory.py."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "particlerobotsimulations_amd", "csrc")


@pytest.mark.parametrize("flags", [["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []],
                         ids=["sanitized", "plain"])
def test_owner_with_a_counting_heap_trait(tmp_path, flags):
    exe = tmp_path / "pb_memory_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{CSRC}", *flags,
                    os.path.join(ROOT, "tests", "pb_memory_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pb_memory_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout


def test_live_counter_entry_point_takes_null_pointers():
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    buffers, nbytes = C.c_ulonglong(1 << 60), C.c_ulonglong(1 << 60)
    assert L.pbDeviceMemoryLive(C.byref(buffers), C.byref(nbytes)) == 0
    assert buffers.value < (1 << 40) and nbytes.value < (1 << 50)
    assert (buffers.value == 0) == (nbytes.value == 0)
    assert L.pbDeviceMemoryLive(None, C.byref(nbytes)) == 0 and L.pbDeviceMemoryLive(C.byref(buffers), None) == 0
    assert L.pbDeviceMemoryLive(None, None) == 0
