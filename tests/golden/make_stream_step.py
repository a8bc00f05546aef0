"""Generates tests/golden/stream_step/yardstick.json: how far the oracle's own fp32 builds (the oracle, and the
fma / fma_powf / cuda_like bracket builds of oracle/Makefile) are from the float64 reference of one collide step
(tests/stream_ref.py), per output and per input of the streamlined kernel's per-step tests.

    python tests/golden/make_stream_step.py            # a few seconds

Nothing of the device is involved: tests/test_stream_ref.py recomputes these numbers on the CPU and holds them to
this file; tests/test_gpu_stream_step.py holds the streamlined kernel to a small multiple of them."""
import json
import os
import platform
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import orclib as orc  # noqa: E402
import stream_ref as sr  # noqa: E402


def main():
    out = {
        "generator": "tests/golden/make_stream_step.py",
        "compiler": subprocess.check_output(["gcc", "--version"], text=True).splitlines()[0],
        "libc": " ".join(platform.libc_ver()),
        "machine": platform.machine(),
        "builds": ["exact" if b is None else b for b in sr.BUILDS],
        "errors": "vel: |dv| / (dt / m) / max(|F|, Sum|F_attr| + Sum|F_rep|); fa, fr: relative to their own value; "
                  "rad: relative to max_radius; max and 99th percentile over the bots with no decision within "
                  f"{sr.DELTA_GAP} (gaps) / {sr.DELTA_REL} (hold, stop, actuation branches) of its threshold",
    }
    out.update(sr.measure_yardstick(orc))
    path = os.path.join(HERE, "stream_step", "yardstick.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
