"""particlebot_run's handling of the analysis flags, as one table: the values each flag refuses, the boundary values it
takes, and the engine check that follows the parse loop.  Every case returns from main() before a Particlebot exists:
no device is opened and nothing is written."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")

USAGE = ("usage: " + RUN + " [config.cfg] [--set NAME VALUE]... [--engine fused|legacy] [--quiet] "
         "[--frames DIR [--frame-size PIXELS] [--frame-style plain|reference] [--frame-render host|device]] "
         "[--trail FILE] [--clusters FILE [--cluster-gap G]] [--contacts FILE [--contact-gap G]] "
         "[--structure FILE [--structure-gap G]] [--rdf FILE [--rdf-rmax R] [--rdf-bins B]] "
         "[--rearrange FILE [--rearrange-gap G] [--rearrange-window]] [--resume FILE [--overwrite-csv]] "
         "[--checkpoint FILE [--checkpoint-every SECONDS] [--checkpoint-steps N]] [--final-checkpoint FILE]\n")

NOT_A_GAP = ["", "abc", "-1", "-1e-30", "nan", "inf", "-inf", "0.1x"]
GAP_FLAGS = ["--cluster-gap", "--contact-gap", "--structure-gap", "--rearrange-gap"]
BAD = ([(flag, v) for flag in GAP_FLAGS for v in NOT_A_GAP]
       + [("--rdf-rmax", v) for v in NOT_A_GAP + ["0"]]
       + [("--rdf-bins", v) for v in ("0", "4097", "-3", "1.5", "")])

# (the value flag, a value on the edge of what it takes, its file flag, what the engine check then says)
GOOD = [
    ("--cluster-gap", "0", "--clusters",
     "--clusters needs the fused engine (the analysis runs on its resident state)\n"),
    ("--cluster-gap", "3.4e38", "--clusters",
     "--clusters needs the fused engine (the analysis runs on its resident state)\n"),
    ("--contact-gap", "0", "--contacts",
     "--contacts needs the fused engine (the export runs on its resident state)\n"),
    ("--contact-gap", "3.4e38", "--contacts",
     "--contacts needs the fused engine (the export runs on its resident state)\n"),
    ("--structure-gap", "0", "--structure",
     "--structure needs the fused engine (the analysis runs on its resident state)\n"),
    ("--structure-gap", "3.4e38", "--structure",
     "--structure needs the fused engine (the analysis runs on its resident state)\n"),
    ("--rearrange-gap", "0", "--rearrange",
     "--rearrange needs the fused engine (the analysis runs on its resident state)\n"),
    ("--rearrange-gap", "3.4e38", "--rearrange",
     "--rearrange needs the fused engine (the analysis runs on its resident state)\n"),
    ("--rdf-rmax", "1e-30", "--rdf", "--rdf needs the fused engine (the analysis runs on its resident state)\n"),
    ("--rdf-bins", "1", "--rdf", "--rdf needs the fused engine (the analysis runs on its resident state)\n"),
    ("--rdf-bins", "4096", "--rdf", "--rdf needs the fused engine (the analysis runs on its resident state)\n"),
]

TAKES_A_VALUE = ["--clusters", "--cluster-gap", "--contacts", "--contact-gap", "--structure", "--structure-gap", "--rdf",
                 "--rdf-rmax", "--rdf-bins", "--rearrange", "--rearrange-gap"]


def run(args, cwd):
    return subprocess.run([RUN] + args, capture_output=True, text=True, timeout=60, cwd=cwd)


@pytest.mark.parametrize("flag,value", BAD, ids=[f"{f}={v!r}" for f, v in BAD])
def test_a_bad_value_is_a_usage_error(tmp_path, flag, value):
    for args in ([flag, value], [CFG, flag, value, "--quiet"]):
        r = run(args, tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), args
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("flag,value,file_flag,said", GOOD, ids=[f"{f}={v}" for f, v, _, _ in GOOD])
def test_a_boundary_value_passes_and_the_engine_check_stops_the_run(tmp_path, flag, value, file_flag, said):
    r = run([CFG, "--engine", "legacy", file_flag, "a.csv", flag, value], tmp_path)
    assert (r.returncode, r.stdout, r.stderr) == (2, "", said)
    assert not os.listdir(tmp_path)


def test_the_engine_check_names_the_first_file_flag_in_its_own_order(tmp_path):
    files = ["--rearrange", "e.csv", "--rdf", "d.csv", "--structure", "c.csv", "--contacts", "b.csv", "--clusters",
             "a.csv"]
    said = [
        "--rearrange needs the fused engine (the analysis runs on its resident state)\n",
        "--rdf needs the fused engine (the analysis runs on its resident state)\n",
        "--structure needs the fused engine (the analysis runs on its resident state)\n",
        "--contacts needs the fused engine (the export runs on its resident state)\n",
        "--clusters needs the fused engine (the analysis runs on its resident state)\n",
    ]
    for k in range(5):  # k = 4: all five given, --clusters speaks; k = 0: --rearrange alone
        r = run([CFG, "--engine", "legacy"] + files[:2 * (k + 1)], tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", said[k])
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("flag", TAKES_A_VALUE)
def test_a_flag_without_its_value_is_a_usage_error(tmp_path, flag):
    r = run([CFG, flag], tmp_path)
    assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE)
    assert not os.listdir(tmp_path)
