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
       + [("--rdf-bins", v) for v in ("0", "4097", "-3", "1.5", "", " 7x")]
       + [("--series-interval", v) for v in ("-1", "nan")]
       + [("--series-capacity", v) for v in ("0", "1048577")]
       + [("--correlate-kind", "displacement"), ("--correlate-rmax", "0")]
       + [("--correlate-bins", v) for v in ("0", "1025")]
       + [("--timecorr-interval", "-1")]
       + [("--timecorr-lags", v) for v in ("0", "65")]
       + [("--timecorr-overlap", v) for v in ("-1", "2048")]
       + [("--field-cells", v) for v in ("0", "1025")]
       + [("--field-half", "0"), ("--sk-kind", "x")]
       + [("--sk-box-log2", v) for v in ("-9", "13")]
       + [("--sk-nmax", v) for v in ("0", "45")]
       + [("--scatter-interval", "inf"), ("--scatter-lags", "65"), ("--scatter-box-log2", "13")]
       + [("--scatter-nmax", v) for v in ("0", "11")]
       + [("--frame-style", "bogus"), ("--frame-render", "gpu")])

# the file flags in the engine check's order, each with the noun its line uses
ENGINE_ORDER = [("--clusters", "analysis"), ("--contacts", "export"), ("--structure", "analysis"), ("--rdf", "analysis"),
                ("--rearrange", "analysis"), ("--series", "recorder"), ("--correlate", "analysis"),
                ("--timecorr", "recorder"), ("--field", "analysis"), ("--sk", "analysis"), ("--scatter", "recorder")]


def engine_line(file_flag):
    return f"{file_flag} needs the fused engine (the {dict(ENGINE_ORDER)[file_flag]} runs on its resident state)\n"


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
] + [(flag, value, file_flag, engine_line(file_flag)) for file_flag, flag, values in [
    ("--rdf", "--rdf-bins", [" +7"]),
    ("--series", "--series-interval", ["0"]),
    ("--series", "--series-capacity", ["1", "1048576"]),
    ("--correlate", "--correlate-kind", ["radius"]),
    ("--correlate", "--correlate-bins", ["1024"]),
    ("--correlate", "--correlate-rmax", ["1e-30"]),
    ("--timecorr", "--timecorr-lags", ["64"]),
    ("--timecorr", "--timecorr-overlap", ["0", "2047.9999"]),
    ("--field", "--field-cells", ["1024"]),
    ("--field", "--field-half", ["1e-30"]),
    ("--sk", "--sk-box-log2", ["-8", "12"]),
    ("--sk", "--sk-nmax", ["44"]),
    ("--scatter", "--scatter-interval", ["0"]),
    ("--scatter", "--scatter-lags", ["64"]),
    ("--scatter", "--scatter-box-log2", ["-8"]),
    ("--scatter", "--scatter-nmax", ["10"]),
] for value in values]

TAKES_A_VALUE = ["--clusters", "--cluster-gap", "--contacts", "--contact-gap", "--structure", "--structure-gap", "--rdf",
                 "--rdf-rmax", "--rdf-bins", "--rearrange", "--rearrange-gap", "--series", "--series-interval",
                 "--series-capacity", "--correlate", "--correlate-kind", "--correlate-rmax", "--correlate-bins", "--timecorr",
                 "--timecorr-interval", "--timecorr-lags", "--timecorr-overlap", "--field", "--field-cells", "--field-half",
                 "--sk", "--sk-kind", "--sk-box-log2", "--sk-nmax", "--scatter", "--scatter-interval", "--scatter-lags",
                 "--scatter-box-log2", "--scatter-nmax", "--frame-style", "--frame-render"]


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
    given = []
    for file_flag, _ in reversed(ENGINE_ORDER):  # --scatter alone first; at the end all eleven, and --clusters speaks
        given += [file_flag, "a.csv"]
        r = run([CFG, "--engine", "legacy"] + given, tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", engine_line(file_flag)), given
    assert not os.listdir(tmp_path)


def test_an_unknown_flag_is_a_usage_error(tmp_path):
    r = run([CFG, "--bogus"], tmp_path)
    assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE)
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("flag", TAKES_A_VALUE)
def test_a_flag_without_its_value_is_a_usage_error(tmp_path, flag):
    r = run([CFG, flag], tmp_path)
    assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE)
    assert not os.listdir(tmp_path)
