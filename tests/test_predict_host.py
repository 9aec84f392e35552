"""The host half of kb2e_predict's filter (kb2e_amd/csrc/predict_host.hpp): the
known candidates of every query, listed once from the filter triples.  A
stand-alone program checks the lists against a brute-force loop (empty filter,
duplicate filter triples, queries that share (e, r, side), both sides), built
with ASan + UBSan and run directly."""
import os
import subprocess

from conftest import ROOT


def test_known_candidate_lists_match_brute_force(tmp_path):
    exe = tmp_path / "predict_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "kb2e_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "predict_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok"
