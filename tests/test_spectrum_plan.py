"""The plan of kgma_genome_kmer_count (kgma_spectrum.h: argument checks, considered starts, unit prefix, form and geometry) alone,
on the CPU: tools/spectrum_plan_main.cpp checks it against a model that counts the considered starts one by one, over seeded
random range lists and over every argument error.  The program is built with the address and undefined-behaviour sanitizers and
run on its own; nothing of it is loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spectrum_plan_against_the_counting_model(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "spectrum_plan"
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(ROOT, "tools", "spectrum_plan_main.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "spectrum plan ok" in run.stdout
