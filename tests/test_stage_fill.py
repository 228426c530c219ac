"""The window filler of the staged upload (kgma_stage_fill.h) alone, on the CPU: tools/stage_fill_main.cpp checks it against a
byte-by-byte model over seeded random segment lists and over a file that is shorter than a segment claims.  The program is built
with the address and undefined-behaviour sanitizers and run on its own; nothing of it is loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_fill_against_the_byte_model(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "stage_fill"
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(ROOT, "tools", "stage_fill_main.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
