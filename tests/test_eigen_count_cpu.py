"""CPU: the count of a proposal's decompositions (icp-proposal_amd/csrc/icp_eigen_count.hpp) — places in the cycle of 128, which decide
the cold starts, and completion-word numbers, which are never issued twice.

The header is plain C++; tests/support/eigen_count_check.cpp plays random chains (one-lane steps, twin passes whose second lane is
used or dropped, steps repeated from scratch, planned-only places, ordinary decompositions) in the one-at-a-time order of a single
counter and in the early order of EigenCount, and compares the cold starts of every decomposition the two have in common.  Foreign
writers (the on-device loops: they count on from the place and raise completion words to the places they take) come in between: no
number issued behind one may lie at or below a word it wrote."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_places_and_numbers_of_early_second_lanes(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on the path")
    exe = str(tmp_path / "eigen_count_check")
    src = os.path.join(ROOT, "tests", "support", "eigen_count_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, src], check=True, timeout=120)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok")
