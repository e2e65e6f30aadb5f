"""CPU: the round and piece plans of the context-free "many in one call" entry points (icp-proposal_amd/csrc/icp_round_plan.hpp) — which
items share a round of the one buffer, where every item's part of every region starts, how large the buffer and the staging blocks
are, and how the rows of the bases are cut into pieces that fill the chunk buffer.

The header is plain C++; tests/support/round_plan_check.cpp restates the loops the entry points were written with before they shared it
(icp_scans_prepare_many, icp_decimate_many, icp_surface_samples_many; the piece loop of the GP and Nyström models) and compares every
integer of RegionCursor, RegionRounds<3>, RegionRounds<4> and RowPieces with them, exactly: designed edges (an item of exactly the
budget, one word more, a budget of 1, every item oversize, empty regions; fewer rows than a quantum, a chunk of one quantum, an item
that takes no part, the cap on pieces) and a few thousand random plans from a fixed seed.  Built twice: as it is, and with the address
and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_rounds_offsets_and_pieces_match_the_loops_they_replace(tmp_path, sanitize):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on the path")
    exe = str(tmp_path / "round_plan_check")
    src = os.path.join(ROOT, "tests", "support", "round_plan_check.cpp")
    flags = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        flags += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, "-o", exe, src], check=True, timeout=120)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok")
