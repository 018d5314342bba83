"""CPU test of the grouping helpers and the chunk plan the spot, spot detection and spot quantile host drivers share (csrc/apd_plan.h:
number_by_first_appearance, GroupMembers, GroupChunkPlan): tests/cpp/group_check.cpp checks them against their definitions on seeded
random lists, built under AddressSanitizer + UBSan as a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_helpers_match_their_definitions(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "group_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "group_check.cpp"), "-o", exe])
    out = subprocess.run([exe, "3000", "20262"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "groups ok: 3000 rounds, no sanitizer report" in out.stdout, out.stdout[-1000:] + out.stderr[-3000:]
