"""The pure decisions of the hand-over of hard envs inside a launch (hsr_env_amd/csrc/split_logic.h) - which envs a wave gives away
at a check point, and whether a launch splits at all (split_plan, and plan_launch of launch_plan.h, which asks it and sets the grid) - are plain C++ that the kernel, the
host layer and a host program all compile.  tests/split_logic_main.cpp checks the donor's decision exhaustively over small inputs and the
plan over its cases; an ordinary host build, no GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")
def test_split_decisions(tmp_path):
    exe = tmp_path / "split_logic"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe), str(HERE / "split_logic_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert r.stdout.startswith("ok ")

