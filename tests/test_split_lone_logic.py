"""The lone rule of the hand-over inside a launch (hsr_env_amd/csrc/split_logic.h: split_decide_lone - a wave's one hard env leaves its
easier neighbours for a finished workgroup) is plain C++ that the kernel and a host program both compile.  tests/split_lone_logic_main.cpp
checks its properties exhaustively over small inputs - off it is split_decide; never a dead group; never every live env, nor does any
subset of the result; on, no env at or above the threshold stays next to a live env below it - and the way plan_launch carries the setting;
an ordinary host build, no GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")
def test_lone_decisions(tmp_path):
    exe = tmp_path / "split_lone_logic"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", str(exe), str(HERE / "split_lone_logic_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert r.stdout.startswith("ok ")
