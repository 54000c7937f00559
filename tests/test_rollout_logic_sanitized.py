"""The host books of the on-policy rollout (hsr_env_amd/csrc/rollout_logic.h: row layout, state machine, slot arithmetic, the shuffle's
domain, argument checks) are plain C++ without a HIP call, so a stand-alone program (tests/rollout_logic_main.cpp) runs them under
AddressSanitizer and UndefinedBehaviorSanitizer here, as tests/test_replay_logic_sanitized.py does for the replay's.  Any report fails the
test."""
import shutil
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")
def test_rollout_books_under_asan_ubsan(tmp_path):
    exe = tmp_path / "rollout_logic"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), str(HERE / "rollout_logic_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.startswith("ok ")
