"""The normaliser's arithmetic and argument checks (hsr_env_amd/csrc/normalize_logic.h: the HSR_EINVAL conditions, the finite test, Chan's
merge, the publish rule, the float32 apply, the shape of the sums) are plain C++ that the kernels and a host program both compile, so a
stand-alone program (tests/normalize_logic_main.cpp) runs them under AddressSanitizer and UndefinedBehaviorSanitizer here, as
tests/test_replay_prio_logic_sanitized.py does for the priorities.  Any report fails the test."""
import shutil
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")
def test_normalize_logic_under_asan_ubsan(tmp_path):
    exe = tmp_path / "normalize_logic"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe), str(HERE / "normalize_logic_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.startswith("ok ")
