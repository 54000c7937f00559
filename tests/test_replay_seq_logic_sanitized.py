"""The window sampler's host logic (hsr_env_amd/csrc/replay_logic.h: replay_sample_seq_error, replay_nstep) is plain C++ that the kernel
and a host program both compile, so a stand-alone program (tests/replay_seq_logic_main.cpp) runs it under AddressSanitizer and
UndefinedBehaviorSanitizer here, as tests/test_replay_logic_sanitized.py does for the books.  Any report fails the test.
-ffp-contract=off is to g++ what the header's clang pragma is to hipcc: products and sums round separately."""
import shutil
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")
def test_replay_seq_logic_under_asan_ubsan(tmp_path):
    exe = tmp_path / "replay_seq_logic"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe), str(HERE / "replay_seq_logic_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.startswith("ok ")
