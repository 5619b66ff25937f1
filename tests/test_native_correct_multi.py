"""CPU: gf_host.hpp's check_correct (the arithmetic of sec_check_correct, the model of the correcting
kernels' judge) under sanitizers, as a stand-alone program: g++ -fsanitize=address,undefined of
tests/native/test_correct_multi.cpp, run directly."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "test_correct_multi.cpp")
CSRC = os.path.join(ROOT, "storb_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_native_correct_multi_sanitized(tmp_path):
    exe = tmp_path / "test_correct_multi"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    f"-I{CSRC}", SRC, "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "native correct_multi tests ok" in r.stdout
