"""CPU: the tile maps' XCD-major placement (kernels.hpp tile_slot, bs_plan.hpp append_placed) under
AddressSanitizer + UBSan: g++ builds tests/native/test_tile_slot.cpp, a program of its own."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "test_tile_slot.cpp")
CSRC = os.path.join(ROOT, "storb_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_native_tile_slot_sanitized(tmp_path):
    exe = tmp_path / "test_tile_slot"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    f"-I{CSRC}", SRC, "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tile slot tests ok" in r.stdout
