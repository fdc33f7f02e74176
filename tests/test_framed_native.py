"""csrc/tests/test_framed.cpp (Pump::check_frames and send_framed_batch over
seeded, mutated buffers), built with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a stand-alone program."""

import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_framed_pump_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "test_framed_asan"
    subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
         "-I", str(REPO / "csrc"), str(REPO / "csrc" / "tests" / "test_framed.cpp"),
         "-o", str(exe), "-lpthread"],
        check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "framed pump OK" in out.stdout
