"""Where a large np_sgemm launch goes — the library stream behind everything, the library stream next to the side lane, or the
side lane (numpower_amd/csrc/np_sgemm_lane.h) — is decided by a device-free function.  tests/sgemm_lane/lane_decide_main.cpp runs
it through a table of operand ranges (zero-size, abutting, one shared float, nested, windows of wider matrices, rows folded
over each other), sequence numbers and flags; here that program is built with AddressSanitizer + UndefinedBehaviorSanitizer and
run on its own: exit status 0, its closing line, and not a word from a sanitizer."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_lane_decide_table_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = tmp_path / "lane_decide"
    cmd = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-g", "-O1", "-I%s" % (ROOT / "numpower_amd" / "csrc"),
           str(ROOT / "tests" / "sgemm_lane" / "lane_decide_main.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert built.returncode == 0, "%s\n%s" % (" ".join(cmd), built.stderr[-3000:])
    ran = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert ran.returncode == 0, "%s\n%s" % (ran.stdout[-3000:], ran.stderr[-3000:])
    assert ran.stdout.strip().endswith("lane_decide: all rows pass"), ran.stdout[-3000:]
    assert "Sanitizer" not in ran.stderr and "runtime error" not in ran.stderr, ran.stderr[-3000:]
