"""csrc/edt_table.h's pure layer (the column walk, the three table layouts, the range sweep) on the
host alone: tests/c_abi/table_host_test.cpp, a program of its own, built with the host C++ compiler
under AddressSanitizer and UBSan and run as a child process. No GPU, no ROCm, nothing loaded here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_pure_layer_under_asan_and_ubsan(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "table_host_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover", "-I", os.path.join(ROOT, "evolutionarydistributedtraining_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_abi", "table_host_test.cpp"), "-o", exe], check=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                                UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert p.returncode == 0 and "table host checks ok" in p.stdout, (p.stdout + p.stderr)[-3000:]
