"""The GPU-free half of the C ABI (zig-tfhe_amd/csrc/tfhe_cpu.cpp): its stand-alone
test program passes (zig-tfhe_amd/cpp/test_cpu.cpp, linked with tfhe_cpu.o alone),
and the unit compiles with the host compiler and no ROCm include path."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cpu_unit_tests_pass():
    exe = os.path.join(PKG, "lib", "test_cpu")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cpu_unit_compiles_without_hip():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", f"-I{ROOT}/include",
                        f"-I{PKG}/csrc", os.path.join(PKG, "csrc", "tfhe_cpu.cpp")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
