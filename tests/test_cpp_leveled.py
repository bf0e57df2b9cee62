"""The C++ mirror of the leveled surface (zig-tfhe_amd/cpp/tfhe.hpp: TRLWELv1,
TRGSWLv1FFT, cmux, TableLookup): the reference's own CMUX test (trgsw.zig:637-692)
and a lookup whose outputs feed a gate pass on the GPU (cpp/test_leveled.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")


@pytest.mark.gpu
def test_cpp_leveled_tests_pass_on_gpu():
    exe = os.path.join(PKG, "lib", "test_leveled")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
