"""The C++ mirror of the extended LUT bootstrap (zig-tfhe_amd/cpp/tfhe.hpp: lutGenerateExt, blindRotateExt,
lutApplyExt): the random 6-bit-to-4-bit table of cpp/test_lut_ext.cpp, looked up at m = 64 with eta = 2 for every
6-bit message, decrypts on the GPU, and one item equals the stage entry's acc_0 extracted and key-switched."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")


@pytest.mark.gpu
def test_cpp_lut_ext_tests_pass_on_gpu():
    exe = os.path.join(PKG, "lib", "test_lut_ext")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
