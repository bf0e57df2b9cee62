"""The C++ mirror of the bivariate LUT bootstrap (zig-tfhe_amd/cpp/tfhe.hpp: lutGenerate2, lutApply2, lutSpread,
bootstrapLutEach): the 4-bit x 4-bit products of cpp/test_lut_tree.cpp decrypt on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")


@pytest.mark.gpu
def test_cpp_lut_tree_tests_pass_on_gpu():
    exe = os.path.join(PKG, "lib", "test_lut_tree")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
