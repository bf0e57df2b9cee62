"""The C++ mirror of the encrypted table write (zig-tfhe_amd/cpp/tfhe.hpp: packedScatterAdd, packedWrite):
three entries of a 16 x 4-bit packed table set by encrypted addresses and all 16 read back, and one
scatter-add into a table of 4 whole TRLWEs, decrypt to the plaintext model on the GPU
(cpp/test_packed_write.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")


@pytest.mark.gpu
def test_cpp_packed_write_tests_pass_on_gpu():
    exe = os.path.join(PKG, "lib", "test_packed_write")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
