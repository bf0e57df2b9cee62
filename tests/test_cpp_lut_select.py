"""The C++ mirror of the select nodes (zig-tfhe_amd/cpp/tfhe.hpp: LutCircuit::select / node2, lutSelect): the
S-box after a key addition on nibbles of cpp/test_lut_select.cpp, S[x ^ k] for 4 byte pairs in one circuit of
depth 4, decrypts on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")


@pytest.mark.gpu
def test_cpp_lut_select_tests_pass_on_gpu():
    exe = os.path.join(PKG, "lib", "test_lut_select")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
