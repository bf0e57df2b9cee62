"""The C++ mirror of the packing key switch (zig-tfhe_amd/cpp/tfhe.hpp: PackingKey, packTlwe,
PackedTableLookup::fromCiphertexts): a table computed by 64 gates, packed into one TRLWE and looked up
by 4 TRGSW-encrypted address bits decrypts to value[addr] ^ mask on the GPU (cpp/test_pack.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")


@pytest.mark.gpu
def test_cpp_pack_tests_pass_on_gpu():
    exe = os.path.join(PKG, "lib", "test_pack")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
