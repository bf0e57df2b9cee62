"""The C++ mirror of the packed lookup (zig-tfhe_amd/cpp/tfhe.hpp: PackedTableLookup,
rotateByBits): a 256-entry S-box as 2 TRLWEs looked up with 8 CMUXes per query, and a
rotation by three encrypted bits, pass on the GPU (cpp/test_packed_lookup.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")


@pytest.mark.gpu
def test_cpp_packed_lookup_tests_pass_on_gpu():
    exe = os.path.join(PKG, "lib", "test_packed_lookup")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
