"""The C++ mirror of the extended nodes (zig-tfhe_amd/cpp/tfhe.hpp: LutCircuit's eta arguments, lutSelectExt,
bootstrapLutEachExt): the 64-word encrypted memory of cpp/test_lut_circuit_ext.cpp, read through one extended
select node per address, decrypts on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")


@pytest.mark.gpu
def test_cpp_lut_circuit_ext_tests_pass_on_gpu():
    exe = os.path.join(PKG, "lib", "test_lut_circuit_ext")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
