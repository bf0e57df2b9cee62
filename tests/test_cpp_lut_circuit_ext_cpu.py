"""The extended nodes' planner and the E-copies identity through their stand-alone C++ test program
(zig-tfhe_amd/cpp/test_lut_circuit_ext_cpu.cpp, linked with tfhe_cpu.o alone): no GPU, no Python extension."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")


def test_cpp_lut_circuit_ext_cpu_program_passes():
    exe = os.path.join(PKG, "lib", "test_lut_circuit_ext_cpu")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASSED" in r.stdout and "ok   E copies" in r.stdout, r.stdout + r.stderr
