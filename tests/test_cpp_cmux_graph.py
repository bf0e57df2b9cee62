"""The C++ mirror of the CMUX graphs (zig-tfhe_amd/cpp/tfhe.hpp: CmuxGraph, cmuxGraph): a 16-bit a < b on
encrypted bits, its results fed to a gate, on the GPU (cpp/test_cmux_graph.cpp); and the planner's stand-alone
host program (cpp/test_cmux_graph_cpu.cpp, linked with tfhe_cpu.o alone: no GPU, no Python extension)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")


def test_cpp_cmux_graph_cpu_program_passes():
    exe = os.path.join(PKG, "lib", "test_cmux_graph_cpu")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASSED" in r.stdout and "ok   plan: refusals" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_cmux_graph_tests_pass_on_gpu():
    exe = os.path.join(PKG, "lib", "test_cmux_graph")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
