"""CPU tests of the leveled operations: the host-only table packing against numpy,
the argument checks that return before any device is touched, the stand-alone
host program under the sanitizers (make cpu-check), and the leveled kernels'
register report (no scratch spill on gfx950).  No kernel is launched here."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tfhe_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")
u32p = C.POINTER(C.c_uint32)


@pytest.mark.parametrize("pname", ["128", "uint4"])
@pytest.mark.parametrize("width", [0, 1, 8, 64, 70, 1024])
def test_lookup_table_pack_bits_matches_numpy(pname, width):
    p = tfhe_amd.make_params(pname)
    values = np.random.default_rng(width).integers(0, 1 << 63, 9, dtype=np.uint64) * 2 + 1
    got = tfhe_amd.lookup_table_pack_bits(p, values, width)
    c = np.arange(p.N)
    bits = ((values[:, None] >> np.minimum(c, 63).astype(np.uint64)[None, :]) & 1).astype(bool) & (c < 64)[None, :]
    b = np.where(c[None, :] < width, np.where(bits, 0x20000000, 0xE0000000), 0).astype(np.uint32)
    assert got.shape == (9, 2 * p.N)
    assert not got[:, :p.N].any()
    assert np.array_equal(got[:, p.N:], b)


def test_lookup_table_pack_bits_rejects_bad_arguments():
    lib = tfhe_amd.load_library()
    p = tfhe_amd.make_params("128")
    v = np.array([5], np.uint64)
    vp_ = v.ctypes.data_as(C.POINTER(C.c_uint64))
    t = np.zeros(2 * p.N, np.uint32)
    tp = t.ctypes.data_as(u32p)
    assert lib.tfhe_lookup_table_pack_bits(None, vp_, 1, 8, tp) == tfhe_amd.ERR_INVALID
    assert lib.tfhe_lookup_table_pack_bits(C.byref(p), None, 1, 8, tp) == tfhe_amd.ERR_INVALID
    assert lib.tfhe_lookup_table_pack_bits(C.byref(p), vp_, 1, 8, None) == tfhe_amd.ERR_INVALID
    assert lib.tfhe_lookup_table_pack_bits(C.byref(p), vp_, 1, p.N + 1, tp) == tfhe_amd.ERR_INVALID
    with pytest.raises(tfhe_amd.TfheError):
        tfhe_amd.lookup_table_pack_bits(p, [1, 2], 2000)
    p.N = 512
    assert lib.tfhe_lookup_table_pack_bits(C.byref(p), vp_, 1, 8, tp) == tfhe_amd.ERR_INVALID


def test_leveled_entries_refuse_a_null_context():
    """Every leveled entry point returns TFHE_ERR_INVALID for a NULL context (or set)
    before it touches a device."""
    lib = tfhe_amd.load_library()
    x = np.zeros(2048, np.uint32)
    xp = x.ctypes.data_as(u32p)
    f = np.zeros(8, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    b = np.zeros(1024, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    INV = tfhe_amd.ERR_INVALID
    assert lib.tfhe_gpu_trlwe_encrypt_batch(None, xp, f, 0.0, 1, xp, 1) == INV
    assert lib.tfhe_gpu_trlwe_decrypt_bool_batch(None, xp, xp, b, 1) == INV
    assert lib.tfhe_gpu_trgsw_encrypt_batch(None, xp, xp, 0.0, 1, f, 1) == INV
    h = C.c_void_p(1)
    assert lib.tfhe_gpu_trgsw_set_load(None, f, 1, C.byref(h)) == INV and not h.value
    assert lib.tfhe_gpu_cmux_batch(None, None, xp, xp, xp, xp, 1) == INV
    assert lib.tfhe_gpu_cmux_batch_dev(None, None, xp, None, None, None, 1) == INV
    assert lib.tfhe_gpu_table_lookup_batch(None, None, xp, 3, xp, xp, 1) == INV
    assert lib.tfhe_gpu_table_lookup_dev(None, None, xp, 3, None, None, 1) == INV
    assert lib.tfhe_gpu_sample_extract_batch(None, xp, xp, 1, 0, xp, 1) == INV
    assert lib.tfhe_gpu_sample_extract_dev(None, None, xp, 1, 1, None, 1) == INV
    lib.tfhe_gpu_trgsw_set_destroy(None)  # like free(NULL)
    assert tfhe_amd.OPTIONS["cmux_form"] == 18 and tfhe_amd.OPTION_DEFAULTS["cmux_form"] == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cpu_check_passes():
    """make cpu-check: test_cpu.cpp and test_leveled_cpu.cpp with tfhe_cpu.cpp under ASan + UBSan."""
    r = subprocess.run(["make", "-s", "-C", PKG, "cpu-check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.count("PASSED") == 2, r.stdout[-2000:] + r.stderr[-2000:]


def test_leveled_kernels_compile_without_scratch():
    """hipcc's resource report for tfhe_kernels_leveled.hip on gfx950, with the library's flags: every
    kernel of the unit (k_cmux<1..3>, k_cmux_shared<1..3>, k_sample_extract) uses no scratch memory."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall",
                        f"-I{ROOT}/include", f"-I{PKG}/csrc", "-c", "-o", os.devnull,
                        os.path.join(PKG, "csrc", "tfhe_kernels_leveled.hip"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) >= 5
    for want in ("k_cmuxILi1E", "k_cmuxILi3E", "k_sample_extract"):
        assert any(want in n for n in names), (want, names)
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
