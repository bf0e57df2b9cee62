"""The host-only half of the extended LUT bootstrap (include/tfhe_gpu.h "Extended LUT bootstrap"): the
extended test vector's components against the oracle's generator at degree N * E, X^a on E components
against the oracle's polyMulWithXK at degree N * E, and the point of the feature from the mod switch
alone: at UINT4 and m = 64 the rounding to 2N positions throws one input in six off its block, the
rounding to 8N positions (eta = 2) none.  No kernel runs here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tfhe_amd
from conftest import rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zig-tfhe_amd")
UINT4 = tfhe_amd.make_params("uint4")
N = UINT4.N


def words(seed, *shape):
    return rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def interleave(comps):
    """(E, 2N) components -> the two polynomials of degree N * E, (2, N * E): coefficient k E + j = component j's k."""
    E = comps.shape[0]
    return comps.reshape(E, 2, N).transpose(1, 2, 0).reshape(2, N * E)


def split(halves, E):
    """The inverse of interleave: (2, N * E) -> (E, 2N)."""
    return halves.reshape(2, N, E).transpose(2, 0, 1).reshape(E, 2 * N)


@pytest.mark.parametrize("eta", [0, 1, 2])
@pytest.mark.parametrize("m", [2, 16, 32, 64, 128])
def test_generate_ext_is_the_component_split_of_the_oracles_table(oracle, eta, m):
    E = 1 << eta
    f = [(7 * x + 3) % m for x in range(m)]
    got = tfhe_amd.lut_generate_ext(UINT4, eta, m, f)
    assert got.shape == (E, 2 * N)
    want = oracle.lut_generate(N * E, m, f).reshape(2, N * E)
    assert np.array_equal(got, split(want, E))
    assert not got[:, :N].any()  # tv_j.a = 0
    assert np.array_equal(got, tfhe_amd.lut_generate_ext(UINT4, eta, m, lambda x: (7 * x + 3) % m))
    if eta == 0:
        assert np.array_equal(got[0], tfhe_amd.lut_generate(UINT4, m, lambda x: (7 * x + 3) % m))


@pytest.mark.parametrize("eta", [0, 1, 2])
def test_ext_rotate_is_the_rotation_of_the_interleaved_polynomial(oracle, eta):
    E, D = 1 << eta, N << eta
    comps = words(60 + eta, E, 2 * N)
    poly = interleave(comps)
    g = rng(70 + eta)
    for a in [0, 1, E - 1, E, D - 1, D, D + 1, 2 * D - 1, 2 * D] + [int(v) for v in g.integers(0, 2 * D + 1, 12)]:
        got = tfhe_amd.lut_ext_rotate_host(UINT4, eta, comps, a)
        want = np.array([oracle.poly_mul_with_xk(poly[h], a) for h in range(2)])
        assert np.array_equal(got, split(want, E)), a
    assert np.array_equal(tfhe_amd.lut_ext_rotate_host(UINT4, eta, comps, 2 * D), comps)  # the identity
    with pytest.raises(tfhe_amd.TfheError) as e:
        tfhe_amd.lut_ext_rotate_host(UINT4, eta, comps, 2 * D + 1)
    assert e.value.status == tfhe_amd.ERR_INVALID


def mod_switch(x, eta):
    """(word + 2^(sh-1)) >> sh in 64 bits, sh = 32 - (nbit + 1) - eta, on an array."""
    sh = 32 - 11 - eta
    return (x.astype(np.uint64) + (1 << (sh - 1))) >> sh


@pytest.mark.parametrize("eta", [0, 1, 2])
def test_mod_switch_entry_is_the_64_bit_formula(eta):
    sh, top = 21 - eta, 2 * N << eta
    x = np.concatenate([words(80 + eta, 500),
                        np.array([0, 0xFFFFFFFF, (1 << (sh - 1)) - 1, 1 << (sh - 1), 1 << 31, 0xFFFFFFFF - (1 << (sh - 1))],
                                 np.uint32)])
    got = [tfhe_amd.lut_ext_mod_switch(UINT4, eta, int(v)) for v in x]
    assert got == mod_switch(x, eta).tolist()
    assert got[500:504] == [0, top, 0, 1] and max(got) == top


def rounding_phase_error(eta, cts, key):
    """The phase error the mod switch to 2N E positions adds to each ciphertext, as a fraction of the torus in
    [-1/2, 1/2): (b~ - sum a~_i s_i) / (2N E) - (b - sum a_i s_i) / 2^32, exactly, from the key."""
    sh = 21 - eta
    s = key.astype(np.uint64)
    phase = (cts[:, -1].astype(np.uint64) - cts[:, :-1].astype(np.uint64) @ s) & 0xFFFFFFFF
    r = mod_switch(cts, eta)
    rounded = ((r[:, -1] - r[:, :-1] @ s) << sh) & 0xFFFFFFFF  # back on the 2^32 scale: exact
    d = ((rounded - phase) & 0xFFFFFFFF).astype(np.int64)
    return np.where(d >= 1 << 31, d - (1 << 32), d) / 2.0 ** 32


def test_the_mod_switch_alone_decides_six_bit_digits():
    """4,096 uniform UINT4 ciphertexts under a seeded binary key, rounding error only.  At m = 64 a block is read
    1/(4m) = 1/256 of the torus from its edge.  Measured on 20,000 such ciphertexts: eta = 0 puts 16.5 % outside
    (1.4 sigma), eta = 2 none (5.5 sigma)."""
    sk = tfhe_amd.secret_key_new(UINT4, 4242)
    cts = words(90, 4096, UINT4.n + 1)
    half_spacing = 1.0 / 256
    e0 = rounding_phase_error(0, cts, sk.key_lv0)
    e2 = rounding_phase_error(2, cts, sk.key_lv0)
    outside0, outside2 = int((np.abs(e0) > half_spacing).sum()), int((np.abs(e2) > half_spacing).sum())
    print(f"outside the half-spacing: eta=0 {outside0}/4096, eta=2 {outside2}/4096; "
          f"sigma {e0.std():.3e} / {e2.std():.3e} of the torus")
    assert outside0 >= 0.10 * 4096
    assert outside2 == 0
    # the rule of the header: sigma ~ sqrt((n/2 + 1) / 12) positions of 2N E whatever eta is
    want = np.sqrt((UINT4.n / 2 + 1) / 12)
    assert abs(e0.std() * 2 * N - want) < 0.1 * want and abs(e2.std() * 8 * N - want) < 0.1 * want


def test_eta_three_is_refused_by_every_host_function():
    for call in (lambda: tfhe_amd.lut_generate_ext(UINT4, 3, 16, lambda x: x),
                 lambda: tfhe_amd.lut_ext_rotate_host(UINT4, 3, np.zeros((8, 2 * N), np.uint32), 0),
                 lambda: tfhe_amd.lut_ext_mod_switch(UINT4, 3, 0)):
        with pytest.raises(tfhe_amd.TfheError) as e:
            call()
        assert e.value.status == tfhe_amd.ERR_INVALID
    # the ABI keeps its number: additions only
    assert tfhe_amd.load_library().tfhe_gpu_abi_version() == 7


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_host_unit_tests_pass():
    exe = os.path.join(PKG, "lib", "test_lut_ext_cpu")
    assert os.path.exists(exe), "build first: make -C zig-tfhe_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
