"""CPU tests of the packed scatter-add's GPU-free half: the exported entries and their null-context refusal, the
chunk option's key and default, the Python wrappers' size check, and the definition the GPU tests compare with
(tests/scatter_model.py), checked here by decryption on the oracle."""
import ctypes as C

import numpy as np
import pytest

import tfhe_amd
from scatter_model import scatter_add, scatter_leaves, trlwe_phase

u32p = C.POINTER(C.c_uint32)


def test_entries_are_exported_and_refuse_a_null_context():
    lib = tfhe_amd.load_library()
    x = np.zeros(2048, np.uint32)
    xp = x.ctypes.data_as(u32p)
    INV = tfhe_amd.ERR_INVALID
    assert lib.tfhe_gpu_packed_scatter_add_batch(None, None, xp, 3, 8, xp, xp, 1) == INV
    assert lib.tfhe_gpu_packed_scatter_add_dev(None, None, xp, 3, 8, None, None, 1) == INV
    for name in ("tfhe_gpu_packed_scatter_add_batch", "tfhe_gpu_packed_scatter_add_dev"):
        assert name in tfhe_amd.EXPORTED_SYMBOLS


def test_scatter_scratch_option_key_and_default():
    assert tfhe_amd.OPTIONS["scatter_scratch_mb"] == 20 and tfhe_amd.OPTION_DEFAULTS["scatter_scratch_mb"] == 256


class _NoLibrary:
    """Stands in for a Context: the wrappers must raise before they reach the C library."""

    def __init__(self):
        self.params = tfhe_amd.make_params("128")

    @property
    def lib(self):
        raise AssertionError("the wrapper reached the C library")

    h = None

    def check(self, rc, what):
        raise AssertionError("the wrapper reached the C library")


def test_wrappers_refuse_a_table_of_the_wrong_size_before_the_call():
    fake = _NoLibrary()
    addr = np.zeros((1, 8), np.uint32)  # k = 8, width 8: 2 TRLWEs
    delta = np.zeros((1, 2048), np.uint32)
    for rows in (1, 3):
        with pytest.raises(ValueError):
            tfhe_amd.Context.packed_scatter_add(fake, None, addr, 8, delta, np.zeros((rows, 2048), np.uint32))
        with pytest.raises(ValueError):
            tfhe_amd.Context.packed_scatter_add_dev(fake, None, addr, 8, 0x1000, 0x2000, table_trlwes=rows)
    with pytest.raises(AssertionError):  # the right size goes on to the library
        tfhe_amd.Context.packed_scatter_add(fake, None, addr, 8, delta, np.zeros((2, 2048), np.uint32))


def test_definition_moves_a_delta_to_its_slot(oracle, keys128):
    """k = 9, width 8 (stride 8, h = 7, v = 2) at the 128-bit set: +1/4 on coefficients 0 .. 7, written to address
    0b10_1100101, arrives at coefficients 8 * 101 .. 8 * 101 + 7 of leaf 2; every other coefficient of every leaf
    holds noise only.  Then the sum: a table of -1/8 bits with the delta added decrypts to 1 exactly there."""
    p, k1 = keys128.p, keys128.k1
    N = p.N
    tp = tfhe_amd.make_params("128")
    plan = tfhe_amd.packed_lookup_plan(tp, 9, 8)
    assert (plan.stride, plan.h, plan.v, plan.trlwes) == (8, 7, 2, 4)
    off = oracle.decomposition_offset(p)
    trgsw = np.array([oracle.trgsw_encrypt_torus_fft(p, mu, p.alpha_bsk, k1, 960 + mu) for mu in (0, 1)])
    address = 0b101100101
    addr_row = [(address >> j) & 1 for j in range(9)]
    mu = np.zeros(N)
    mu[:8] = 0.25
    delta = oracle.trlwe_encrypt_f64(p, mu, p.alpha_lv1, k1, 970)
    leaves = scatter_leaves(oracle, p, off, trgsw, plan, 9, delta, addr_row)
    assert len(leaves) == 4
    slot, leaf = address & 127, address >> 7
    for i, x in enumerate(leaves):
        want = np.zeros(N)
        if i == leaf:
            want[8 * slot:8 * slot + 8] = 0.25
        assert np.abs(trlwe_phase(oracle, N, x, k1) - want).max() < 0.01, i
    table = tfhe_amd.lookup_table_pack_slots(tp, np.zeros(512, np.uint64), 8)
    new = scatter_add(oracle, p, off, trgsw, plan, 9, [delta], [addr_row], table)
    for i in range(4):
        bits = oracle.trlwe_decrypt_bool(p, new[i], k1)
        want = np.zeros(N, bool)
        if i == leaf:
            want[8 * slot:8 * slot + 8] = True
        assert np.array_equal(bits, want), i
