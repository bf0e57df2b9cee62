"""Host-only half of the gadget grid (gadget_grid_cases.py): the oracle's decomposition and
both decomposition offsets against plain Python integers at every accepted (L, bgbit) boundary, what the
parameter check accepts and refuses, and the two facts the GPU half builds on: the oracle's pre-rounding
values at (1,24) stay inside the reference's defined range, and the crafted near-tie key parts the
oracle's fused arithmetic from its reference trees at (1,7).  No kernel runs here."""
import ctypes as C

import numpy as np
import pytest

import tfhe_amd
from gadget_grid_cases import (GRID, L2SMALL, grid_keys, grid_set, lut_nodes_case, near_tie_batch, rotate_modes, rotation_inputs,
                               small_products, whole_form_packs, words)

M32 = (1 << 32) - 1


def py_offset(L, bgbit):
    return sum((1 << (bgbit - 1)) << (32 - (l + 1) * bgbit) for l in range(L)) & M32


def py_digit(x, off, l, bgbit):
    return ((((x + off) & M32) >> (32 - (l + 1) * bgbit)) & ((1 << bgbit) - 1)) - (1 << (bgbit - 1))


def _params_status(d):
    """A context-free call whose only reason to refuse these arguments is params_ok."""
    p, v = tfhe_amd.make_params(d), C.c_uint32()
    return tfhe_amd.load_library().tfhe_decomposition_offset(C.byref(p), C.byref(v))


@pytest.mark.parametrize("L,bgbit", GRID)
def test_offset_and_digits_are_the_integer_definition(oracle, L, bgbit):
    """1,000 random words plus 0, 0xFFFFFFFF and 0x80000000 on both polynomials: every digit of
    oracle.decomposition equals ((x + offset) >> (32 - (l+1) bgbit)) & (Bg - 1)) - Bg/2 in Python integers, lies
    in [-Bg/2, Bg/2), and the digits rebuild x to within the 32 - L bgbit dropped low bits (x minus the
    rebuilt word is exactly the low bits of x + offset, in [0, 2^drop); 0 at (2,16), where nothing is dropped).  The oracle's offset and the library's
    host-side one (tfhe_decomposition_offset) are the same integer."""
    from oracle import OracleParams
    d = grid_set(L, bgbit)
    p = OracleParams(**d)
    off = py_offset(L, bgbit)
    assert oracle.decomposition_offset(p) == off
    assert tfhe_amd.decomposition_offset(tfhe_amd.make_params(d)) == off
    xs = words(100 * L + bgbit, 2 * p.N)
    xs[:3], xs[p.N:p.N + 3] = [0, 0xFFFFFFFF, 0x80000000], [0x80000000, 0, 0xFFFFFFFF]
    dig = oracle.decomposition(p, xs, off).view(np.int32).astype(np.int64)  # (2L, N): a's levels, then b's
    half, drop = 1 << (bgbit - 1), 32 - L * bgbit
    assert dig.min() >= -half and dig.max() < half
    for j in list(range(1000)) + list(range(p.N, p.N + 24)):
        x = int(xs[j])
        rows = dig[L * (j // p.N):L * (j // p.N + 1), j % p.N]
        assert [int(v) for v in rows] == [py_digit(x, off, l, bgbit) for l in range(L)], (j, hex(x))
        rebuilt = sum(int(v) << (32 - (l + 1) * bgbit) for l, v in enumerate(rows))
        # the offset's Bg/2 per level cancels the digits' - Bg/2: what is left is (x + offset)'s dropped bits
        assert (x - rebuilt) % (1 << 32) == ((x + off) & M32) & ((1 << drop) - 1), (j, hex(x))


def test_one_bit_gadget_has_digits_minus_one_and_zero(oracle):
    from oracle import OracleParams
    p = OracleParams(**grid_set(1, 1))
    dig = oracle.decomposition(p, words(5, 2 * p.N), py_offset(1, 1)).view(np.int32)
    assert set(np.unique(dig).tolist()) == {-1, 0}


def test_parameter_check_accepts_the_grid_and_refuses_beyond_it():
    """Every grid set passes params_ok through a context-free call.  Refused with TFHE_ERR_INVALID: bgbit = 32
    (Bg does not fit a 32-bit word; it used to be accepted at L = 1), bgbit = 0, and L bgbit > 32 at each L.
    (1,31), the new upper edge, is accepted.  tfhe_gpu_create gives the reason, before it touches a device."""
    for L, bgbit in GRID:
        assert _params_status(grid_set(L, bgbit)) == 0, (L, bgbit)
    assert _params_status(L2SMALL) == 0 and _params_status(grid_set(1, 31)) == 0
    for L, bgbit in [(1, 32), (1, 33), (1, 0), (2, 17), (3, 11), (2, 32)]:
        assert _params_status(grid_set(L, bgbit)) == tfhe_amd.ERR_INVALID, (L, bgbit)
    for (L, bgbit), text in [((1, 32), r"bgbit must be in \[1, 31\]"), ((3, 11), "bgbit\\*L must be <= 32")]:
        with pytest.raises(tfhe_amd.TfheError, match=text) as e:
            tfhe_amd.Context(tfhe_amd.make_params(grid_set(L, bgbit)), 0)
        assert e.value.status == tfhe_amd.ERR_INVALID


def test_the_grid_sits_on_the_boundaries_it_claims():
    """small_products() and whole_form_packs() restated: the grid has both sides of each boundary."""
    assert [g for g in GRID if small_products(*g)] == [(1, 1), (1, 7), (2, 1), (3, 1)]
    assert small_products(2, 6) and small_products(3, 6) and not small_products(2, 7) and not small_products(1, 8)
    assert [g for g in GRID if not whole_form_packs(*g)] == [(3, 9), (3, 10)]
    assert {L * b for L, b in GRID if L * b == 32} == {32}


def test_pre_rounding_values_stay_in_the_defined_range_at_1_24(oracle):
    """The reference's @intFromFloat is defined for |r| < 2^63 only.  At (1,24) every value the oracle rounds on
    the GPU tests' inputs stays below it: measured max |r| = 2^60.2 over the 131,072 values of the 8 rotation
    inputs, and 2^60.3 over the lut_apply nodes with uniform tables (a margin of 2^2.7).  The other sets are far
    below (2^52.6 at (2,16), 2^46.9 at (3,10))."""
    k = grid_keys(oracle, 1, 24)
    run = lambda cts, tvs: oracle.rounded_values(
        lambda: [oracle.blind_rotate(k.p, c, np.ascontiguousarray(tv), k.ck.bk, k.ck.offset) for c, tv in zip(cts, tvs)],
        cap=1 << 20)
    x = rotation_inputs()
    vals = run(x, [k.ck.testvec] * len(x))
    assert vals.size == len(x) * k.p.n * 2 * k.p.N
    pool, nodes, tables, xs = lut_nodes_case()
    vals2 = run(xs, [tables[n[0]] for n in nodes])
    worst = max(np.abs(vals).max(), np.abs(vals2).max())
    print(f"(1,24): max |r| = 2^{np.log2(np.abs(vals).max()):.2f} (rotations), 2^{np.log2(np.abs(vals2).max()):.2f} (LUT nodes)")
    assert worst < 2.0 ** 63


def test_crafted_key_parts_the_fused_arithmetic_at_1_7(oracle):
    """What test_gadget_grid.test_margin_guard_recomputes_near_ties_at_l1 relies on: under
    conftest.crafted_near_tie_case at (1,7) (every digit of step 0 is -64) the oracle's fused mode returns other
    words than its reference mode on the crafted item."""
    k = grid_keys(oracle, 1, 7)
    tv, bk, cts = near_tie_batch(oracle, k.p)
    want, fused = rotate_modes(oracle, k.p, cts, tv, bk, k.ck.offset)
    assert not np.array_equal(want[2], fused[2])
