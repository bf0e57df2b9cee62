"""The gadget grid: test-only parameter sets at the boundaries of what params_ok
accepts for (L, bgbit), shared by test_gadget_grid_cpu.py (host only) and test_gadget_grid.py (GPU).

Every set has n = 8 (an oracle blind rotation is 8 CMUXes), N = 1024, UINT4's key switch (basebit 5, 3
levels: the lane, gather and GEMM forms all exist for it) and the noise fields of test_param_sets.SYNTHETIC;
keys come from oracle.cloud_key (sk 42, ck 43).  The points:

  (1,1) (2,1) (3,1)  Bg = 2: a one-bit signed field, digits in {-1, 0}
  (1,7)              the largest gadget with small products at L = 1 (the <1,true,*> kernels)
  (1,8) (2,7) (3,7)  the first gadget without small products at each L (L = 3: <3,false,false>)
  (1,24)             above UINT3's 23
  (2,16)             L bgbit = 32: the last level's field starts at bit 0
  (3,8)              4 bgbit = 32: the largest gadget the L = 3 whole form's packed tmp words hold
  (3,9) (3,10)       4 bgbit > 32: no whole form (the latency form runs; whole_form_packs)
"""
import numpy as np

from conftest import rng

N = 1024
_NOISE = dict(alpha_lv0=2.0e-5, alpha_lv1=2.0e-8, alpha_ksk=2.0e-5, alpha_bsk=2.0e-8)
GRID = [(1, 1), (1, 7), (1, 8), (1, 24), (2, 1), (2, 7), (2, 16), (3, 1), (3, 7), (3, 8), (3, 9), (3, 10)]
EXTREMES = [(1, 1), (2, 16), (3, 8), (3, 10)]
# test_param_sets.SYNTHETIC["l2small"] at n = 8: the one L = 2 gadget with small products besides (2,1)
L2SMALL = dict(n=8, N=N, nbit=10, L=2, bgbit=6, basebit=3, iks_t=4, **_NOISE)


def grid_set(L, bgbit):
    return dict(n=8, N=N, nbit=10, L=L, bgbit=bgbit, basebit=5, iks_t=3, **_NOISE)


def small_products(L, bgbit):
    """tfhe_kernels.hip small_products(): 2 L N Bg/2 2^31 < 2^49, i.e. L Bg < 256."""
    return L * (1 << bgbit) < 256


def whole_form_packs(L, bgbit):
    """tfhe_internal.hpp whole_form_packs(): the L = 3 whole form needs 4 bgbit <= 32."""
    return L != 3 or 4 * bgbit <= 32


def words(seed, *shape):
    return rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def rotation_inputs(n=8):
    """8 TLWELv0 of uniform words, run as B = 3 (rows 0-2) and B = 5 (rows 3-7).  Row 1 has a~ = 0 on the
    first half of its mask and row 4 a~ = 2N (0xFFFFFFFF: the 64-bit add of the modulus switch does not
    wrap) with b~ = 0: CMUX steps whose tmp is zero, as in test_bootstrap_edge_rotations."""
    x = words(7700, 8, n + 1)
    x[1, : n // 2] = 0
    x[4, : n // 2] = 0xFFFFFFFF
    x[4, n] = 0xFFFFFFFF
    return x


I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def lut_nodes_case(n=8):
    """5 LUT-circuit nodes over 4 uniform inputs and 3 uniform tables (bit-exactness only): 0-3 terms, table
    selectors 1, 0, 2, 1, 0 (neighbours differ), a constant on two nodes and int32-edge coefficients on one.
    -> (pool, nodes, tables, the nodes' combined inputs x_i)."""
    from test_lut_circuit import combine
    pool, tables = words(7800, 4, n + 1), words(7801, 3, 2 * N)
    nodes = [(1, [(0, 1), (1, -1)], 0), (0, [(2, 3)], 5 << 27), (2, [], 3 << 29),
             (1, [(3, I32_MIN), (0, I32_MAX), (1, -1)], 0), (0, [(1, 2), (2, 1)], 0)]
    return pool, nodes, tables, combine(pool, nodes)


_KEYS = {}


class GridKeys:
    """Oracle parameters, secret keys and cloud key of a set given as a dict."""

    def __init__(self, oracle, d):
        from oracle import OracleParams
        self.d, self.p = d, OracleParams(**d)
        self.k0, self.k1 = oracle.secret_key(self.p, 42)
        self.ck = oracle.cloud_key(self.p, 43, self.k0, self.k1)


def grid_keys(oracle, L, bgbit):
    """Cached per process; (2, 6) is L2SMALL."""
    if (L, bgbit) not in _KEYS:
        _KEYS[L, bgbit] = GridKeys(oracle, L2SMALL if (L, bgbit) == (2, 6) else grid_set(L, bgbit))
    return _KEYS[L, bgbit]


def near_tie_batch(oracle, p):
    """The margin guard's L = 1 case at (1,7): conftest.crafted_near_tie_case's key and ciphertext (item 2)
    among five uniform ones."""
    from conftest import crafted_near_tie_case
    tv, bk, ct = crafted_near_tie_case(oracle, p)
    cts = np.concatenate([words(4242, 2, p.n + 1), ct[None], words(4243, 3, p.n + 1)])
    return tv, bk, cts


def rotate_modes(oracle, p, cts, tv, bk, off):
    """(reference-mode, fused-mode) accumulators of the oracle."""
    out = []
    try:
        for mode in (0, 1):
            oracle.set_fused(mode)
            out.append(np.array([oracle.blind_rotate(p, x, tv, bk, off) for x in cts]))
    finally:
        oracle.set_fused(0)
    return out
