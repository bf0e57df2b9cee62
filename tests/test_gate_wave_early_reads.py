"""The L = 3 whole form after its gate wave's twist factors became resident and its tB words joined
the hand-off counter's LDS batch (DESIGN.md §4.1b "Gate-wave early reads"): k_blind_rotate_assist<true>
under mixed gate ops and k_blind_rotate_assist<true,TV> under per-item tables, at the 128- and
80-bit sets, with B = 1 (a lone gate beside three idle slots), 4 (a full workgroup), 5 (one gate
wave beside three idle ones in a second workgroup) and 9 (a ragged third workgroup).  Every word is
compared with the oracle, the kernel name says which form ran, and the device error word is zero
after each call (Context.sync raises otherwise).  No wait is steered: the spin cap stays at its
default.  The references are computed once per module."""
import numpy as np
import pytest

import tfhe_amd
from conftest import rng
from test_assist_schedule import ctx_for
from test_lut_circuit import oracle_nodes, tables_for

pytestmark = pytest.mark.gpu

SHAPES = [1, 4, 5, 9]
_CACHE = {}


def gate_case(oracle, pname):
    """9 gates, nine of the ten reference ops, over uniform TLWEs (bit-exactness only)."""
    if ("gates", pname) not in _CACHE:
        _, k = ctx_for(oracle, pname)
        g = rng(2100)
        a = g.integers(0, 1 << 32, (9, k.p.n + 1), dtype=np.uint64).astype(np.uint32)
        b = g.integers(0, 1 << 32, (9, k.p.n + 1), dtype=np.uint64).astype(np.uint32)
        ops = np.array([3, 0, 7, 1, 9, 4, 2, 8, 5], dtype=np.uint8)
        _CACHE["gates", pname] = (ops, a, b, oracle.gate_batch(k.p, ops, a, b, k.ck, threads=4))
    return _CACHE["gates", pname]


def table_case(oracle, pname):
    """9 nodes over 4 fresh encryptions and 3 tables of m = 4; neighbours use different tables."""
    if ("lut", pname) not in _CACHE:
        c, k = ctx_for(oracle, pname)
        sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
        g = rng(2101)
        pool = sk.encrypt_lwe_message(g.integers(0, 2, 4).astype(np.uint32), 4, seed0=2102)
        nodes = [((2 * i + 1) % 3, [(int(g.integers(0, 4)), int(g.integers(-2, 5))) for _ in range(1 + i % 2)],
                  (1 << 29) if i == 3 else 0) for i in range(9)]
        tables = tables_for(c.params, 4, 3)
        _CACHE["lut", pname] = (pool, nodes, tables, oracle_nodes(oracle, k.p, k.ck, pool, nodes, tables))
    return _CACHE["lut", pname]


@pytest.mark.parametrize("B", SHAPES)
@pytest.mark.parametrize("pname", ["128", "80"])
def test_mixed_gates_vs_oracle(oracle, pname, B):
    c, _ = ctx_for(oracle, pname)
    ops, a, b, want = gate_case(oracle, pname)
    assert c.get_option("br_spin_cap") == 0
    with c.options(br_form="whole"):
        got = c.gate_batch(ops[:B], a[:B], b[:B])
        kernels = c.last_kernels()
        c.sync()  # the device error word: a wait that gave up fails here
    assert "assist" in kernels and kernels.startswith("k_blind_rotate_assist<true> "), kernels
    assert got.shape == want[:B].shape
    bad = np.flatnonzero((got != want[:B]).any(axis=1))
    assert bad.size == 0, bad.tolist()


@pytest.mark.parametrize("B", SHAPES)
@pytest.mark.parametrize("pname", ["128", "80"])
def test_per_item_tables_vs_oracle(oracle, pname, B):
    c, _ = ctx_for(oracle, pname)
    pool, nodes, tables, want = table_case(oracle, pname)
    assert c.get_option("br_spin_cap") == 0
    ls = tfhe_amd.LutSet(c, tables)
    try:
        with c.options(br_form="whole"):
            got = c.lut_apply(ls, pool, nodes[:B])
            kernels = c.last_kernels()
            c.sync()
    finally:
        ls.close()
    assert "assist" in kernels and kernels.startswith("k_blind_rotate_assist<true,TV>"), kernels
    assert got.shape == want[:B].shape
    bad = np.flatnonzero((got != want[:B]).any(axis=1))
    assert bad.size == 0, bad.tolist()
