"""The whole form's blind-rotation kernels after their LDS reads were rescheduled:
k_blind_rotate_assist<true> and k_blind_rotate_assist<true,TV> at the 128- and 80-bit sets with
B = 3 and B = 5 (one and three idle gate slots, one and two workgroups), and the L = 1 and L = 2
whole-form kernels, which share the pipelined transform pair, at B = 3.  Every word is compared
with the oracle: the schedule of a wave's table reads must not change one bit.  The references
are computed once per module (the L = 1, 2 ones are test_param_sets' own)."""
import numpy as np
import pytest

import tfhe_amd
from conftest import get_keys, rng
from test_lut_circuit import oracle_nodes, tables_for
from test_param_sets import br_case, ctx_for as ctx_for_set

pytestmark = pytest.mark.gpu

_CTX, _CACHE = {}, {}


def ctx_for(oracle, pname):
    """Context with the oracle's seeded cloud key loaded (sk 42, ck 43)."""
    if pname not in _CTX:
        k = get_keys(oracle, pname)
        c = tfhe_amd.Context(pname, 0)
        c.load_cloud_key(k.ck.offset, k.ck.testvec, k.ck.bk, k.ck.ksk)
        _CTX[pname] = (c, k)
    return _CTX[pname]


def rotation_case(oracle, pname):
    """5 uniform TLWEs (bit-exactness only) and the oracle's rotations of them."""
    if ("br", pname) not in _CACHE:
        _, k = ctx_for(oracle, pname)
        cts = rng(1900).integers(0, 1 << 32, (5, k.p.n + 1), dtype=np.uint64).astype(np.uint32)
        want = np.array([oracle.blind_rotate(k.p, t, k.ck.testvec, k.ck.bk, k.ck.offset) for t in cts])
        _CACHE["br", pname] = (cts, want)
    return _CACHE["br", pname]


def table_case(oracle, pname):
    """5 nodes over 4 fresh encryptions and 3 tables of m = 4; neighbours use different tables."""
    if ("lut", pname) not in _CACHE:
        c, k = ctx_for(oracle, pname)
        sk = tfhe_amd.SecretKey(c.params, k.k0, k.k1)
        g = rng(1901)
        pool = sk.encrypt_lwe_message(g.integers(0, 2, 4).astype(np.uint32), 4, seed0=1902)
        nodes = [((2 * i + 1) % 3, [(int(g.integers(0, 4)), int(g.integers(-2, 5))) for _ in range(1 + i % 2)],
                  (1 << 29) if i == 3 else 0) for i in range(5)]
        tables = tables_for(c.params, 4, 3)
        _CACHE["lut", pname] = (pool, nodes, tables, oracle_nodes(oracle, k.p, k.ck, pool, nodes, tables))
    return _CACHE["lut", pname]


@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("pname", ["128", "80"])
def test_assist_rotation_vs_oracle(oracle, pname, B):
    c, _ = ctx_for(oracle, pname)
    cts, want = rotation_case(oracle, pname)
    with c.options(br_form="whole"):
        got = c.blind_rotate_batch(cts[:B])
        assert c.last_kernels().startswith("k_blind_rotate_assist<true> "), c.last_kernels()
    assert got.shape == want[:B].shape
    bad = np.flatnonzero((got != want[:B]).any(axis=1))
    assert bad.size == 0, bad.tolist()


@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("pname", ["128", "80"])
def test_assist_per_item_tables_vs_oracle(oracle, pname, B):
    c, _ = ctx_for(oracle, pname)
    pool, nodes, tables, want = table_case(oracle, pname)
    ls = tfhe_amd.LutSet(c, tables)
    try:
        with c.options(br_form="whole"):
            got = c.lut_apply(ls, pool, nodes[:B])
            assert c.last_kernels().startswith("k_blind_rotate_assist<true,TV>"), c.last_kernels()
    finally:
        ls.close()
    assert got.shape == want[:B].shape
    bad = np.flatnonzero((got != want[:B]).any(axis=1))
    assert bad.size == 0, bad.tolist()


@pytest.mark.parametrize("pname,kernel", [("uint2", "k_blind_rotate<1,"), ("l2small", "k_blind_rotate<2,true,true>")])
def test_whole_form_pair_kernels_at_l1_and_l2(oracle, pname, kernel):
    c, _ = ctx_for_set(oracle, pname)
    cts, want = br_case(oracle, pname)
    with c.options(br_form="whole"):
        got = c.blind_rotate_batch(cts[:3])
        assert c.last_kernels().startswith(kernel), c.last_kernels()
    assert np.array_equal(got, want[:3])
