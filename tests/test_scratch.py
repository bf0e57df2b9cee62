"""The scratch arena under the host paths (csrc/tfhe_scratch.hpp) at the 128-bit set: every case
runs the same seeded inputs through a long-lived context, whose arena grows, coalesces and is reused from call to
call, and through a context that sees only that one call, and requires equal words (np.array_equal).  Inputs,
tables, selectors and packing-key rows are seeded random words: only bit equality is asked, never a decryption.

Every context here gets the session's cloud key device-to-device (export_key_device / import_key_device) from one
donor, not through load_cloud_key: a host key load stages 69 MB of BK in the arena, after which none of these
small calls would make it grow, and the cases are about growth."""
import numpy as np
import pytest

import tfhe_amd
from conftest import rng

pytestmark = pytest.mark.gpu

N = 1024
_DONOR = {}


def words(seed, *shape):
    return rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def new_ctx(keys128):
    """A context at the 128-bit set with the cached cloud key, its arena untouched."""
    import torch
    if not _DONOR:
        d = tfhe_amd.Context("128", 0)
        d.load_cloud_key(keys128.ck.offset, keys128.ck.testvec, keys128.ck.bk, keys128.ck.ksk)
        nb, nk = d.key_blob_bytes()
        bk = torch.empty(nb, dtype=torch.uint8, device="cuda:0")
        ksk = torch.empty(nk, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        off, tv = d.export_key_device(bk.data_ptr(), ksk.data_ptr())
        d.close()
        _DONOR.update(bk=bk, ksk=ksk, off=off, tv=tv)
    c = tfhe_amd.Context("128", 0)
    c.import_key_device(_DONOR["bk"].data_ptr(), _DONOR["ksk"].data_ptr(), _DONOR["off"], _DONOR["tv"])
    return c


def alone(keys128, call):
    """call(context) on a context that sees nothing else."""
    c = new_ctx(keys128)
    try:
        return call(c)
    finally:
        c.close()


def gates(seed, B, n1):
    return (rng(seed).integers(0, 10, B).astype(np.uint8), words(seed + 1, B, n1), words(seed + 2, B, n1))


# ---- 1. grow, then shrink, through host entries ----------------------------------------------------
def test_gate_batch_grows_then_shrinks(keys128):
    """B = 3, 70, 3: the second call needs new blocks, the third opens on the coalesced one."""
    long = new_ctx(keys128)
    try:
        for i, B in enumerate((3, 70, 3)):
            ops, a, b = gates(100 + 10 * i, B, long.n1)
            got = long.gate_batch(ops, a, b)
            assert got.any() and np.array_equal(got, alone(keys128, lambda c: c.gate_batch(ops, a, b))), B
    finally:
        long.close()


# ---- 2. multi-output LUT nodes: the extractions are taken before the bootstrap takes its own --------
def test_lut_apply_multi_nodes(keys128):
    """theta = 1 on every node, B = 2, 9, 2 (2B outputs): lut_multi_launch holds its accumulators and extractions
    across run_bootstrap_dev's nested frame."""
    tables, pool = words(200, 4, 2 * N), None
    long = new_ctx(keys128)
    ls = tfhe_amd.LutSet(long, tables)
    try:
        pool = words(201, 5, long.n1)
        for i, B in enumerate((2, 9, 2)):
            nodes = [((j + i) % 4, [(j % 5, 1), ((j + 2) % 5, 3)], 7 * j + i) for j in range(B)]
            theta = np.ones(B, np.uint32)
            got = long.lut_apply_multi(ls, pool, nodes, theta)
            assert got.shape == (2 * B, long.n1)

            def one(c):
                s = tfhe_amd.LutSet(c, tables)
                try:
                    return c.lut_apply_multi(s, pool, nodes, theta)
                finally:
                    s.close()
            assert got.any() and np.array_equal(got, alone(keys128, one)), B
    finally:
        ls.close()
        long.close()


# ---- 3. bivariate nodes: pack frames nested in the call's ------------------------------------------
def test_lut_apply2_nested_pack_frames(keys128):
    """m = 2, B = 1, then 6 under TFHE_OPT_PACK_SCRATCH_MB = 1.  At m = 2 six nodes are 12 items, whose sums fit
    1 MB, so a third call with B = 40 (80 items; 1 MB holds the sums of 32) makes the pack, and with it the node
    loop, really go in chunks."""
    m, basebit, t = 2, 2, 8
    long = new_ctx(keys128)
    p = long.params
    rows = words(300, p.n * t << basebit, 2 * N)  # any rows: the key's shape is what the GEMM needs
    tables, pool = words(301, 2 * m, 2 * N), words(302, 6, long.n1)
    ls, key = tfhe_amd.LutSet(long, tables), tfhe_amd.PackingKey(long, rows, basebit, t)
    try:
        for i, (B, mb) in enumerate(((1, 256), (6, 1), (40, 1))):
            g = rng(310 + i)
            nodes = (g.integers(0, 2, B).astype(np.uint32), g.integers(0, 6, B).astype(np.uint32),
                     g.integers(0, 6, B).astype(np.uint32))
            with long.options(pack_scratch_mb=mb):
                got = long.lut_apply2(ls, key, m, pool, nodes)

            def one(c):
                s, k = tfhe_amd.LutSet(c, tables), tfhe_amd.PackingKey(c, rows, basebit, t)
                try:
                    return c.lut_apply2(s, k, m, pool, nodes)  # unchunked: chunking changes no word
                finally:
                    s.close()
                    k.close()
            assert got.any() and np.array_equal(got, alone(keys128, one)), B
    finally:
        ls.close()
        key.close()
        long.close()


# ---- 4. leveled calls on one context, no cloud key -------------------------------------------------
def test_leveled_calls_share_one_arena():
    """table_lookup k = 3, Q = 1; packed_lookup Q = 5; packed_scatter_add Q = 5 under TFHE_OPT_SCATTER_SCRATCH_MB
    = 1; table_lookup again.  The packed table has 13 address bits of 4-bit entries, so 32 TRLWEs (v = 5): a
    query's leaves are 256 KB and 1 MB holds 4 queries' — the five go in two chunks."""
    k, width, Q = 13, 4, 5
    long = tfhe_amd.Context("128", 0)
    p = long.params
    plan = tfhe_amd.packed_lookup_plan(p, k, width)
    assert plan.v >= 1 and plan.h >= 1 and (1 << 20) // ((1 << plan.v) * 8 * N) < Q
    trgsw = rng(400).integers(-(1 << 20), 1 << 20, (2, 2 * p.L, 2, N)).astype(np.float64)
    small, big = words(401, 8, 2 * N), words(402, plan.trlwes, 2 * N)
    addr3, addr = rng(403).integers(0, 2, (1, 3)).astype(np.uint32), rng(404).integers(0, 2, (Q, k)).astype(np.uint32)
    deltas = words(405, Q, 2 * N)
    calls = [
        lambda c, s: c.table_lookup(s, addr3, small),
        lambda c, s: c.packed_lookup(s, addr, width, big),
        lambda c, s: c.packed_scatter_add(s, addr, width, deltas, big),
        lambda c, s: c.table_lookup(s, addr3[:, ::-1], small),
    ]
    sel = tfhe_amd.TrgswSet(long, trgsw)
    try:
        for i, call in enumerate(calls):
            with long.options(scatter_scratch_mb=1 if i == 2 else 256):
                got = call(long, sel)
            c = tfhe_amd.Context("128", 0)
            s = tfhe_amd.TrgswSet(c, trgsw)
            try:
                assert got.any() and np.array_equal(got, call(c, s)), i
            finally:
                s.close()
                c.close()
    finally:
        sel.close()
        long.close()


# ---- 5. coalesce while work is in flight -----------------------------------------------------------
def test_coalesce_under_a_running_dev_call(keys128):
    """gate_batch_dev B = 8 on torch tensors with no synchronisation after it, then at once the host gate_batch
    with B = 300, which outgrows what the first call left; and the same pair again (B = 8 on the device, B = 3 on
    the host), whose host call opens on the several blocks the growth left and frees them while the device call's
    kernels may still run.  Then synchronise and compare all four outputs."""
    import torch
    long = new_ctx(keys128)
    n1 = long.n1
    try:
        dev_in = [gates(500, 8, n1), gates(510, 8, n1)]
        host_in = [gates(520, 300, n1), gates(530, 3, n1)]
        t = [[torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to("cuda:0") for x in g] for g in dev_in]
        outs = [torch.full((8, n1), -1, dtype=torch.int32, device="cuda:0") for _ in dev_in]
        torch.cuda.synchronize()
        host_got = []
        for (ops, a, b), out, h in zip(t, outs, host_in):
            long.gate_batch_dev(ops.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), 8)
            host_got.append(long.gate_batch(*h))
        long.sync()
        for g, out, h, got in zip(dev_in, outs, host_in, host_got):
            assert np.array_equal(out.cpu().numpy().view(np.uint32), alone(keys128, lambda c: c.gate_batch(*g)))
            assert got.any() and np.array_equal(got, alone(keys128, lambda c: c.gate_batch(*h)))
    finally:
        long.close()
