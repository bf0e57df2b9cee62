"""The packed scatter-add's definition on the CPU (include/tfhe_gpu.h, tfhe_gpu_packed_scatter_add_batch), built
from oracle.cmux, oracle.poly_mul_with_xk, oracle.external_product and numpy's wrapping u32 adds.  Shared by
tests/test_packed_write_cpu.py, which checks it by decryption, and tests/test_packed_write.py, which compares the
GPU's words with it."""
import numpy as np


def rotate_to_slot(oracle, p, off, trgsw, plan, delta, addr_row):
    """d <- cmux(d, X^(stride * 2^j) d, set[addr[j]]) for j = 0 .. h-1, in order."""
    N = p.N
    d = np.array(delta, np.uint32)
    for j in range(plan.h):
        r = plan.stride << j
        turned = np.concatenate([oracle.poly_mul_with_xk(d[:N], r), oracle.poly_mul_with_xk(d[N:], r)])
        d = oracle.cmux(p, d, turned, trgsw[addr_row[j]], off)
    return d


def demux(oracle, p, off, trgsw, v, k, d, addr_row):
    """Level l under address bit k-1-l: node i with value x has the children 2i+1 = hi = ExtProd(selector, x) and
    2i = lo = x - hi.  -> the 2^v leaves."""
    nodes = [np.array(d, np.uint32)]
    for l in range(v):
        sel = trgsw[addr_row[k - 1 - l]]
        nxt = []
        for x in nodes:
            hi = oracle.external_product(p, sel, x, off)
            nxt += [(x - hi).astype(np.uint32), hi]
        nodes = nxt
    return nodes


def scatter_leaves(oracle, p, off, trgsw, plan, k, delta, addr_row):
    return demux(oracle, p, off, trgsw, plan.v, k, rotate_to_slot(oracle, p, off, trgsw, plan, delta, addr_row), addr_row)


def scatter_add(oracle, p, off, trgsw, plan, k, deltas, addr, table):
    """table[i] += sum over q of leaf i of query q, wrapping u32.  -> the new table."""
    out = np.array(table, np.uint32).reshape(plan.trlwes, 2 * p.N).copy()
    for q in range(len(addr)):
        for i, leaf in enumerate(scatter_leaves(oracle, p, off, trgsw, plan, k, deltas[q], addr[q])):
            out[i] += leaf
    return out


def trlwe_phase(oracle, N, ct, k1):
    """b - a * s as signed fractions of the torus."""
    ph = (ct[N:] - oracle.poly_mul(ct[:N], k1)).astype(np.uint32)
    return ph.view(np.int32).astype(np.float64) / 2.0 ** 32
