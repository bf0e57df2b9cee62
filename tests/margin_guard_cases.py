"""Fixtures of the margin-guard tests over the crafted key of
conftest.crafted_near_tie_case: constant test vector offset/2, BK[0]'s rows all FFT(2^31 - 1), the
other steps zero.  Under that key only step 0 of a blind rotation computes anything, and what it
computes depends on two numbers: a~_0 (word 0 after the modulus switch) and b~ (word n).

 - a HOT ciphertext has a~_0 = N and b~ in {0, 2N}: tmp = X^N acc - acc = -offset on every
   coefficient, every digit is -32, and the fused arithmetic rounds near a tie and parts from the
   reference's trees.  Words 1 .. n-1 are free (their BK rows are zero).
 - a QUIET ciphertext has a~_0 in {0, 2N}: tmp = 0, the external product is exactly zero, and
   nothing but exact integers is ever rounded, whatever the test vector.  No fused form flags it.

test_margin_guard_cpu.py proves both statements with the oracle; test_margin_guard.py builds its
batches out of them, so it knows which items the guard must recompute and which it must not."""
import numpy as np

from conftest import crafted_near_tie_case, rng

COPY = 255
GATE_OPS = list(range(10)) + [COPY]
# gate_combine(op, a, b) = sa * a + sb * b + const(op) on word n (gates.zig:48-121)
GATE_COEFS = {0: (-1, -1), 1: (1, 1), 2: (1, 1), 3: (1, 2), 4: (1, -2), 5: (-1, -1), 6: (-1, 1), 7: (1, -1),
              8: (-1, 1), 9: (1, -1), COPY: (1, 0)}
MASK = (1 << 32) - 1
# test_param_sets.SYNTHETIC["l2small"]: the one L = 2 set in the exact-integer regime (fused kernels <2,true,true>)
L2SMALL = dict(n=600, N=1024, nbit=10, L=2, bgbit=6, basebit=3, iks_t=4,
               alpha_lv0=2.0e-5, alpha_lv1=2.0e-8, alpha_ksk=2.0e-5, alpha_bsk=2.0e-8)


def oracle_params(name):
    """OracleParams of "128" or "l2small"."""
    from oracle import OracleParams, params
    return OracleParams(**L2SMALL) if name == "l2small" else params(name)


def switched(word) -> int:
    """a~ of a word: (a + 2^20) >> 21 in 64 bits (trgsw.zig:297), 0 .. 2N."""
    return (int(word) + (1 << 20)) >> 21


def word_rounding_to(g, centre: int) -> int:
    """A random word of the 2^21 words the modulus switch rounds to `centre` (0 stands for 0 and 2N)."""
    return ((centre << 21) + int(g.integers(-(1 << 20), 1 << 20))) & MASK


def is_hot(p, ct) -> bool:
    return switched(ct[0]) == p.N and switched(ct[p.n]) in (0, 2 * p.N)


def is_quiet(p, ct) -> bool:
    return switched(ct[0]) in (0, 2 * p.N)


def words(g, *shape):
    return g.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def hot_ct(p, seed, w0=None, wn=None):
    """Random words; word 0 = w0 (default: random in the window that rounds to N), word n = wn (default:
    random in the window that rounds to 0 or 2N)."""
    g = rng(seed)
    ct = words(g, p.n + 1)
    ct[0] = word_rounding_to(g, p.N) if w0 is None else w0
    ct[p.n] = word_rounding_to(g, 0) if wn is None else wn
    assert is_hot(p, ct)
    return ct


def quiet_ct(p, seed):
    """Random words; word 0 random in the window that rounds to 0 or 2N."""
    g = rng(seed)
    ct = words(g, p.n + 1)
    ct[0] = word_rounding_to(g, 0)
    assert is_quiet(p, ct) and not is_hot(p, ct)
    return ct


def solve_gate_pair(oracle, p, op, target, b):
    """a with oracle.gate_combine(p, op, a, b) == target on all n + 1 words (a's coefficient is +-1)."""
    sa, sb = GATE_COEFS[op]
    zero = np.zeros(p.n + 1, np.uint32)
    t = target.astype(np.int64) - oracle.gate_combine(p, op, zero, zero).astype(np.int64)  # minus the constant
    a = ((sa * (t - sb * b.astype(np.int64))) & MASK).astype(np.uint32)
    assert np.array_equal(oracle.gate_combine(p, op, a, b), target), op
    return a


def hot_gate_pair(oracle, p, op, seed):
    """(a, b), b random, whose gate pre-combination is hot_ct(p, seed) word for word."""
    b = words(rng(seed + 500_000), p.n + 1)
    return solve_gate_pair(oracle, p, op, hot_ct(p, seed), b), b


# The pools: every hot and quiet ciphertext the GPU tests use is one of these (a batch cycles through
# them), so the CPU test can prove each of them hot or quiet with the oracle.  The explicit words are
# the edges of the two rounding windows.
HOT_POOL = [(None, None), (0x80080000, 0), (0x7FF00000, 0xFFFFFFFF), (0x80000000, 0xFFFFF), (0x800FFFFF, 0xFFF00000),
            (None, None), (None, None), (None, None)]
QUIET_POOL = [None, 0, 0xFFFFF, 0xFFF00000, None, None, None, None]


def hot(p, j):
    """Hot ciphertext j of the pool (cyclic)."""
    j %= len(HOT_POOL)
    return hot_ct(p, 7000 + j, *HOT_POOL[j])


def quiet(p, j):
    """Quiet ciphertext j of the pool (cyclic)."""
    j %= len(QUIET_POOL)
    ct = quiet_ct(p, 7100 + j)
    if QUIET_POOL[j] is not None:
        ct[0] = QUIET_POOL[j]
    assert is_quiet(p, ct)
    return ct


def ct_items(p, B, hot_at, first=0):
    """(B, n + 1): pool ciphertexts, hot ones at the indices `hot_at`, quiet ones elsewhere; item i is
    pool entry first + i, so neighbours differ."""
    hot_at = set(int(i) for i in hot_at)
    return np.array([hot(p, first + i) if i in hot_at else quiet(p, first + i) for i in range(B)])


def gate_items(oracle, p, ops, hot_at, seed):
    """(A, B) of a gate batch with ops[i] on item i, whose pre-combinations are ct_items(p, len(ops),
    hot_at) word for word; the b operands are random (seed + i)."""
    target = ct_items(p, len(ops), hot_at)
    Bv = np.array([words(rng(seed + i), p.n + 1) for i in range(len(ops))])
    A = np.array([solve_gate_pair(oracle, p, int(op), t, b) for op, t, b in zip(ops, target, Bv)])
    return A, Bv


class oracle_arith:
    """`with oracle_arith(oracle, fused, regroup):` runs the oracle in that arithmetic and puts the
    reference's trees back.  regroup: 0 the whole form's MAC order, 2 the latency form's."""

    def __init__(self, oracle, fused, regroup=0):
        self.o, self.fused, self.regroup = oracle, fused, regroup

    def __enter__(self):
        self.o.set_fused(self.fused)
        self.o.set_regroup(self.regroup if self.fused else 0)

    def __exit__(self, *exc):
        self.o.set_fused(0)
        self.o.set_regroup(0)


FORM_REGROUP = {"auto": 2, "wide": 2, "whole": 0}  # auto below 512 items is the latency form


def rotate(oracle, p, cts, tvs, bk, off, fused=0, regroup=0):
    """The oracle's accumulators (B, 2N); tvs one test vector (2N,) or one per item (B, 2N)."""
    tvs = np.asarray(tvs, np.uint32)
    with oracle_arith(oracle, fused, regroup):
        return np.array([oracle.blind_rotate(p, ct, np.ascontiguousarray(tvs if tvs.ndim == 1 else tvs[i]), bk, off)
                         for i, ct in enumerate(cts)])


def crafted_key(oracle, p):
    """(offset, testvec, bk) of conftest.crafted_near_tie_case."""
    tv, bk, _ = crafted_near_tie_case(oracle, p)
    return oracle.decomposition_offset(p), tv, bk
