"""Comparisons and pattern matching on encrypted bits on the MI355X, without a bootstrap: decision
diagrams evaluated by CMUXes (the leveled mode of TFHE).

  client  encrypts every bit of two 32-bit numbers, and of an 8-character string, as a TRGSW
          (TRGSWLv1.encryptTorus, trgsw.zig:35-71)
  server  a < b:    the comparator's diagram, 3 CMUXes per bit pair (CmuxGraph.less_than(32))
          match:    a DFA that accepts the strings containing "ab", unrolled over the 8 characters
                    (CmuxGraph.dfa, 8 bits per symbol)
          both through Context.cmux_graph with extract = 2: the results come out as TLWELv0, and
          an AND gate combines them like any other gate inputs
  client  decrypts

    python examples/encrypted_compare.py [--pairs 4] [--seed 2024] [--device 0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zig-tfhe_amd"))
import tfhe_amd  # noqa: E402
from tfhe_amd import CmuxGraph  # noqa: E402

WORDS = ["fabulous", "tabletop", "drawback", "absolute", "bathroom", "baseball", "xylitols", "aaaaaaab"]


def contains_ab_dfa():
    """States: 0 nothing yet, 1 the last character was 'a', 2 "ab" seen (accepting, a sink)."""
    delta = np.zeros((3, 256), int)
    delta[0, ord("a")] = delta[1, ord("a")] = 1
    delta[1, ord("b")] = 2
    delta[2, :] = 2
    return delta


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4, help="comparisons and strings (at most 8)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    Q = max(1, min(args.pairs, len(WORDS)))

    print("=== TFHE Encrypted Compare / Match Example (MI355X) ===\n")
    t0 = time.perf_counter()
    ctx = tfhe_amd.Context("128", args.device)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    print(f"Keys generated in {time.perf_counter() - t0:.2f} s\n")

    g = np.random.default_rng(args.seed)
    a = g.integers(0, 1 << 32, Q, dtype=np.uint64)
    b = np.where(g.integers(0, 2, Q) == 1, a, g.integers(0, 1 << 32, Q, dtype=np.uint64))  # some equal pairs
    b[0] = a[0] ^ np.uint64(1)  # and one that differs in the lowest bit only
    words = WORDS[:Q]

    # client: variable 2i of a comparison is bit 31 - i of a, variable 2i + 1 that bit of b;
    # variable 8p + j of a string is bit j of character p
    shifts = np.arange(31, -1, -1, dtype=np.uint64)
    cmp_bits = np.stack([(a[:, None] >> shifts) & np.uint64(1), (b[:, None] >> shifts) & np.uint64(1)], axis=2).reshape(Q, 64)
    chars = np.array([[ord(ch) for ch in w] for w in words])
    str_bits = ((chars[:, :, None] >> np.arange(8)) & 1).reshape(Q, 64)
    plain = np.concatenate([cmp_bits.astype(np.uint32), str_bits.astype(np.uint32)]).reshape(-1)
    selectors = tfhe_amd.TrgswSet(ctx, ctx.trgsw_encrypt(sk.key_lv1, plain, seed0=30_000))
    addr = np.arange(2 * Q * 64, dtype=np.uint32).reshape(2 * Q, 64)

    less, match = CmuxGraph.less_than(32), CmuxGraph.dfa(3, contains_ab_dfa(), {2}, 8, 8)
    for name, gr in (("a < b", less), ('contains "ab"', match)):
        _, _, depth, n_slots = gr.plan()
        print(f"{name:14s}: {gr.n_nodes} CMUXes per query in {depth} levels, {n_slots} scratch TRLWEs per query")

    leaves = CmuxGraph.bool_leaves(ctx.params.N)
    t0 = time.perf_counter()
    lt = ctx.cmux_graph(selectors, addr[:Q], less, leaves, extract=2)[:, 0]      # server
    kernels = ctx.last_kernels()
    hit = ctx.cmux_graph(selectors, addr[Q:], match, leaves, extract=2)[:, 0]
    both = ctx.gate_batch(np.full(Q, tfhe_amd.AND, np.uint8), lt, hit)          # gate inputs like any other
    ms = (time.perf_counter() - t0) * 1e3
    print(f"\n{2 * Q} graph evaluations and {Q} gates in {ms:.1f} ms  ({kernels})\n")

    got = np.stack([sk.decrypt_bool(x) for x in (lt, hit, both)], axis=1)       # client
    want = np.stack([a < b, np.array(["ab" in w for w in words]), (a < b) & np.array(["ab" in w for w in words])], axis=1)
    for q in range(Q):
        print(f"{int(a[q]):#010x} < {int(b[q]):#010x}: {bool(got[q, 0])!s:5}   "
              f'"ab" in "{words[q]}": {bool(got[q, 1])!s:5}   both: {bool(got[q, 2])!s:5}')
    ok = bool(np.array_equal(got, want))
    selectors.close()
    ctx.close()
    print("\n✓ Success! Every result matches the plaintext computation." if ok else "\n✗ Error! Result mismatch.")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
