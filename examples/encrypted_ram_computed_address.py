"""A read of a client-encrypted table by an address the server computed, on the MI355X: LutCircuit.select over
input wires.

The client encrypts 16 words of 4 bits as ordinary TLWE ciphertexts (UINT4, m = 16) and two digits a and b.  The
server computes the address (a + b) mod 16 by a bivariate node (LutCircuit.node2) and reads the word at that address
with a select node whose 16 entries are the client's ciphertexts themselves: the table is packed on the device from
the wires and the address digit is bootstrapped with it.  The leveled lookups (encrypted_ram.py) cannot do this:
their selectors are TRGSW ciphertexts only the client can make.  One circuit call, depth 3.

    python examples/encrypted_ram_computed_address.py [--reads 4] [--seed 2024] [--device 0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zig-tfhe_amd"))
import tfhe_amd  # noqa: E402

M = 16


def build_circuit(reads: int) -> tfhe_amd.LutCircuit:
    """Inputs: the 16 words, then (a, b) per read.  Outputs: the word at (a + b) mod 16 per read."""
    c = tfhe_amd.LutCircuit()
    words = [c.input() for _ in range(M)]
    ab = [(c.input(), c.input()) for _ in range(reads)]
    for a, b in ab:
        addr = c.node2(0, [(a, 1)], [(b, 1)], M)
        c.output(c.select([(addr, 1)], words))
    return c


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    print("=== TFHE read of an encrypted table by a server-computed address (MI355X) ===\n")
    t0 = time.perf_counter()
    ctx = tfhe_amd.Context("uint4", args.device)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    key = tfhe_amd.PackingKey.generate(ctx, sk, seed0=50_000)  # the set's own shape (5, 3), alpha_lv1
    print(f"Keys generated in {time.perf_counter() - t0:.2f} s\n")

    tables = tfhe_amd.LutSet(ctx, tfhe_amd.lut_generate2(ctx.params, M, lambda a, b: (a + b) % M))
    g = np.random.default_rng(args.seed)
    words = g.integers(0, M, M).astype(np.uint32)
    ab = g.integers(0, M, (args.reads, 2)).astype(np.uint32)
    inputs = sk.encrypt_lwe_message(np.concatenate([words, ab.reshape(-1)]), M, seed0=60_000)
    circuit = build_circuit(args.reads)
    _, depth = circuit.schedule()
    print(f"table: {words.tolist()}")
    print(f"{args.reads} reads: {len(circuit.nodes)} nodes, bootstrap depth {depth}\n")

    t0 = time.perf_counter()
    out, _ = circuit.run(ctx, tables, inputs, packing_key=key)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"Evaluated in {ms:.1f} ms ({ctx.last_kernels()})\n")

    dec = sk.decrypt_lwe_message(out, M)
    want = words[(ab[:, 0] + ab[:, 1]) % M]
    for (a, b), d, w in zip(ab.tolist(), dec.tolist(), want.tolist()):
        print(f"  table[({a:2d} + {b:2d}) mod 16] = {d:2d}  (expected {w:2d})")
    ok = np.array_equal(dec, want) and depth == 3
    tables.close()
    key.close()
    ctx.close()
    print("\n✓ Success! Every read decrypts to the addressed word." if ok else "\n✗ Error! Result mismatch.")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
