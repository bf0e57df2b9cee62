"""A 64-word client-encrypted memory read at a server-computed address in ONE bootstrap, on the MI355X: an extended
select node (LutCircuit.select with m = 64, eta = 2).

The client encrypts 64 words of 6 bits as ordinary TLWE ciphertexts (UINT4 key, message modulus 64) and, per read, a
base and an offset.  The server adds the two ciphertexts, which is the select node's own linear combination, and reads
the word at base + offset: the node's table is packed on the device from the 64 input wires, and the address is read
by the extended blind rotation on 4 accumulator components, whose mod switch rounds to 8,192 positions.  Without eta
a select node stops at 16 entries on this key; the nested lookup that reads 64 costs 9 bootstraps and 9 packs.

The sum stays below 64, like every carry-free digit sum: the bootstrap is negacyclic, so an address that crossed the
padding bit would read the negated word.  Outputs are digits at m = 64 again; feed them to eta = 2 nodes only after
a look at the noise rule (include/tfhe_gpu.h "Extended nodes").

    python examples/encrypted_table_64.py [--offsets 0 5 21] [--seed 2024] [--device 0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zig-tfhe_amd"))
import tfhe_amd  # noqa: E402

M, ETA = 64, 2


def build_circuit(reads: int) -> tfhe_amd.LutCircuit:
    """Inputs: the 64 words, then (base, offset) per read.  Outputs: the word at base + offset per read."""
    c = tfhe_amd.LutCircuit()
    words = [c.input() for _ in range(M)]
    ops = [(c.input(), c.input()) for _ in range(reads)]
    for base, offset in ops:
        c.output(c.select([(base, 1), (offset, 1)], words, eta=ETA))
    return c


def plan_reads(offsets):
    """One read per address a = 0 .. 63: the offset cycles through `offsets`, reduced so that base = a - offset >= 0."""
    addr = np.arange(M, dtype=np.uint32)
    off = np.array([offsets[a % len(offsets)] % (a + 1) for a in range(M)], np.uint32)
    return addr - off, off


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--offsets", type=int, nargs="+", default=[0, 5, 21])
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    print("=== TFHE read of a 64-word encrypted memory by one extended select node (MI355X) ===\n")
    t0 = time.perf_counter()
    ctx = tfhe_amd.Context("uint4", args.device)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    key = tfhe_amd.PackingKey.generate(ctx, sk, seed0=50_000)  # the set's own shape (5, 3), alpha_lv1
    print(f"Keys generated in {time.perf_counter() - t0:.2f} s\n")

    # the circuit has no ordinary node; the evaluator still takes a set
    tables = tfhe_amd.LutSet(ctx, tfhe_amd.lut_generate(ctx.params, M, lambda x: x))
    words = np.random.default_rng(args.seed).integers(0, M, M).astype(np.uint32)
    base, off = plan_reads(args.offsets)
    inputs = sk.encrypt_lwe_message(np.concatenate([words, np.stack([base, off], axis=1).reshape(-1)]), M, seed0=60_000)
    circuit = build_circuit(M)
    _, depth, groups = circuit.schedule_ext()
    print(f"memory: {words.tolist()}")
    print(f"{M} reads: {len(circuit.nodes)} select nodes of {M} entries, bootstrap depth {depth}, "
          f"eta groups per level {groups.tolist()}\n")

    t0 = time.perf_counter()
    out, _ = circuit.run(ctx, tables, inputs, packing_key=key)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"Evaluated in {ms:.1f} ms ({ctx.last_kernels()})\n")

    dec = sk.decrypt_lwe_message(out, M)
    want = words[base + off]
    for b, o, d, w in list(zip(base.tolist(), off.tolist(), dec.tolist(), want.tolist()))[::7]:
        print(f"  memory[{b:2d} + {o:2d}] = {d:2d}  (expected {w:2d})")
    wrong = np.flatnonzero(dec != want)
    ok = wrong.size == 0 and depth == 1
    tables.close()
    key.close()
    ctx.close()
    print(f"\n✓ Success! All {M} reads decrypt to the addressed word." if ok
          else f"\n✗ Error! Wrong reads at addresses {wrong.tolist()}.")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
