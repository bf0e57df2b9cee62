"""8-bit + 8-bit on encrypted base-4 digits on the MI355X: a radix adder as a LUT circuit.

Each number is four digits of 2 bits, encrypted under the UINT4 set with message modulus 16 (2
message bits and 2 bits of carry room; encryptLweMessage, tlwe.zig:74-88).  Encoder.encode is
message x scale (encoder.zig:66-73), so adding ciphertexts adds messages; per digit

    s = a_i + b_i + carry      (TLWELv0.add, on the device: no bootstrap)
    message = LUT_msg(s) = s mod 4,  carry = LUT_carry(s) = s div 4      (two programmable bootstraps)

The message and carry tables of one digit run in the SAME launch: every item of a batch picks its
own table of a resident set (tfhe_gpu_lut_set).  The whole adder is one call,
tfhe_gpu_lut_circuit_eval: 8 nodes in 4 levels per addition, every wire in HBM, and any number of
additions side by side in the same levels.

    python examples/encrypted_radix_add.py [--pairs 4] [--seed 2024] [--device 0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zig-tfhe_amd"))
import tfhe_amd  # noqa: E402

M, DIGITS = 16, 4


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    print("=== TFHE Encrypted Radix Addition Example (MI355X) ===\n")
    t0 = time.perf_counter()
    ctx = tfhe_amd.Context("uint4", args.device)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    print(f"Keys generated in {time.perf_counter() - t0:.2f} s\n")

    g = np.random.default_rng(args.seed)
    pairs = [(0xB7, 0x5E), (0xFF, 0xFF)][:args.pairs]
    pairs += [tuple(int(v) for v in g.integers(0, 256, 2)) for _ in range(args.pairs - len(pairs))]
    tables = tfhe_amd.LutSet(ctx, [tfhe_amd.lut_generate(ctx.params, M, lambda x: x % 4),    # table 0: message
                                   tfhe_amd.lut_generate(ctx.params, M, lambda x: x // 4)])  # table 1: carry

    # the circuit: every addition's digits are inputs, its 4 message digits + final carry are outputs
    circ = tfhe_amd.LutCircuit()
    ins = [[circ.input() for _ in range(2 * DIGITS)] for _ in pairs]
    for w in ins:
        circ.output(*circ.radix_add(w[:DIGITS], w[DIGITS:], msg_lut=0, carry_lut=1))
    levels, depth = circ.schedule()
    print(f"{len(pairs)} additions: {len(circ.nodes)} LUT nodes in {depth} levels "
          f"({int((levels == 1).sum())} nodes per level)\n")

    # client: base-4 digits, least significant first
    digits = lambda v: [(v >> (2 * i)) & 3 for i in range(DIGITS)]  # noqa: E731
    msgs = np.array([d for a, b in pairs for d in digits(a) + digits(b)], np.uint32)
    cts = sk.encrypt_lwe_message(msgs, M, seed0=10_000)

    # server
    t0 = time.perf_counter()
    out, ran = circ.run(ctx, tables, cts)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"Evaluated in {ms:.1f} ms ({ran} levels; {ctx.last_kernels()})\n")

    # client
    dec = sk.decrypt_lwe_message(out, M).reshape(len(pairs), DIGITS + 1)
    ok = True
    for (a, b), d in zip(pairs, dec):
        s = sum(int(x) << (2 * i) for i, x in enumerate(d))
        ok = ok and s == a + b
        print(f"  0x{a:02X} + 0x{b:02X} = 0x{s:03X}  (digits {[int(x) for x in d]}, expected 0x{a + b:03X})")
    tables.close()
    ctx.close()
    print("\n✓ Success! Encrypted additions computed correctly." if ok else "\n✗ Error! Result mismatch.")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
