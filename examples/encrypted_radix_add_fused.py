"""8-bit + 8-bit on encrypted base-4 digits on the MI355X with ONE bootstrap per digit: the radix
adder of encrypted_radix_add.py through the multi-output LUT bootstrap.

There, message = s mod 4 and carry = s div 4 of the same s = a_i + b_i + carry are two nodes with the
same terms and two tables: two blind rotations.  Here the two tables are interleaved into one test
vector (tfhe_lut_interleave), the digit's s is rounded to a multiple of 2 positions (theta = 1) and ONE
blind rotation leaves the message at coefficient 0 and the carry at coefficient 1 of the accumulator;
both are extracted and key switched.  The price is one bit of message room: message modulus 8 instead
of 16 (2 message bits, 1 bit of carry room: s <= 3 + 3 + 1 = 7), at the same noise margin.

    python examples/encrypted_radix_add_fused.py [--pairs 4] [--seed 2024] [--device 0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zig-tfhe_amd"))
import tfhe_amd  # noqa: E402

M, DIGITS = 8, 4


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    print("=== TFHE Encrypted Radix Addition, fused message + carry (MI355X) ===\n")
    t0 = time.perf_counter()
    ctx = tfhe_amd.Context("uint4", args.device)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    print(f"Keys generated in {time.perf_counter() - t0:.2f} s\n")

    g = np.random.default_rng(args.seed)
    pairs = [(0xB7, 0x5E), (0xFF, 0xFF)][:args.pairs]
    pairs += [tuple(int(v) for v in g.integers(0, 256, 2)) for _ in range(args.pairs - len(pairs))]
    fused = tfhe_amd.lut_interleave(ctx.params, [tfhe_amd.lut_generate(ctx.params, M, lambda x: x % 4),    # coefficient 0
                                                 tfhe_amd.lut_generate(ctx.params, M, lambda x: x // 4)])  # coefficient 1
    tables = tfhe_amd.LutSet(ctx, [fused])

    circ = tfhe_amd.LutCircuit()
    ins = [[circ.input() for _ in range(2 * DIGITS)] for _ in pairs]
    for w in ins:
        circ.output(*circ.radix_add_fused(w[:DIGITS], w[DIGITS:], lut=0))
    levels, depth = circ.schedule()
    two_table = 2 * DIGITS * len(pairs)
    print(f"{len(pairs)} additions: {len(circ.nodes)} LUT nodes = {len(circ.nodes)} blind rotations in {depth} levels "
          f"(two-table form: {two_table} nodes = {two_table} blind rotations)\n")

    digits = lambda v: [(v >> (2 * i)) & 3 for i in range(DIGITS)]  # noqa: E731
    msgs = np.array([d for a, b in pairs for d in digits(a) + digits(b)], np.uint32)
    cts = sk.encrypt_lwe_message(msgs, M, seed0=10_000)

    t0 = time.perf_counter()
    out, ran = circ.run(ctx, tables, cts)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"Evaluated in {ms:.1f} ms ({ran} levels; {ctx.last_kernels()})\n")

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
