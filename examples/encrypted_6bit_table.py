"""A 6-bit-to-4-bit S-box (DES S1) on an encrypted 6-bit digit in ONE bootstrap, on the MI355X: the extended LUT
bootstrap (Context.lut_apply_ext).

UINT4's message room is 4 bits: at the message modulus m = 64 the blind rotation's own mod switch, which rounds
the n = 820 mask words to 2N = 2048 positions, throws one input in six off its block (1.4 sigma of margin).  The
extended bootstrap runs the blind rotation in Z[X]/(X^(4N) + 1) instead, kept as E = 4 accumulator components over
the ring of the key, so the mod switch rounds to 8192 positions (5.5 sigma, the margin of 4-bit digits today).  The
key and the transforms stay as they are; the price is 4 external products per step.  The outputs are encoded at
m = 64 again, so tables chain and digits add (radix-64 arithmetic).

    python examples/encrypted_6bit_table.py [--items 16] [--seed 2024] [--device 0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zig-tfhe_amd"))
import tfhe_amd  # noqa: E402

M, ETA = 64, 2

# FIPS 46-3, S1: the row is bits 1 and 6 of the input (most significant first), the column bits 2-5
S1_ROWS = [[14, 4, 13, 1, 2, 15, 11, 8, 3, 10, 6, 12, 5, 9, 0, 7],
           [0, 15, 7, 4, 14, 2, 13, 1, 10, 6, 12, 11, 9, 5, 3, 8],
           [4, 1, 14, 8, 13, 6, 2, 11, 15, 12, 9, 7, 3, 10, 5, 0],
           [15, 12, 8, 2, 4, 9, 1, 7, 5, 11, 3, 14, 10, 0, 6, 13]]


def des_s1(x: int) -> int:
    return S1_ROWS[(x >> 5) << 1 | (x & 1)][(x >> 1) & 15]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    print("=== TFHE 6-bit S-box in one extended LUT bootstrap (MI355X) ===\n")
    t0 = time.perf_counter()
    ctx = tfhe_amd.Context("uint4", args.device)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    print(f"Keys generated in {time.perf_counter() - t0:.2f} s\n")

    assert des_s1(0b011011) == 0b0101  # the textbook example
    # one extended table: E = 4 test vectors, component j = coefficients j, j + 4, ... of the degree-4096 table
    tables = tfhe_amd.LutSet(ctx, tfhe_amd.lut_generate_ext(ctx.params, ETA, M, des_s1))

    g = np.random.default_rng(args.seed)
    data = ([0b011011, 0, 63][:args.items] + [int(v) for v in g.integers(0, M, max(args.items - 3, 0))])
    B = len(data)
    pool = sk.encrypt_lwe_message(np.array(data, np.uint32), M, seed0=70_000)
    nodes = [(0, [(i, 1)], 0) for i in range(B)]
    print(f"{B} digits of 6 bits: {B} extended bootstraps, {1 << ETA} external products per step\n")

    t0 = time.perf_counter()
    out = ctx.lut_apply_ext(tables, ETA, pool, nodes)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"Evaluated in {ms:.1f} ms ({ctx.last_kernels()})\n")

    got = [int(v) for v in sk.decrypt_lwe_message(out, M)]
    for d, s in zip(data, got):
        print(f"  S1[{d:06b}] = {s:04b}  (expected {des_s1(d):04b})")
    ok = got == [des_s1(d) for d in data]
    tables.close()
    ctx.close()
    print("\n✓ Success! Encrypted S-box outputs computed correctly." if ok else "\n✗ Error! Result mismatch.")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
