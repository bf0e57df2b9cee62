"""The AES S-box on an encrypted byte held as two 4-bit digits, on the MI355X: a function of two full-width
digits through the bivariate LUT bootstrap (Context.lut_apply2).

A LUT node is a table over ONE combined input; a + 16 b does not fit the message room of UINT4 (m = 16).  The
tree-based functional bootstrap evaluates f(x, y) anyway: y goes through the 16 tables f(i, .), the 16 results are
packed into the coefficient slots of one TRLWE (the packing key switch), the slots are spread into a test vector
(lut_spread), and x is bootstrapped with that encrypted test vector.  The S-box has two output nibbles, so F = 2
functions: per byte 32 level-1 bootstraps, 2 packs and 2 level-2 bootstraps, all in one device call.  The inputs
are ordinary TLWE ciphertexts (fresh here; gate or LUT outputs work the same), not TRGSW-encrypted address bits
as in encrypted_sbox.py, and the outputs are two 4-bit digits again: S-boxes chain.

    python examples/encrypted_sbox_nibbles.py [--bytes 8] [--seed 2024] [--device 0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zig-tfhe_amd"))
import tfhe_amd  # noqa: E402

M = 16


def aes_sbox():
    """FIPS 197: the inverse in GF(2^8) mod x^8 + x^4 + x^3 + x + 1, then the affine map."""
    def mul(a, b):
        r = 0
        while b:
            if b & 1:
                r ^= a
            a = (a << 1) ^ (0x11B if a & 0x80 else 0)
            b >>= 1
        return r
    box = []
    for v in range(256):
        inv = next((c for c in range(1, 256) if mul(v, c) == 1), 0)
        rot = lambda x, k: ((x << k) | (x >> (8 - k))) & 0xFF  # noqa: E731
        box.append(inv ^ rot(inv, 1) ^ rot(inv, 2) ^ rot(inv, 3) ^ rot(inv, 4) ^ 0x63)
    return box


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=8)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    print("=== TFHE AES S-box on two encrypted nibbles, bivariate LUT bootstrap (MI355X) ===\n")
    t0 = time.perf_counter()
    ctx = tfhe_amd.Context("uint4", args.device)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    key = tfhe_amd.PackingKey.generate(ctx, sk, seed0=50_000)  # the set's own shape (5, 3), alpha_lv1
    print(f"Keys generated in {time.perf_counter() - t0:.2f} s\n")

    sbox = aes_sbox()
    assert sbox[0x00] == 0x63 and sbox[0x53] == 0xED
    # x = the high nibble, y = the low one; function 0 gives the output's high nibble, function 1 its low one
    tables = tfhe_amd.LutSet(ctx, np.concatenate([
        tfhe_amd.lut_generate2(ctx.params, M, lambda x, y: sbox[16 * x + y] >> 4),
        tfhe_amd.lut_generate2(ctx.params, M, lambda x, y: sbox[16 * x + y] & 15)]))

    g = np.random.default_rng(args.seed)
    data = [0x00, 0x53, 0xFF][:args.bytes] + [int(v) for v in g.integers(0, 256, max(args.bytes - 3, 0))]
    B = len(data)
    msgs = np.array([d >> 4 for d in data] + [d & 15 for d in data], np.uint32)  # pool: B high nibbles, B low ones
    pool = sk.encrypt_lwe_message(msgs, M, seed0=60_000)
    at = np.arange(B, dtype=np.uint32)
    nodes = (np.repeat(np.array([0, 1], np.uint32), B), np.tile(at, 2), np.tile(at + B, 2))
    print(f"{B} bytes: {2 * B} bivariate nodes = {2 * B * M} level-1 bootstraps, {2 * B} packs of {M} slots, "
          f"{2 * B} spreads, {2 * B} level-2 bootstraps\n")

    t0 = time.perf_counter()
    out = ctx.lut_apply2(tables, key, M, pool, nodes)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"Evaluated in {ms:.1f} ms ({ctx.last_kernels()})\n")

    dec = sk.decrypt_lwe_message(out, M)
    got = [int(dec[b]) << 4 | int(dec[B + b]) for b in range(B)]
    for d, s in zip(data, got):
        print(f"  S[0x{d:02X}] = 0x{s:02X}  (expected 0x{sbox[d]:02X})")
    ok = got == [sbox[d] for d in data]
    tables.close()
    key.close()
    ctx.close()
    print("\n✓ Success! Encrypted S-box outputs computed correctly." if ok else "\n✗ Error! Result mismatch.")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
