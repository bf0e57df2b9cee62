"""S[x ^ k], the AES S-box after a key addition, on encrypted bytes held as two 4-bit digits, on the MI355X: one
LUT-circuit call whose bivariate nodes are select nodes (LutCircuit.node2).

A byte x and a key byte k are two digits each at the full message modulus of UINT4 (m = 16).  The nibble XOR is a
function of two full-width digits, and so is each output nibble of the S-box: four node2 per byte, each 16 ordinary
nodes over one digit feeding one select node over the other, whose table is packed on the device from those 16
wires.  The XORed nibbles never leave the device: the circuit evaluator routes them into the S-box nodes, level by
level, every level's ordinary and select nodes in one blind-rotation launch.  Depth 4 for any number of bytes.

    python examples/encrypted_sbox_circuit.py [--bytes 4] [--seed 2024] [--device 0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zig-tfhe_amd"))
import tfhe_amd  # noqa: E402

M = 16
XOR, SBOX_HI, SBOX_LO = 0, M, 2 * M  # where each function's 16 tables start in the set


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


def build_circuit(n_bytes: int) -> tfhe_amd.LutCircuit:
    """Inputs per byte: x high, x low, k high, k low.  Outputs per byte: S[x ^ k] high, low."""
    c = tfhe_amd.LutCircuit()
    wires = [c.input() for _ in range(4 * n_bytes)]
    for b in range(n_bytes):
        xh, xl, kh, kl = wires[4 * b:4 * b + 4]
        th = c.node2(XOR, [(xh, 1)], [(kh, 1)], M)
        tl = c.node2(XOR, [(xl, 1)], [(kl, 1)], M)
        c.output(c.node2(SBOX_HI, [(th, 1)], [(tl, 1)], M), c.node2(SBOX_LO, [(th, 1)], [(tl, 1)], M))
    return c


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=4)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    print("=== TFHE S[x ^ k] on encrypted nibbles, one LUT circuit of select nodes (MI355X) ===\n")
    t0 = time.perf_counter()
    ctx = tfhe_amd.Context("uint4", args.device)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    key = tfhe_amd.PackingKey.generate(ctx, sk, seed0=50_000)  # the set's own shape (5, 3), alpha_lv1
    print(f"Keys generated in {time.perf_counter() - t0:.2f} s\n")

    sbox = aes_sbox()
    assert sbox[0x00] == 0x63 and sbox[0x53] == 0xED
    tables = tfhe_amd.LutSet(ctx, np.concatenate([
        tfhe_amd.lut_generate2(ctx.params, M, lambda a, b: a ^ b),
        tfhe_amd.lut_generate2(ctx.params, M, lambda h, lo: sbox[16 * h + lo] >> 4),
        tfhe_amd.lut_generate2(ctx.params, M, lambda h, lo: sbox[16 * h + lo] & 15)]))

    g = np.random.default_rng(args.seed)
    xs = [0x00, 0x53][:args.bytes] + [int(v) for v in g.integers(0, 256, max(args.bytes - 2, 0))]
    ks = [0x00, 0x00][:args.bytes] + [int(v) for v in g.integers(0, 256, max(args.bytes - 2, 0))]
    B = len(xs)
    msgs = np.array([n for x, k in zip(xs, ks) for n in (x >> 4, x & 15, k >> 4, k & 15)], np.uint32)
    inputs = sk.encrypt_lwe_message(msgs, M, seed0=60_000)
    circuit = build_circuit(B)
    levels, depth = circuit.schedule()
    print(f"{B} bytes: {len(circuit.nodes)} nodes ({4 * B} of them select nodes), bootstrap depth {depth}\n")

    t0 = time.perf_counter()
    out, depth_run = circuit.run(ctx, tables, inputs, packing_key=key)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"Evaluated in {ms:.1f} ms ({ctx.last_kernels()})\n")

    dec = sk.decrypt_lwe_message(out, M)
    got = [int(dec[2 * b]) << 4 | int(dec[2 * b + 1]) for b in range(B)]
    for x, k, s in zip(xs, ks, got):
        print(f"  S[0x{x:02X} ^ 0x{k:02X}] = 0x{s:02X}  (expected 0x{sbox[x ^ k]:02X})")
    ok = got == [sbox[x ^ k] for x, k in zip(xs, ks)] and depth == 4 and depth_run == 4
    tables.close()
    key.close()
    ctx.close()
    print("\n✓ Success! Encrypted S-box outputs computed correctly." if ok else "\n✗ Error! Result mismatch.")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
