"""A table computed under encryption, then looked up by an encrypted address, on the MI355X: the
way from the bootstrapped half of the engine (gates: TLWELv0) into the leveled half (packed
lookup: TRLWELv1) through the packing key switch, and back.

  client  encrypts 16 4-bit values and a 4-bit mask bit by bit (TLWELv0), and each bit of an
          address as a TRGSW (TRGSWLv1.encryptTorus, trgsw.zig:35-71); hands over a packing key
  server  XORs every value with the mask: 64 gate bootstraps (gate_batch)
          packs the 64 gate outputs into one TRLWE, 16 slots of 4 coefficients: the table of
          packed_lookup (pack_table: identityKeySwitching's arithmetic with TRLWE rows)
          picks the addressed entry with 4 rotate-CMUXes per query (packed_lookup), extracts
          its 4 bits and key-switches them back to gate inputs (sample_extract)
  client  decrypts value[addr] ^ mask

Everything between the client's ciphertexts and the result stays on the device's side.

    python examples/encrypted_computed_table.py [--queries 4] [--seed 2024] [--device 0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zig-tfhe_amd"))
import tfhe_amd  # noqa: E402
from tfhe_amd import bit_utils  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=4)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    print("=== TFHE Encrypted Computed-Table Lookup Example (MI355X) ===\n")
    t0 = time.perf_counter()
    ctx = tfhe_amd.Context("128", args.device)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    p = ctx.params
    key = tfhe_amd.PackingKey.generate(ctx, sk, seed0=50_000, basebit=2, t=8)
    print(f"Keys generated in {time.perf_counter() - t0:.2f} s (packing key: {p.n * 8 * 3} TRLWE encryptions)\n")

    g = np.random.default_rng(args.seed)
    k, width, Q = 4, 4, args.queries
    values = g.integers(0, 16, 1 << k)
    mask = int(g.integers(1, 16))
    addrs = g.integers(0, 1 << k, Q)
    want = [int(values[a]) ^ mask for a in addrs]
    print(f"Plaintext values:  {[int(v) for v in values]}\nMask: {mask}  addresses: {[int(a) for a in addrs]}\n"
          f"Expected outputs:  {want}\n")

    # client: the values and the mask bit by bit (entry-major, then bit), the address bits as TRGSWs
    vbits = ((values[:, None] >> np.arange(width)[None, :]) & 1).astype(np.uint8).reshape(-1)
    mbits = np.tile(((mask >> np.arange(width)) & 1).astype(np.uint8), 1 << k)
    ct_v, ct_m = sk.encrypt_bool(vbits, seed0=10_000), sk.encrypt_bool(mbits, seed0=20_000)
    abits = ((addrs[:, None] >> np.arange(k)[None, :]) & 1).astype(np.uint32)
    selectors = tfhe_amd.TrgswSet(ctx, ctx.trgsw_encrypt(sk.key_lv1, abits.reshape(-1), seed0=30_000))
    addr = np.arange(Q * k, dtype=np.uint32).reshape(Q, k)

    # server
    t0 = time.perf_counter()
    gates = ctx.gate_batch(np.full(width << k, tfhe_amd.XOR, np.uint8), ct_v, ct_m)   # 64 TLWELv0
    table = ctx.pack_table(key, gates, k, width)                                      # (1, 2N) TRLWELv1
    packed_by = ctx.last_kernels()
    out = ctx.packed_lookup(selectors, addr, width, table)                            # (Q, 2N) TRLWELv1
    lv0 = ctx.sample_extract(out, np.arange(width), key_switch=True)                  # (Q, 4, n + 1) TLWELv0
    ms = (time.perf_counter() - t0) * 1e3
    print(f"{width << k} gates, 1 pack of {width << k} ciphertexts ({packed_by}), {Q} lookups and {Q * width} "
          f"extractions with key switch in {ms:.1f} ms")

    # client
    got = [bit_utils.convert(sk.decrypt_bool(lv0[q])) for q in range(Q)]
    print(f"Decrypted outputs: {got}")
    ok = got == want
    selectors.close()
    key.close()
    ctx.close()
    print("\n✓ Success! Lookups in the computed table are correct." if ok else "\n✗ Error! Result mismatch.")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
