"""An encrypted S-box lookup on the MI355X through the packed lookup: the 256-entry byte table
of encrypted_sbox.py (a fixed permutation of 0..255 from a seed) sits in 2 TRLWEs, 128 entries
side by side in each ("horizontal packing"), and is addressed by 8 TRGSW-encrypted bits per
query: one CMUX under the top bit picks the TRLWE, then 7 rotate-CMUXes under the low bits turn
the addressed entry to coefficients 0..7 (trgsw.cmux on polyMulWithXK, trgsw.zig:260-284, :442-466).

  client  encrypts each address bit as a TRGSW (TRGSWLv1.encryptTorus, trgsw.zig:35-71)
  server  8 CMUXes per query, where the CMUX tree of encrypted_sbox.py takes 255, pick the table
          entry (tfhe_gpu_packed_lookup_batch), then the 8
          output bits are extracted and key-switched (sampleExtractIndex + identityKeySwitching):
          ordinary TLWELv0 ciphertexts, which feed Gates like any other; one of them is ANDed
          with a fresh ciphertext
  client  decrypts

The same lookup with gates alone takes hundreds of bootstraps of 700 CMUX steps each.

    python examples/encrypted_sbox_packed.py [--queries 4] [--seed 2024] [--device 0]
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

    print("=== TFHE Encrypted S-box Lookup Example, packed table (MI355X) ===\n")
    t0 = time.perf_counter()
    ctx = tfhe_amd.Context("128", args.device)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    p = ctx.params
    print(f"Keys generated in {time.perf_counter() - t0:.2f} s\n")

    g = np.random.default_rng(args.seed)
    sbox = g.permutation(256).astype(np.uint64)
    table = tfhe_amd.lookup_table_pack_slots(p, sbox, 8)  # public table: trivial TRLWEs, 128 entries in each
    plan = tfhe_amd.packed_lookup_plan(p, 8, 8)
    print(f"Table: {plan.trlwes} TRLWEs of {plan.slots} entries, {plan.v} tree level + {plan.h} rotation steps "
          f"= {plan.cmuxes} CMUXes per query\n")
    Q, k = args.queries, 8
    xs = g.integers(0, 256, Q)
    print(f"Plaintext inputs:  {[int(x) for x in xs]}\nExpected outputs:  {[int(sbox[x]) for x in xs]}\n")

    # client: one TRGSW per address bit, least significant first
    bits = ((xs[:, None] >> np.arange(k)[None, :]) & 1).astype(np.uint32)
    selectors = tfhe_amd.TrgswSet(ctx, ctx.trgsw_encrypt(sk.key_lv1, bits.reshape(-1), seed0=10_000))
    addr = np.arange(Q * k, dtype=np.uint32).reshape(Q, k)

    # server
    t0 = time.perf_counter()
    out = ctx.packed_lookup(selectors, addr, 8, table)              # (Q, 2N) TRLWELv1
    lv0 = ctx.sample_extract(out, np.arange(8), key_switch=True)    # (Q, 8, n + 1) TLWELv0
    ms = (time.perf_counter() - t0) * 1e3
    print(f"{Q} lookups ({Q * plan.cmuxes} CMUXes, {ctx.last_kernels()}) + {Q * 8} extractions with key switch in {ms:.1f} ms")
    fresh = sk.encrypt_bool([1] * Q, seed0=20_000)
    anded = tfhe_amd.Gates(ctx).and_gate(lv0[:, 0], fresh)          # output bit 0 AND an encrypted 1

    # client
    got = [bit_utils.convert(sk.decrypt_bool(lv0[q])) for q in range(Q)]
    and_bits = sk.decrypt_bool(anded)
    print(f"Decrypted outputs: {got}")
    print(f"Bit 0 AND 1 (through a gate bootstrap): {[int(b) for b in and_bits]}")
    ok = got == [int(sbox[x]) for x in xs] and all(bool(b) == bool(int(sbox[x]) & 1) for b, x in zip(and_bits, xs))
    selectors.close()
    ctx.close()
    print("\n✓ Success! Encrypted lookups computed correctly." if ok else "\n✗ Error! Result mismatch.")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
