"""An encrypted RAM on the MI355X: a 16-entry table of 4-bit words that the server reads and
writes by addresses it cannot see.

  client  encrypts the new words bit by bit (TLWELv0) and each bit of every address as a TRGSW
          (TRGSWLv1.encryptTorus, trgsw.zig:35-71); hands over a packing key
  server  holds the table as one TRLWE, 16 slots of 4 coefficients (lookup_table_pack_slots)
          write: reads the old word (packed_lookup, sample_extract), refreshes it with a
                 bootstrap, packs new - old into a TRLWE (pack_tlwe), and adds it to the slot the
                 address names: 4 rotate-CMUXes per write (packed_scatter_add)
          read:  packed_lookup, then sample_extract back to gate inputs
  client  decrypts what was read

The addresses of one write call must differ from each other (two writes to one entry would both
subtract its old word); across calls they may repeat, as they do here.

    python examples/encrypted_ram.py [--rounds 2] [--seed 2024] [--device 0]
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
    ap.add_argument("--rounds", type=int, default=2, help="write calls of 3 words each")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    print("=== TFHE Encrypted RAM Example (MI355X) ===\n")
    t0 = time.perf_counter()
    ctx = tfhe_amd.Context("128", args.device)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    p = ctx.params
    key = tfhe_amd.PackingKey.generate(ctx, sk, seed0=50_000, basebit=2, t=8)
    print(f"Keys generated in {time.perf_counter() - t0:.2f} s\n")

    g = np.random.default_rng(args.seed)
    k, width = 4, 4
    model = g.integers(0, 16, 1 << k)
    table = tfhe_amd.lookup_table_pack_slots(p, model.astype(np.uint64), width)    # (1, 2N) TRLWELv1
    print(f"Initial memory:    {[int(v) for v in model]}")

    # the 16 addresses' bits as TRGSWs, shared by the writes and the reads: selector 4 a + j is bit j of a
    every = np.arange(1 << k)
    abits = ((every[:, None] >> np.arange(k)[None, :]) & 1).astype(np.uint32)
    selectors = tfhe_amd.TrgswSet(ctx, ctx.trgsw_encrypt(sk.key_lv1, abits.reshape(-1), seed0=30_000))
    addr_of = np.arange(k << k, dtype=np.uint32).reshape(1 << k, k)

    ms = 0.0
    for r in range(args.rounds):
        where = g.choice(1 << k, 3, replace=False)
        what = g.integers(0, 16, 3)
        bits = ((what[:, None] >> np.arange(width)[None, :]) & 1).astype(np.uint8).reshape(-1)
        new = sk.encrypt_bool(bits, seed0=10_000 + 100 * r)                        # client: 12 TLWELv0
        t0 = time.perf_counter()
        table = ctx.packed_write(selectors, key, addr_of[where], width, new, table)  # server
        ms += (time.perf_counter() - t0) * 1e3
        model[where] = what
        print(f"Write {r + 1}: mem[{[int(a) for a in where]}] = {[int(v) for v in what]}  ({ctx.last_kernels()})")

    t0 = time.perf_counter()
    out = ctx.packed_lookup(selectors, addr_of, width, table)                       # server: read all 16
    lv0 = ctx.sample_extract(out, np.arange(width), key_switch=True)
    read_ms = (time.perf_counter() - t0) * 1e3
    got = [bit_utils.convert(sk.decrypt_bool(lv0[a])) for a in every]               # client
    print(f"\nPlaintext model:   {[int(v) for v in model]}\nDecrypted memory:  {got}")
    print(f"{3 * args.rounds} writes in {ms:.1f} ms, 16 reads in {read_ms:.1f} ms")
    ok = got == [int(v) for v in model]
    selectors.close()
    key.close()
    ctx.close()
    print("\n✓ Success! The encrypted memory matches the model." if ok else "\n✗ Error! Memory mismatch.")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
