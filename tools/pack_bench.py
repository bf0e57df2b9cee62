#!/usr/bin/env python3
"""The packing key switch (TLWELv0 -> TRLWELv1 slots) against the identity key switch on one
MI355X: one JSON line.

Set 128, packing key of shape (2, 8) (184 MB resident).  Workloads:

  pack_1x1024     1,024 TLWELv0 into every coefficient of one TRLWE
  pack_16x1024    16 x 1,024 TLWELv0 into 16 TRLWEs
  key_switch_1024 tfhe_gpu_key_switch_batch on 1,024 TLWELv1, the engine's own key switch

The packed ciphertexts are fresh encryptions of random bits; both pack outputs are decrypted
first (TRLWELv1.decryptBool) and must give the bits back at every slot, or nothing is timed.
Then the calls alternate, one of each per round, each between device events, until the
device-resident pack of 1,024 has at least --seconds of timed work and --calls calls, after
--warmup calls of each.  The pack
is timed through the host-buffer entry (like the key switch's only entry, so the two carry
the same kind of copies) and through the device-pointer entry; the key switch is also timed
device-resident as tfhe_gpu_sample_extract_dev with the key switch minus the same call
without it.  The ratios are recorded, not targeted.

    python tools/pack_bench.py [--out profiles/pack_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("oracle", "zig-tfhe_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import torch  # noqa: E402  (before the library: one HIP runtime per process)

import tfhe_amd  # noqa: E402


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def timed(fn):
    """Device milliseconds of fn() on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3, help="timed device work of the device-resident pack of 1,024, at least")
    ap.add_argument("--calls", type=int, default=24, help="timed calls of each workload, at least")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pack_bench.py: no GPU (a rate is measured on the MI355X or not at all)")
    pname, basebit, t = "128", 2, 8
    ctx = tfhe_amd.Context(pname, 0)
    p = ctx.params
    N, n1 = p.N, p.n + 1
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    key = tfhe_amd.PackingKey.generate(ctx, sk, seed0=50_000, basebit=basebit, t=t)
    g = np.random.default_rng(11)
    bits = g.integers(0, 2, 16 * N).astype(np.uint8)
    cts = sk.encrypt_bool(bits, seed0=100_000)           # (16 * 1024, n + 1)
    coef = g.permutation(N).astype(np.uint32)
    lv1 = g.integers(0, 1 << 32, (N, N + 1), dtype=np.uint64).astype(np.uint32)
    trlwe = g.integers(0, 1 << 32, (1, 2 * N), dtype=np.uint64).astype(np.uint32)

    # every slot decrypts first
    out1 = ctx.pack_tlwe(key, cts[:N], coef)
    names = {"pack": ctx.last_kernels()}
    out16 = ctx.pack_tlwe(key, cts, coef)
    dec1 = ctx.trlwe_decrypt_bool(sk.key_lv1, out1)[:, coef].reshape(-1)
    dec16 = ctx.trlwe_decrypt_bool(sk.key_lv1, out16)[:, coef].reshape(-1)
    ok = bool(np.array_equal(dec1, bits[:N].astype(bool)) and np.array_equal(dec16, bits.astype(bool)))
    if not ok:
        raise SystemExit("pack_bench.py: the packed slots do not decrypt to their bits; nothing timed")
    ctx.key_switch(lv1)
    names["key_switch"] = " + ".join(ctx.last_kernels().split(" + ")[-2:])  # cut: the key-switch
    # entry sets the second half of last_kernels() only, so the string still starts with the pack's GEMM

    d_in, d_out = dev_i32(cts.reshape(-1)), torch.zeros((16, 2 * N), dtype=torch.int32, device="cuda:0")
    d_trlwe = dev_i32(trlwe)
    d_lv0 = torch.zeros((N, n1), dtype=torch.int32, device="cuda:0")
    d_lv1 = torch.zeros((N, N + 1), dtype=torch.int32, device="cuda:0")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    run = {
        "pack_1x1024": lambda: ctx.pack_tlwe(key, cts[:N], coef),
        "pack_16x1024": lambda: ctx.pack_tlwe(key, cts, coef),
        "key_switch_1024": lambda: ctx.key_switch(lv1),
        "pack_1x1024_dev": lambda: ctx.pack_tlwe_dev(key, d_in.data_ptr(), 1, coef, d_out.data_ptr()),
        "pack_16x1024_dev": lambda: ctx.pack_tlwe_dev(key, d_in.data_ptr(), 16, coef, d_out.data_ptr()),
        "extract_ks_1024_dev": lambda: ctx.sample_extract_dev(d_trlwe.data_ptr(), 1, coef, d_lv0.data_ptr(), True),
        "extract_1024_dev": lambda: ctx.sample_extract_dev(d_trlwe.data_ptr(), 1, coef, d_lv1.data_ptr(), False),
    }
    items = {f: 16 * N if "16x" in f else N for f in run}
    for f in run:
        for _ in range(args.warmup):
            run[f]()
    ctx.sync()
    ms = {f: [] for f in run}
    while sum(ms["pack_1x1024_dev"]) < args.seconds * 1e3 or len(ms["pack_1x1024_dev"]) < args.calls:
        for f in run:  # alternating, one call each
            ms[f].append(timed(run[f]))
    ctx.sync()
    ctx.set_stream(None)
    work = {}
    for f in run:
        med = float(np.median(ms[f]))
        work[f] = {"items": items[f], "calls": len(ms[f]), "ms_median": round(med, 4), "ms_min": round(min(ms[f]), 4),
                   "ms_max": round(max(ms[f]), 4), "items_per_s": round(items[f] / med * 1e3, 1),
                   "us_per_item": round(med * 1e3 / items[f], 4)}
    ks_dev_ms = work["extract_ks_1024_dev"]["ms_median"] - work["extract_1024_dev"]["ms_median"]
    ks_host = work["key_switch_1024"]["us_per_item"]
    line = {"metric": "TLWELv0 packed into TRLWELv1 slots per second (16 x 1,024, set 128, key (2, 8)) on one MI355X",
            "value": work["pack_16x1024_dev"]["items_per_s"], "unit": "items/s", "params": pname, "basebit": basebit, "t": t,
            "kernels": names, "workloads": work,
            "key_switch_dev_ms": round(ks_dev_ms, 4),
            "pack_over_key_switch_per_item": {
                "host_1x1024": round(work["pack_1x1024"]["us_per_item"] / ks_host, 2),
                "host_16x1024": round(work["pack_16x1024"]["us_per_item"] / ks_host, 2),
                "dev_1x1024": round(work["pack_1x1024_dev"]["ms_median"] / ks_dev_ms, 2),
                "dev_16x1024": round(work["pack_16x1024_dev"]["ms_median"] / 16 / ks_dev_ms, 2)},
            "decrypt_check": ok,
            "timing": f"device events around each call, the {len(run)} alternating, >= {args.seconds} s of pack_1x1024_dev and >= "
                      f"{args.calls} calls after {args.warmup} warm-up calls of each; medians; host_* through the host-buffer "
                      "entries of both, dev_* device-resident with the key switch as extract-with-key-switch minus extract",
            "build_id": tfhe_amd.build_id()}
    key.close()
    ctx.close()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
