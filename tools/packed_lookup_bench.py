#!/usr/bin/env python3
"""Packed table lookup against the CMUX tree on one MI355X: one JSON line.

Q queries of the 256 x 8-bit table (an S-box) by 8 TRGSW-encrypted address bits
each, device-resident, set 128.  Every query has its own 8 selectors in HBM (Q * 8
distinct TRGSWs; the host draws 64 encryptions and replicates them, which changes
no traffic).

  tree    tfhe_gpu_table_lookup_dev on the 256-TRLWE table (tfhe_lookup_table_pack_bits):
          255 CMUXes per query, one launch per level
  packed  tfhe_gpu_packed_lookup_dev on the 2-TRLWE table (tfhe_lookup_table_pack_slots):
          1 tree CMUX + 7 rotate-CMUXes per query, two launches

Both forms' outputs are decrypted first and must give the same table entries in
coefficients 0..7 (the ciphertexts differ: other CMUXes, other noise).  Then the
two alternate call by call, each call between device events, until each has at
least --seconds of timed work and at least --calls calls, after --warmup calls of
each.  The chain kernel alone (tfhe_gpu_rotate_by_bits_dev, h = 7, Q items) is
timed in the same loop for its CMUX rate.  The ratio is recorded, not targeted.

    python tools/packed_lookup_bench.py [--out profiles/packed_lookup_bench.json]
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
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=0.5, help="timed device work per form, at least")
    ap.add_argument("--calls", type=int, default=24, help="timed calls per form, at least")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("packed_lookup_bench.py: no GPU (a rate is measured on the MI355X or not at all)")
    Q, k, width, pname = args.queries, 8, 8, "128"
    p = tfhe_amd.make_params(pname)
    N2 = 2 * p.N
    ctx = tfhe_amd.Context(pname, 0)
    sk = tfhe_amd.secret_key_new(p, 42)
    g = np.random.default_rng(7)
    # 32 encryptions of 0 and 32 of 1; address bit (q, j) gets the copy (q * k + j) % 32 of its value
    pool = ctx.trgsw_encrypt(sk.key_lv1, np.repeat([0, 1], 32), seed0=9000)
    values = g.permutation(1 << k).astype(np.uint64)
    queries = g.integers(0, 1 << k, Q)
    bits = (queries[:, None] >> np.arange(k)[None, :]) & 1
    pick = (bits * 32 + (np.arange(Q * k).reshape(Q, k) % 32)).reshape(-1)
    sels = tfhe_amd.TrgswSet(ctx, pool[pick])
    addr = np.arange(Q * k, dtype=np.uint32).reshape(Q, k)
    plan = tfhe_amd.packed_lookup_plan(p, k, width)
    t_tree = dev_i32(tfhe_amd.lookup_table_pack_bits(p, values, width))
    t_packed = dev_i32(tfhe_amd.lookup_table_pack_slots(p, values, width))
    t_out = {f: torch.zeros((Q, N2), dtype=torch.int32, device="cuda:0") for f in ("tree", "packed", "chain")}
    t_in = torch.randint(-2 ** 31, 2 ** 31 - 1, (Q, N2), dtype=torch.int32, device="cuda:0")
    rot = np.array(plan.rot[:plan.h], np.uint32)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    run = {
        "tree": lambda: ctx.table_lookup_dev(sels, addr, t_tree.data_ptr(), t_out["tree"].data_ptr()),
        "packed": lambda: ctx.packed_lookup_dev(sels, addr, width, t_packed.data_ptr(), t_out["packed"].data_ptr()),
        "chain": lambda: ctx.rotate_by_bits_dev(sels, addr[:, :plan.h], rot, t_in.data_ptr(), t_out["chain"].data_ptr()),
    }
    cmux = {"tree": (1 << k) - 1, "packed": plan.cmuxes, "chain": plan.h}

    # the same table entries from both forms first
    got, names = {}, {}
    for f in ("tree", "packed"):
        run[f]()
        ctx.sync()
        names[f] = ctx.last_kernels()
        dec = ctx.trlwe_decrypt_bool(sk.key_lv1, t_out[f].cpu().numpy().view(np.uint32))
        got[f] = np.array([tfhe_amd.bit_utils.convert(dec[q][:width]) for q in range(Q)])
    run["chain"]()
    ctx.sync()
    names["chain"] = ctx.last_kernels()
    want = values[queries].astype(np.int64)
    equal = bool(np.array_equal(got["tree"], got["packed"]))
    correct = bool(np.array_equal(got["packed"], want))
    if not (equal and correct):
        raise SystemExit(f"packed_lookup_bench.py: decrypted outputs equal={equal} correct={correct}; nothing timed")
    for f in run:
        for _ in range(args.warmup):
            run[f]()
    ctx.sync()
    ms = {f: [] for f in run}
    while min(sum(ms[f]) for f in ("tree", "packed")) < args.seconds * 1e3 or len(ms["tree"]) < args.calls:
        for f in run:  # alternating, one call each
            ms[f].append(timed(run[f]))
    ctx.sync()
    ctx.set_stream(None)
    forms = {}
    for f in run:
        med = float(np.median(ms[f]))
        forms[f] = {"kernels": names[f], "calls": len(ms[f]), "cmux_per_item": cmux[f], "ms_median": round(med, 4),
                    "ms_min": round(min(ms[f]), 4), "ms_max": round(max(ms[f]), 4),
                    "lookups_per_s" if f != "chain" else "items_per_s": round(Q / med * 1e3, 1),
                    "cmux_per_s": round(Q * cmux[f] / med * 1e3, 1)}
    line = {"metric": "packed encrypted table lookups/sec (256 x 8-bit table, 8 TRGSW address bits, set 128) on one MI355X",
            "value": forms["packed"]["lookups_per_s"], "unit": "lookups/s", "queries": Q, "k": k, "width": width,
            "params": pname, "plan": {"stride": plan.stride, "slots": plan.slots, "h": plan.h, "v": plan.v,
                                      "trlwes": plan.trlwes, "cmuxes": plan.cmuxes},
            "forms": forms, "packed_over_tree": round(forms["tree"]["ms_median"] / forms["packed"]["ms_median"], 2),
            "chain_kernel_cmux_per_s": forms["chain"]["cmux_per_s"],
            "decrypted_outputs_equal": equal, "decrypt_check": correct,
            "timing": f"device events around each call, the three alternating, >= {args.seconds} s and >= {args.calls} "
                      f"calls per form after {args.warmup} warm-up calls; medians", "build_id": tfhe_amd.build_id()}
    sels.close()
    ctx.close()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
