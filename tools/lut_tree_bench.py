#!/usr/bin/env python3
"""The bivariate LUT bootstrap (tfhe_gpu_lut_apply2_dev) against its floor and its parts, on one MI355X: one JSON line.

--pairs (1,024) products of two 4-bit digits at UINT4, m = 16, f = x * y mod 16, device-resident, in three forms:

  fused        Context.lut_apply2_dev: level 1 (m bootstraps of y per node), pack, spread, level 2, one call
  floor        the same (m + 1) * B bootstraps as ONE plain Context.lut_apply_dev call: no pack, no spread, one
               launch where the tree needs two; what the blind rotations and key switches alone cost
  composed     the separate _dev entries: lut_apply_dev (level 1), pack_tlwe_dev, lut_spread_dev,
               bootstrap_lut_each_dev (level 2)

The fused and the composed outputs are compared word for word and decrypted to x * y mod 16 before anything is
timed.  Times are device events on torch's stream around each call, the forms alternating call by call, medians of at
least --seconds of warmed work per form.  `steps` times the composed form's four entries one by one, alternating
for --step-rounds rounds: the shares of level 1, pack, spread and level 2.

    python tools/lut_tree_bench.py [--out profiles/lut_tree_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zig-tfhe_amd"))

import torch  # noqa: E402  (before the library: one HIP runtime per process)

import tfhe_amd  # noqa: E402

M = 16


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


def stats(ms):
    return {"calls": len(ms), "ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4)}


def alternate(fns, seconds, warmup, rounds=0):
    """Every fn warmed, then one call each in turn: `rounds` times, or (rounds = 0) until each has `seconds`
    of device time.  The steps differ by four orders of magnitude, so they take a fixed number of rounds."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    while (len(next(iter(ms.values()))) < rounds) if rounds else (min(sum(v) for v in ms.values()) < seconds * 1e3):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    return ms


def one_term_nodes(src, lut):
    """LutNodes of one term each: pool[src[i]] with coefficient 1, table lut[i]."""
    n = len(src)
    return tfhe_amd.LutNodes(np.arange(n + 1), src, np.ones(n), np.zeros(n), lut)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed device work per form, at least")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-rounds", type=int, default=12, help="timed rounds of the four separate steps")
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lut_tree_bench.py: no GPU (a rate is measured on the MI355X or not at all)")
    B, N = args.pairs, 1024
    w, rot = N // M, 2 * N - N // (2 * M)
    ctx = tfhe_amd.Context("uint4", 0)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    key = tfhe_amd.PackingKey.generate(ctx, sk, seed0=50_000)
    p, n1 = ctx.params, ctx.n1
    ls = tfhe_amd.LutSet(ctx, tfhe_amd.lut_generate2(p, M, lambda x, y: (x * y) % M))
    g = np.random.default_rng(12)
    xv, yv = g.integers(0, M, B).astype(np.uint32), g.integers(0, M, B).astype(np.uint32)
    # pool: the B x inputs, then the B y inputs
    t_pool = dev_i32(np.concatenate([sk.encrypt_lwe_message(xv, M, seed0=70_000),
                                     sk.encrypt_lwe_message(yv, M, seed0=70_000 + B)]))
    at = np.arange(B, dtype=np.uint32)
    nodes2 = (np.zeros(B, np.uint32), at, at + B)
    level1 = one_term_nodes(np.repeat(at + B, M), np.tile(np.arange(M, dtype=np.uint32), B))
    floor = one_term_nodes(np.concatenate([np.repeat(at + B, M), at]),
                           np.concatenate([np.tile(np.arange(M, dtype=np.uint32), B), np.zeros(B, np.uint32)]))
    coef = np.arange(M, dtype=np.uint32) * w
    t_fused = torch.zeros((B, n1), dtype=torch.int32, device="cuda:0")
    t_comp = torch.zeros((B, n1), dtype=torch.int32, device="cuda:0")
    t_floor = torch.zeros(((M + 1) * B, n1), dtype=torch.int32, device="cuda:0")
    t_g = torch.zeros((B * M, n1), dtype=torch.int32, device="cuda:0")
    t_tv = torch.zeros((B, 2 * N), dtype=torch.int32, device="cuda:0")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    steps = {
        "level1": lambda: ctx.lut_apply_dev(ls, t_pool.data_ptr(), 2 * B, level1, t_g.data_ptr()),
        "pack": lambda: ctx.pack_tlwe_dev(key, t_g.data_ptr(), B, coef, t_tv.data_ptr()),
        "spread": lambda: ctx.lut_spread_dev(t_tv.data_ptr(), w, rot, t_tv.data_ptr(), B),
        "level2": lambda: ctx.bootstrap_lut_each_dev(t_pool.data_ptr(), t_tv.data_ptr(), t_comp.data_ptr(), B),
    }

    def composed():
        for fn in steps.values():
            fn()

    forms = {
        "fused": lambda: ctx.lut_apply2_dev(ls, key, M, t_pool.data_ptr(), 2 * B, nodes2, t_fused.data_ptr()),
        "floor": lambda: ctx.lut_apply_dev(ls, t_pool.data_ptr(), 2 * B, floor, t_floor.data_ptr()),
        "composed": composed,
    }
    kernels = {}
    for name, fn in forms.items():
        fn()
        kernels[name] = ctx.last_kernels()
    ctx.sync()
    fused, comp = (t.cpu().numpy().view(np.uint32) for t in (t_fused, t_comp))
    dec = sk.decrypt_lwe_message(fused, M)
    wrong = int((dec != (xv * yv) % M).sum())
    if wrong or not np.array_equal(fused, comp):
        raise SystemExit(f"lut_tree_bench.py: {wrong} of {B} products wrong, fused == composed: "
                         f"{np.array_equal(fused, comp)}; nothing timed")
    print("outputs equal and correct; timing the forms", file=sys.stderr, flush=True)
    ms = alternate(forms, args.seconds, args.warmup)
    print("forms timed; timing the steps", file=sys.stderr, flush=True)
    step_ms = alternate(steps, 0, args.warmup, rounds=args.step_rounds)
    ctx.sync()
    ctx.set_stream(None)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    smed = {k: float(np.median(v)) for k, v in step_ms.items()}
    line = {"metric": f"bivariate LUT bootstrap over its floor (UINT4, {B} pairs, m = {M}, device-resident) on one MI355X",
            "value": round(med["fused"] / med["floor"], 4), "unit": "x",
            "pairs": B, "m": M, "bootstraps_per_call": (M + 1) * B,
            "forms": {k: dict(stats(v), kernels=kernels[k]) for k, v in ms.items()},
            "fused_over_floor": round(med["fused"] / med["floor"], 4),
            "fused_over_composed": round(med["fused"] / med["composed"], 4),
            "steps": {k: stats(v) for k, v in step_ms.items()},
            "step_share_of_composed": {k: round(v / sum(smed.values()), 5) for k, v in smed.items()},
            "outputs_equal_and_correct": True,
            "timing": f"device events around each call, the forms alternating, >= {args.seconds} s per form after "
                      f"{args.warmup} warm-up calls, the steps {args.step_rounds} rounds; medians", "build_id": tfhe_amd.build_id()}
    ls.close()
    key.close()
    ctx.close()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
