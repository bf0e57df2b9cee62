#!/usr/bin/env python3
"""Packed scatter-add (encrypted table writes) on one MI355X: one JSON line.

Q writes into a packed table of 2^k 8-bit entries by k TRGSW-encrypted address bits
each, device-resident, set 128, at two shapes:

  k = 8   2 TRLWEs:  7 rotate-CMUXes + 1 demux external product per write
  k = 12  32 TRLWEs: 7 rotate-CMUXes + 31 demux external products per write

Every write has its own k selectors in HBM (Q * k TRGSWs; the host draws 64
encryptions and replicates them, which changes no traffic).  Per shape:

  scatter   tfhe_gpu_packed_scatter_add_dev: one chain launch, one launch per demux
            level, one reduce per chunk
  per_wave  the same under TFHE_OPT_CMUX_FORM = 1 (k_demux on every level)
  composed  the same writes from the entry points that were there before it:
            tfhe_gpu_rotate_by_bits_dev, per level tfhe_gpu_cmux_batch_dev with an
            all-zero in0 (which gives hi) and a torch subtraction for lo, and a torch
            sum into the table.  It reads and writes strictly more and launches more.
  lookup    tfhe_gpu_packed_lookup_dev of the same shape and addresses

scatter, per_wave and composed must leave the same table words (torch.equal) from
the same start before anything is timed.  Then the four alternate call by call,
each call between device events, until each has at least --seconds of timed work
and at least --calls calls, after --warmup calls of each.  Ratios are recorded,
not targeted.

    python tools/packed_write_bench.py [--out profiles/packed_write_bench.json]
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


def timed(fn):
    """Device milliseconds of fn() on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rand_i32(*shape):
    return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device="cuda:0")


def shape_record(ctx, pool, p, Q, k, width, args):
    N2 = 2 * p.N
    plan = tfhe_amd.packed_lookup_plan(p, k, width)
    h, v = plan.h, plan.v
    g = np.random.default_rng(100 + k)
    queries = g.integers(0, 1 << k, Q)
    bits = (queries[:, None] >> np.arange(k)[None, :]) & 1
    pick = (bits * 32 + (np.arange(Q * k).reshape(Q, k) % 32)).reshape(-1)
    sels = tfhe_amd.TrgswSet(ctx, pool[pick])
    addr = np.arange(Q * k, dtype=np.uint32).reshape(Q, k)
    rot = np.array([plan.stride << j for j in range(h)], np.uint32)
    start, delta = rand_i32(plan.trlwes, N2), rand_i32(Q, N2)
    tables = {f: start.clone() for f in ("scatter", "per_wave", "composed")}
    rotated = torch.zeros((Q, N2), dtype=torch.int32, device="cuda:0")
    his = [torch.zeros((Q << lv, N2), dtype=torch.int32, device="cuda:0") for lv in range(v)]
    zeros = torch.zeros((Q << max(v - 1, 0), N2), dtype=torch.int32, device="cuda:0")
    level_sel = [np.ascontiguousarray(np.repeat(addr[:, k - 1 - lv], 1 << lv)) for lv in range(v)]
    looked = torch.zeros((Q, N2), dtype=torch.int32, device="cuda:0")

    def scatter(form):
        ctx.packed_scatter_add_dev(sels, addr, width, delta.data_ptr(), tables[form].data_ptr())

    def per_wave():
        with ctx.options(cmux_form=1):
            scatter("per_wave")

    def composed():
        ctx.rotate_by_bits_dev(sels, addr[:, :h], rot, delta.data_ptr(), rotated.data_ptr())
        x = rotated
        for lv in range(v):
            ctx.cmux_dev(sels, level_sel[lv], zeros.data_ptr(), x.data_ptr(), his[lv].data_ptr())
            x = torch.stack((x - his[lv], his[lv]), dim=1).view(Q << (lv + 1), N2)
        tables["composed"] += x.view(Q, 1 << v, N2).sum(dim=0).to(torch.int32)

    run = {"scatter": lambda: scatter("scatter"), "per_wave": per_wave, "composed": composed,
           "lookup": lambda: ctx.packed_lookup_dev(sels, addr, width, tables["scatter"].data_ptr(), looked.data_ptr())}
    names = {}
    for f in run:
        run[f]()
        ctx.sync()
        names[f] = ctx.last_kernels()
    equal = bool(torch.equal(tables["scatter"], tables["composed"]) and torch.equal(tables["scatter"], tables["per_wave"]))
    changed = not bool(torch.equal(tables["scatter"], start))
    if not (equal and changed):
        raise SystemExit(f"packed_write_bench.py: k = {k}: tables equal={equal} changed={changed}; nothing timed")
    for f in run:
        for _ in range(args.warmup):
            run[f]()
    ctx.sync()
    ms = {f: [] for f in run}
    while min(sum(ms[f]) for f in run) < args.seconds * 1e3 or len(ms["scatter"]) < args.calls:
        for f in run:  # alternating, one call each
            ms[f].append(timed(run[f]))
    ctx.sync()
    sels.close()
    forms = {}
    for f in run:
        med = float(np.median(ms[f]))
        forms[f] = {"kernels": names[f], "calls": len(ms[f]), "ms_median": round(med, 4), "ms_min": round(min(ms[f]), 4),
                    "ms_max": round(max(ms[f]), 4), "per_s": round(Q / med * 1e3, 1),
                    "ms_per_call": [round(x, 4) for x in ms[f]]}
    return {"k": k, "width": width, "plan": {"stride": plan.stride, "h": h, "v": v, "trlwes": plan.trlwes},
            "external_products_per_write": h + (1 << v) - 1, "tables_equal": equal, "forms": forms,
            "writes_per_s": forms["scatter"]["per_s"],
            "composed_over_scatter": round(forms["composed"]["ms_median"] / forms["scatter"]["ms_median"], 3),
            "per_wave_over_scatter": round(forms["per_wave"]["ms_median"] / forms["scatter"]["ms_median"], 3),
            "scatter_over_lookup": round(forms["scatter"]["ms_median"] / forms["lookup"]["ms_median"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=0.5, help="timed device work per form, at least")
    ap.add_argument("--calls", type=int, default=16, help="timed calls per form, at least")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("packed_write_bench.py: no GPU (a rate is measured on the MI355X or not at all)")
    Q, width, pname = args.queries, 8, "128"
    p = tfhe_amd.make_params(pname)
    ctx = tfhe_amd.Context(pname, 0)
    sk = tfhe_amd.secret_key_new(p, 42)
    # 32 encryptions of 0 and 32 of 1; address bit (q, j) gets the copy (q * k + j) % 32 of its value
    pool = ctx.trgsw_encrypt(sk.key_lv1, np.repeat([0, 1], 32), seed0=9000)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    shapes = [shape_record(ctx, pool, p, Q, k, width, args) for k in (8, 12)]
    ctx.set_stream(None)
    ctx.close()
    line = {"metric": "packed encrypted table writes/sec (2^k x 8-bit table, k TRGSW address bits, set 128) on one MI355X",
            "value": shapes[0]["writes_per_s"], "unit": "writes/s at k = 8", "queries": Q, "params": pname, "shapes": shapes,
            "timing": f"device events around each call, the four forms alternating, >= {args.seconds} s and >= "
                      f"{args.calls} calls per form after {args.warmup} warm-up calls; medians, and every call's time",
            "build_id": tfhe_amd.build_id()}
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
