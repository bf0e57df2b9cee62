#!/usr/bin/env python3
"""Encrypted table lookup on one MI355X: one JSON line.

Q queries of a 2^k-entry table of trivial TRLWELv1 (tfhe_lookup_table_pack_bits)
by k TRGSW-encrypted address bits each, device-resident (tfhe_gpu_table_lookup_dev):
2^k - 1 CMUXes per query, one launch per tree level.  Every query has its own k
selectors in HBM (Q * k distinct TRGSWs; the host draws 64 encryptions and
replicates them, which changes no traffic).

Reported: lookups/s and CMUX/s from device events around at least --seconds of
warmed work, for both CMUX forms (TFHE_OPT_CMUX_FORM 1 per-wave, 2 shared),
alternating call by call after their outputs compared equal; the per-level
split (a cmux_dev batch of each level's size over distinct inputs: levels >= 1
of the tree exactly, level 0 without its shared table); the host-buffer rate
(tfhe_gpu_table_lookup_batch, wall clock); the CPU oracle's CMUX rate on this
host; and, given --bench-json (a bench.py result line of the same machine), the
blind rotation's CMUX-step rate batch * n / blind-rotation ms.  The two ratios
are yardsticks, not thresholds.

    python tools/lookup_bench.py [--bench-json FILE] [--out profiles/lookup_bench.json]
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--params", default="128")
    ap.add_argument("--seconds", type=float, default=0.5, help="timed device work per form, at least")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bench-json", default="", help="a bench.py result line of this machine (blind-rotation yardstick)")
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lookup_bench.py: no GPU (a rate is measured on the MI355X or not at all)")
    Q, k, pname = args.queries, args.k, args.params
    p = tfhe_amd.make_params(pname)
    N2 = 2 * p.N
    ctx = tfhe_amd.Context(pname, 0)
    sk = tfhe_amd.secret_key_new(p, 42)
    g = np.random.default_rng(7)
    # 32 encryptions of 0 and 32 of 1; address bit (q, j) gets the copy (q * k + j) % 32 of its value
    pool = ctx.trgsw_encrypt(sk.key_lv1, np.repeat([0, 1], 32), seed0=9000)
    values = g.permutation(1 << k).astype(np.uint64) & 0xFF
    queries = g.integers(0, 1 << k, Q)
    bits = (queries[:, None] >> np.arange(k)[None, :]) & 1
    pick = (bits * 32 + (np.arange(Q * k).reshape(Q, k) % 32)).reshape(-1)
    sels = tfhe_amd.TrgswSet(ctx, pool[pick])
    addr = np.arange(Q * k, dtype=np.uint32).reshape(Q, k)
    table = tfhe_amd.lookup_table_pack_bits(p, values, 8)
    t_table = dev_i32(table)
    t_out = torch.zeros((Q, N2), dtype=torch.int32, device="cuda:0")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    def lookup(form):
        ctx.set_option("cmux_form", form)
        ctx.table_lookup_dev(sels, addr, t_table.data_ptr(), t_out.data_ptr())

    # identical outputs first, and the right table entries
    outs, names = {}, {}
    for form in (1, 2):
        lookup(form)
        ctx.sync()
        outs[form] = t_out.cpu().numpy().view(np.uint32).copy()
        names[form] = ctx.last_kernels()
    identical = bool(np.array_equal(outs[1], outs[2]))
    dec = ctx.trlwe_decrypt_bool(sk.key_lv1, outs[1][:16])
    correct = all(tfhe_amd.bit_utils.convert(dec[q][:8]) == int(values[queries[q]]) for q in range(16))
    if not (identical and correct):
        raise SystemExit(f"lookup_bench.py: outputs identical={identical} correct={correct}; nothing timed")
    for form in (1, 2):
        for _ in range(args.warmup):
            lookup(form)
    ctx.sync()
    ms = {1: [], 2: []}
    while min(sum(ms[1]), sum(ms[2])) < args.seconds * 1e3:  # alternating, one call each
        for form in (1, 2):
            ms[form].append(timed(lambda: lookup(form)))
    cm = Q * ((1 << k) - 1)
    forms = {}
    for form, label in ((1, "per_wave"), (2, "shared")):
        med = float(np.median(ms[form]))
        forms[label] = {"kernels": names[form], "calls": len(ms[form]), "ms_median": round(med, 4),
                        "ms_min": round(min(ms[form]), 4), "ms_max": round(max(ms[form]), 4),
                        "lookups_per_s": round(Q / med * 1e3, 1), "cmux_per_s": round(cm / med * 1e3, 1)}
    ctx.set_option("cmux_form", 0)
    lookup(0)
    ctx.sync()
    auto_kernels = ctx.last_kernels()
    auto = "shared" if "shared" in auto_kernels else "per_wave"
    # per-level split: a cmux_dev batch of each level's size (per-wave form, distinct inputs)
    big = 1 << (k - 1)
    t_in = torch.randint(-2 ** 31, 2 ** 31 - 1, (Q * big * 2, N2), dtype=torch.int32, device="cuda:0")
    t_lv = torch.zeros((Q * big, N2), dtype=torch.int32, device="cuda:0")
    levels = []
    for j in range(k):
        n = Q * (big >> j)
        sel = np.repeat(addr[:, j], big >> j).astype(np.uint32)
        run = lambda: ctx.cmux_dev(sels, sel, t_in.data_ptr(), t_in.data_ptr() + n * N2 * 4, t_lv.data_ptr())  # noqa: E731
        run()
        ctx.sync()
        t = [timed(run) for _ in range(5)]
        levels.append({"level": j, "cmux": n, "ms_median": round(float(np.median(t)), 4)})
    ctx.sync()
    ctx.set_stream(None)
    # host-buffer rate (table and outputs cross PCIe, indices built on the host): wall clock
    ctx.table_lookup(sels, addr, table)
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        ctx.table_lookup(sels, addr, table)
    host_ms = (time.perf_counter() - t0) / reps * 1e3
    # the CPU oracle's CMUX on this host, one thread
    from oracle import Oracle, params as oparams
    o = Oracle()
    op = oparams(pname)
    off = o.decomposition_offset(op)
    x0, x1 = outs[1][0], outs[1][1]
    o.cmux(op, x0, x1, pool[0], off)
    t0 = time.perf_counter()
    n_or = 0
    while time.perf_counter() - t0 < 0.5:
        o.cmux(op, x0, x1, pool[0], off)
        n_or += 1
    oracle_rate = n_or / (time.perf_counter() - t0)
    best = forms[auto]
    line = {"metric": f"encrypted table lookups/sec ({1 << k}-entry table, {k} TRGSW address bits, set {pname}) on one MI355X",
            "value": best["lookups_per_s"], "unit": "lookups/s", "cmux_per_s": best["cmux_per_s"], "queries": Q, "k": k,
            "params": pname, "cmux_per_lookup": (1 << k) - 1, "auto_form": auto, "auto_kernels": auto_kernels,
            "forms": forms, "outputs_identical": identical, "decrypt_check": correct, "levels_per_wave": levels,
            "host_buffer": {"ms_per_call": round(host_ms, 3), "lookups_per_s": round(Q / host_ms * 1e3, 1)},
            "oracle_cmux_per_s": round(oracle_rate, 1),
            "cmux_rate_over_oracle": round(best["cmux_per_s"] / oracle_rate, 1),
            "timing": f"device events around each call, alternating forms, >= {args.seconds} s per form after "
                      f"{args.warmup} warm-up calls; medians", "build_id": tfhe_amd.build_id()}
    if args.bench_json:
        with open(args.bench_json) as f:
            b = json.loads([ln for ln in f.read().splitlines() if ln.strip().startswith("{")][-1])
        n = tfhe_amd.PARAM_SETS[b["config"]["params"]]["n"]
        br_ms = b.get("roofline", {}).get("kernel_avg_ms") or b["ms_per_step"]
        rate = b["config"]["global_batch"] * n / br_ms * 1e3
        line["blind_rotation"] = {"cmux_steps_per_s": round(rate, 1), "batch": b["config"]["global_batch"], "n": n,
                                  "ms": br_ms, "source": "bench.py line of the same run: " +
                                  ("roofline.kernel_avg_ms" if b.get("roofline", {}).get("kernel_avg_ms") else "ms_per_step")}
        line["cmux_rate_over_blind_rotation"] = round(best["cmux_per_s"] / rate, 3)
    else:
        line["blind_rotation"] = "not measured (no --bench-json)"
    sels.close()
    ctx.close()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
