#!/usr/bin/env python3
"""The multi-output LUT bootstrap against two single-output nodes, on one MI355X: one JSON line.

--additions (256 and 1,024) radix additions of 8-bit numbers at UINT4, four base-4 digits each, side by
side in one device-resident circuit call, in two forms:

  two_table  message modulus 16, per digit a message node and a carry node over the same terms:
             8 nodes = 8 blind rotations per addition (LutCircuit.radix_add, tfhe_gpu_lut_circuit_eval_dev)
  fused      message modulus 8, theta = 1, per digit ONE node with the interleaved (message, carry) table:
             4 nodes = 4 blind rotations per addition, the two outputs extracted from one accumulator
             (LutCircuit.radix_add_fused, tfhe_gpu_lut_circuit_eval_multi_dev)

Both forms add the same numbers; their decrypted sums are compared with a + b and with each other before
anything is timed.  Times are device events on torch's stream around each call, the two forms alternating
call by call, medians of at least --seconds of warmed work per form.  per_level splits a call by the
library's own events (tfhe_gpu_profile_*): the blind rotation, and what follows it in the level (two_table:
the key switch; fused: the fan-out extraction and the key switch), as means over the 4 levels.

    python tools/lut_multi_bench.py [--out profiles/lut_multi_bench.json]
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

DIGITS = 4


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


def alternate(fns, seconds, warmup):
    """Every fn warmed, then one call each in turn until each has `seconds` of device time."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    while min(sum(v) for v in ms.values()) < seconds * 1e3:
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--additions", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--seconds", type=float, default=0.5, help="timed device work per form, at least")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lut_multi_bench.py: no GPU (a rate is measured on the MI355X or not at all)")
    ctx = tfhe_amd.Context("uint4", 0)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    p, n1 = ctx.params, ctx.n1
    g = np.random.default_rng(11)
    gen = lambda m, f: tfhe_amd.lut_generate(p, m, f)  # noqa: E731
    sets = {"two_table": tfhe_amd.LutSet(ctx, [gen(16, lambda x: x % 4), gen(16, lambda x: x // 4)]),
            "fused": tfhe_amd.LutSet(ctx, [tfhe_amd.lut_interleave(p, [gen(8, lambda x: x % 4), gen(8, lambda x: x // 4)])])}
    modulus = {"two_table": 16, "fused": 8}
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    def share(fn, reps=5):
        """Medians of (call, blind rotations, what follows them) in ms, from the library's events inside the call."""
        rows = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.profile_begin()
            a.record()
            fn()
            b.record()
            br, rest, launches = ctx.profile_end()
            b.synchronize()
            rows.append((a.elapsed_time(b), br, rest, launches))
        call, br, rest, launches = (float(np.median([r[i] for r in rows])) for i in range(4))
        return {"call_ms": round(call, 4), "launches": int(launches), "blind_rotate_ms_per_level": round(br / DIGITS, 4),
                "after_blind_rotate_ms_per_level": round(rest / DIGITS, 4),
                "combine_and_upload_ms_per_level": round((call - br - rest) / DIGITS, 4)}

    results = {}
    for A in args.additions:
        vals = g.integers(0, 256, (A, 2))
        digs = np.array([[(int(v) >> (2 * i)) & 3 for v in pr for i in range(DIGITS)] for pr in vals], np.uint32).reshape(-1)
        runs, sums, info = {}, {}, {}
        for form in ("two_table", "fused"):
            circ = tfhe_amd.LutCircuit()
            ins = [[circ.input() for _ in range(2 * DIGITS)] for _ in range(A)]
            for w in ins:
                circ.output(*(circ.radix_add(w[:DIGITS], w[DIGITS:], 0, 1) if form == "two_table"
                              else circ.radix_add_fused(w[:DIGITS], w[DIGITS:], 0)))
            t_in = dev_i32(sk.encrypt_lwe_message(digs, modulus[form], seed0=20_000))
            t_sum = torch.zeros(((DIGITS + 1) * A, n1), dtype=torch.int32, device="cuda:0")
            # the tensors and the circuit live as long as the closure
            runs[form] = lambda c=circ, s=sets[form], i=t_in, o=t_sum: c.run_dev(ctx, s, i.data_ptr(), o.data_ptr())
            depth = runs[form]()
            kernels = ctx.last_kernels()
            ctx.sync()
            d = sk.decrypt_lwe_message(t_sum.cpu().numpy().view(np.uint32), modulus[form]).reshape(A, DIGITS + 1)
            sums[form] = [sum(int(x) << (2 * i) for i, x in enumerate(r)) for r in d]
            info[form] = {"nodes": len(circ.nodes), "blind_rotations": len(circ.nodes), "outputs_per_level": 2 * A,
                          "levels": depth,
                          "message_modulus": modulus[form], "kernels": kernels}
        want = [int(a) + int(b) for a, b in vals]
        if sums["two_table"] != want or sums["fused"] != want:
            wrong = {k: sum(int(s != w) for s, w in zip(v, want)) for k, v in sums.items()}
            raise SystemExit(f"lut_multi_bench.py: {A} additions, wrong sums {wrong}; nothing timed")
        ms = alternate(runs, args.seconds, args.warmup)
        row = {}
        for form in runs:
            med = float(np.median(ms[form]))
            row[form] = dict(stats(ms[form]), **info[form], additions_per_s=round(A / med * 1e3, 1),
                             per_level=share(runs[form]))
        row["sums_equal_and_correct"] = True
        row["fused_speedup"] = round(row["two_table"]["ms_median"] / row["fused"]["ms_median"], 4)
        results[str(A)] = row
    ctx.sync()
    ctx.set_stream(None)
    last = results[str(args.additions[-1])]
    line = {"metric": f"fused over two-table radix additions (UINT4, {args.additions[-1]} 8-bit additions, "
                      "device-resident) on one MI355X",
            "value": last["fused_speedup"], "unit": "x", "additions": results,
            "timing": f"device events around each call, the two forms alternating, >= {args.seconds} s per form after "
                      f"{args.warmup} warm-up calls; medians", "build_id": tfhe_amd.build_id()}
    for s in sets.values():
        s.close()
    ctx.close()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
