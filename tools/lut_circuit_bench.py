#!/usr/bin/env python3
"""LUT circuits on one MI355X: one JSON line.

At UINT4 (message modulus 16) with --nodes nodes (4,096), device-resident:

  mixed    tfhe_gpu_lut_apply_dev, one term (i, 1) per node, 4 tables interleaved (lut[i] = i mod 4),
           against tfhe_gpu_bootstrap_lut_batch_dev over the same ciphertexts with ONE table: the
           same blind-rotation kernel plus one scalar read per item, the linear-combination kernel
           and the descriptor upload.  Alternating call by call after the outputs were compared
           (the items of table 0 must carry the single-table call's words).
  combine  the share of a lut_apply_dev call that is not its blind rotation or key switch (the
           library's own events around those two, tfhe_gpu_profile_*): k_lut_combine plus the
           descriptor upload; and the same with 3 terms per node.
  adders   16 and 256 radix additions (8 nodes in 4 levels each) in one tfhe_gpu_lut_circuit_eval_dev.

Times are device events on torch's stream around each call, medians of at least --seconds of
warmed work per variant.

    python tools/lut_circuit_bench.py [--out profiles/lut_circuit_bench.json]
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
    ap.add_argument("--nodes", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=0.5, help="timed device work per variant, at least")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lut_circuit_bench.py: no GPU (a rate is measured on the MI355X or not at all)")
    B = args.nodes
    ctx = tfhe_amd.Context("uint4", 0)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    p, n1 = ctx.params, ctx.n1
    g = np.random.default_rng(7)
    msgs = g.integers(0, 4, B).astype(np.uint32)
    pool = sk.encrypt_lwe_message(msgs, M, seed0=9000)
    f = [lambda x, j=j: ((j + 1) * x + j) % M for j in range(4)]
    tvs = np.array([tfhe_amd.lut_generate(p, M, fj) for fj in f])
    tables = tfhe_amd.LutSet(ctx, tvs)
    t_pool, t_tv0 = dev_i32(pool), dev_i32(tvs[0])
    t_out = torch.zeros((B, n1), dtype=torch.int32, device="cuda:0")
    t_one = torch.zeros((B, n1), dtype=torch.int32, device="cuda:0")
    ar = np.arange(B, dtype=np.uint32)
    mixed = tfhe_amd.LutNodes(np.arange(B + 1), ar, np.ones(B, np.int32), np.zeros(B), ar % 4)
    three = tfhe_amd.LutNodes(3 * np.arange(B + 1), np.stack([ar, (ar + 1) % B, (ar + 2) % B], 1).reshape(-1),
                              np.tile(np.array([1, 2, -1], np.int32), B), np.zeros(B), ar % 4)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    apply_mixed = lambda: ctx.lut_apply_dev(tables, t_pool.data_ptr(), B, mixed, t_out.data_ptr())  # noqa: E731
    apply_three = lambda: ctx.lut_apply_dev(tables, t_pool.data_ptr(), B, three, t_out.data_ptr())  # noqa: E731
    single = lambda: ctx.bootstrap_lut_batch_dev(t_pool.data_ptr(), t_tv0.data_ptr(), t_one.data_ptr(), B)  # noqa: E731

    # the same words where the tables agree, and correct messages under every table
    apply_mixed()
    kernels = ctx.last_kernels()
    single()
    ctx.sync()
    got, one = t_out.cpu().numpy().view(np.uint32), t_one.cpu().numpy().view(np.uint32)
    same = bool(np.array_equal(got[0::4], one[0::4])) and not np.array_equal(got[1::4], one[1::4])
    dec = sk.decrypt_lwe_message(got[:64], M)
    correct = all(int(dec[i]) == f[i % 4](int(msgs[i])) for i in range(64))
    if not (same and correct):
        raise SystemExit(f"lut_circuit_bench.py: table-0 items identical={same} decrypt={correct}; nothing timed")

    ms = alternate({"lut_apply_dev_4_tables": apply_mixed, "bootstrap_lut_batch_dev_1_table": single}, args.seconds,
                   args.warmup)
    mixed_line = {k: stats(v) for k, v in ms.items()}
    ratio = mixed_line["lut_apply_dev_4_tables"]["ms_median"] / mixed_line["bootstrap_lut_batch_dev_1_table"]["ms_median"]

    def share(fn, reps=5):
        """(call ms, blind-rotation ms, key-switch ms) medians: the library's events inside the call."""
        rows = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.profile_begin()
            a.record()
            fn()
            b.record()
            br, ks, _ = ctx.profile_end()
            b.synchronize()
            rows.append((a.elapsed_time(b), br, ks))
        call, br, ks = (float(np.median([r[i] for r in rows])) for i in range(3))
        rest = call - br - ks
        return {"call_ms": round(call, 4), "blind_rotate_ms": round(br, 4), "key_switch_ms": round(ks, 4),
                "combine_and_upload_ms": round(rest, 4), "combine_and_upload_share": round(rest / call, 4)}

    combine = {"terms_1": share(apply_mixed), "terms_3": share(apply_three)}

    # radix adders: A additions side by side, 8 nodes in 4 levels each
    msg_carry = tfhe_amd.LutSet(ctx, [tfhe_amd.lut_generate(p, M, lambda x: x % 4),
                                      tfhe_amd.lut_generate(p, M, lambda x: x // 4)])
    adders = {}
    for A in (16, 256):
        circ = tfhe_amd.LutCircuit()
        ins = [[circ.input() for _ in range(8)] for _ in range(A)]
        for w in ins:
            circ.output(*circ.radix_add(w[:4], w[4:], 0, 1))
        vals = g.integers(0, 256, (A, 2))
        digs = np.array([[(int(v) >> (2 * i)) & 3 for v in pr for i in range(4)] for pr in vals], np.uint32).reshape(-1)
        t_in = dev_i32(sk.encrypt_lwe_message(digs, M, seed0=20_000))
        t_sum = torch.zeros((5 * A, n1), dtype=torch.int32, device="cuda:0")
        nodes, outs = circ.packed(), np.array(circ.outputs, np.uint32)
        run = lambda: ctx.lut_circuit_eval_dev(msg_carry, t_in.data_ptr(), circ.n_inputs, nodes, outs, t_sum.data_ptr())  # noqa: E731
        run()
        ctx.sync()
        d = sk.decrypt_lwe_message(t_sum.cpu().numpy().view(np.uint32), M).reshape(A, 5)
        sums = [sum(int(x) << (2 * i) for i, x in enumerate(r)) for r in d]
        right = sum(int(s == int(a) + int(b)) for s, (a, b) in zip(sums, vals))
        t = alternate({"run": run}, args.seconds / 2, args.warmup)["run"]
        adders[str(A)] = dict(stats(t), nodes=8 * A, levels=4, correct=f"{right}/{A}", kernels=ctx.last_kernels(),
                              additions_per_s=round(A / float(np.median(t)) * 1e3, 1))
    ctx.sync()
    ctx.set_stream(None)
    line = {"metric": f"LUT nodes/sec (UINT4, m = {M}, {B} nodes, 4 tables interleaved, device-resident) on one MI355X",
            "value": round(B / mixed_line["lut_apply_dev_4_tables"]["ms_median"] * 1e3, 1), "unit": "nodes/s",
            "nodes": B, "kernels": kernels, "mixed_tables": mixed_line, "mixed_over_single_table": round(ratio, 4),
            "table0_items_identical": same, "decrypt_check": correct, "combine": combine, "radix_adders": adders,
            "timing": f"device events around each call, alternating variants, >= {args.seconds} s per variant after "
                      f"{args.warmup} warm-up calls; medians", "build_id": tfhe_amd.build_id()}
    msg_carry.close()
    tables.close()
    ctx.close()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
