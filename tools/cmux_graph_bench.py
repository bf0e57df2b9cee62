#!/usr/bin/env python3
"""CMUX graphs on one MI355X: one JSON line.

Q queries of the 32-bit comparator a < b (CmuxGraph.less_than(32): 95 CMUXes in 64 levels of 1 or 2
nodes) at the 128-bit set, device-resident.  The address indices are drawn from one resident set of
4,096 selectors (64 encryptions replicated: per-query selectors would be 6 GB, and the arithmetic
does not care whose bit a selector carries).

Measured with device events, the forms alternating call by call after their outputs compared equal:
  graph     tfhe_gpu_cmux_graph_dev: one k_cmux_rot launch per level over all queries
  composed  the same graph from what existed before it: per level a torch gather of the children
            and tfhe_gpu_cmux_batch_dev, the values of all nodes kept in one tensor
  tree      tfhe_gpu_table_lookup_dev, k = 8, for the scale of its CMUX rate
The first 16 queries are decrypted against the plain comparison of the bits their selectors carry.

    python tools/cmux_graph_bench.py [--out profiles/cmux_graph_bench.json]
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
from tfhe_amd import CmuxGraph  # noqa: E402


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
    ap.add_argument("--bits", type=int, default=32)
    ap.add_argument("--selectors", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=0.5, help="timed device work per form, at least")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cmux_graph_bench.py: no GPU (a rate is measured on the MI355X or not at all)")
    Q, S, pname = args.queries, args.selectors, "128"
    p = tfhe_amd.make_params(pname)
    N2 = 2 * p.N
    ctx = tfhe_amd.Context(pname, 0)
    sk = tfhe_amd.secret_key_new(p, 42)
    g = np.random.default_rng(7)
    pool = ctx.trgsw_encrypt(sk.key_lv1, np.repeat([0, 1], 32), seed0=9000)  # 32 encryptions of 0, 32 of 1
    sel_bit = g.integers(0, 2, S)
    sels = tfhe_amd.TrgswSet(ctx, pool[sel_bit * 32 + np.arange(S) % 32])
    gr = CmuxGraph.less_than(args.bits)
    level, slot, depth, n_slots = gr.plan()
    V, nL, k = gr.n_nodes, gr.n_leaves, gr.k
    addr = g.integers(0, S, (Q, k)).astype(np.uint32)
    leaves = CmuxGraph.bool_leaves(p.N)
    t_leaves = dev_i32(leaves)
    t_out = torch.zeros((Q, 1, N2), dtype=torch.int32, device="cuda:0")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    def graph():
        ctx.cmux_graph_dev(sels, addr, gr, t_leaves.data_ptr(), t_out.data_ptr())

    # composed: all values in one tensor, per level two gathers and one cmux_dev
    vals = torch.zeros((Q, nL + V, N2), dtype=torch.int32, device="cuda:0")
    vals[:, :nL] = t_leaves
    per_level = []
    widest = 0
    for lv in range(1, depth + 1):
        nodes = np.flatnonzero(level == lv)
        widest = max(widest, nodes.size)
        per_level.append((torch.tensor(nL + nodes, device="cuda:0"), torch.tensor(np.array(gr.lo)[nodes], device="cuda:0"),
                          torch.tensor(np.array(gr.hi)[nodes], device="cuda:0"),
                          np.ascontiguousarray(addr[:, np.array(gr.var)[nodes]]).reshape(-1)))
    t_lv = torch.zeros((Q * widest, N2), dtype=torch.int32, device="cuda:0")

    def composed():
        for ids, lo, hi, sel in per_level:
            in0, in1 = vals[:, lo].contiguous(), vals[:, hi].contiguous()
            ctx.cmux_dev(sels, sel, in0.data_ptr(), in1.data_ptr(), t_lv.data_ptr())
            vals[:, ids] = t_lv[:sel.size].view(Q, ids.numel(), N2)

    kt = 8
    t_table = dev_i32(tfhe_amd.lookup_table_pack_bits(p, g.permutation(1 << kt).astype(np.uint64) & 0xFF, 8))
    t_tree = torch.zeros((Q, N2), dtype=torch.int32, device="cuda:0")
    tree_addr = np.ascontiguousarray(addr[:, :kt])

    def tree():
        ctx.table_lookup_dev(sels, tree_addr, t_table.data_ptr(), t_tree.data_ptr())

    # equal outputs first, and the right answers
    graph()
    ctx.sync()
    graph_kernels = ctx.last_kernels()
    composed()
    ctx.sync()
    out = t_out.cpu().numpy().view(np.uint32)[:, 0]
    identical = bool(np.array_equal(out, vals[:, gr.roots[0]].cpu().numpy().view(np.uint32)))
    dec = ctx.trlwe_decrypt_bool(sk.key_lv1, out[:16])[:, 0]
    correct = all(bool(dec[q]) == bool(gr.evaluate_plain(sel_bit[addr[q]])[0][0]) for q in range(16))
    if not (identical and correct):
        raise SystemExit(f"cmux_graph_bench.py: outputs identical={identical} correct={correct}; nothing timed")
    forms = {"graph": graph, "composed": composed, "tree": tree}
    for fn in forms.values():
        for _ in range(args.warmup):
            fn()
    ctx.sync()
    ms = {name: [] for name in forms}
    while min(sum(t) for t in ms.values()) < args.seconds * 1e3:  # alternating, one call each
        for name, fn in forms.items():
            ms[name].append(timed(fn))
    ctx.sync()
    ctx.set_stream(None)
    cmuxes = {"graph": Q * V, "composed": Q * V, "tree": Q * ((1 << kt) - 1)}
    report = {}
    for name in forms:
        med = float(np.median(ms[name]))
        report[name] = {"calls": len(ms[name]), "ms_median": round(med, 4), "ms_min": round(min(ms[name]), 4),
                        "ms_max": round(max(ms[name]), 4), "cmux_per_call": cmuxes[name],
                        "cmux_per_s": round(cmuxes[name] / med * 1e3, 1)}
    report["graph"]["kernels"] = graph_kernels
    line = {"metric": f"{args.bits}-bit encrypted comparisons/sec (a < b as a CMUX graph, set {pname}) on one MI355X",
            "value": round(Q / report["graph"]["ms_median"] * 1e3, 1), "unit": "comparisons/s", "queries": Q,
            "selectors": S, "graph": {"nodes": V, "depth": depth, "n_slots": n_slots, "widest_level": int(widest)},
            "forms": report, "outputs_identical": identical, "decrypt_check": correct,
            "graph_over_composed_time": round(report["graph"]["ms_median"] / report["composed"]["ms_median"], 4),
            "graph_cmux_rate_over_tree": round(report["graph"]["cmux_per_s"] / report["tree"]["cmux_per_s"], 4),
            "chain_form": "not built",
            "timing": f"device events around each call, the three forms alternating, >= {args.seconds} s per form after "
                      f"{args.warmup} warm-up calls; medians", "build_id": tfhe_amd.build_id()}
    sels.close()
    ctx.close()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
