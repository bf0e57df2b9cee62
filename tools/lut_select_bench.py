#!/usr/bin/env python3
"""Select nodes inside the LUT-circuit evaluator against the flat calls they replace, on one MI355X: one JSON line.

products: --pairs (1,024) products of two 4-bit digits at UINT4, m = 16, both halves (x * y mod 16 and x * y >> 4),
device-resident, in three forms:

  circuit      one LutCircuit of 2 * pairs node2 (run_dev): level 1 the 16 ordinary nodes of every node2, level 2
               the select nodes
  apply2       Context.lut_apply2_dev over the same 2 * pairs nodes
  composed     the per-level composition from the flat entries: lut_apply_dev (level 1), lut_select_dev (level 2)

mixed: a circuit of --levels (4) levels of 8 ordinary and 8 select nodes each, every level reading the one before
it, against the same per-level composition (lut_apply_dev and lut_select_dev per level).  The circuit runs one
blind-rotation launch per level where the composition runs two.

The forms' outputs are compared word for word before anything is timed.  Times are device events on torch's stream
around each call, the forms alternating call by call, medians of at least --seconds of warmed work per form.

    python tools/lut_select_bench.py [--out profiles/lut_select_bench.json]
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


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


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


def one_term_nodes(src, lut):
    n = len(src)
    return tfhe_amd.LutNodes(np.arange(n + 1), src, np.ones(n), np.zeros(n), lut)


def products(ctx, sk, key, args):
    """-> (forms, check): the three forms of 2 * pairs bivariate nodes, and check() -> their outputs agree and decrypt."""
    B, n1, p = args.pairs, ctx.n1, ctx.params
    lo, hi = (lambda x, y: (x * y) % M), (lambda x, y: (x * y) // M)
    ls = tfhe_amd.LutSet(ctx, np.concatenate([tfhe_amd.lut_generate2(p, M, lo), tfhe_amd.lut_generate2(p, M, hi)]))
    g = np.random.default_rng(12)
    xv, yv = g.integers(0, M, B).astype(np.uint32), g.integers(0, M, B).astype(np.uint32)
    inputs = np.concatenate([sk.encrypt_lwe_message(xv, M, seed0=70_000), sk.encrypt_lwe_message(yv, M, seed0=70_000 + B)])
    nodes = 2 * B  # node k: function k // B of pair k % B
    at = np.arange(nodes, dtype=np.uint32) % B
    fn = (np.arange(nodes, dtype=np.uint32) // B).astype(np.uint32)
    circ = tfhe_amd.LutCircuit()
    for _ in range(2 * B):
        circ.input()
    circ.output(*[circ.node2(int(fn[k]) * M, [(int(at[k]), 1)], [(int(at[k]) + B, 1)], M) for k in range(nodes)])
    packed, sel, ow = circ.packed(), circ.select_arrays(), np.array(circ.outputs, np.uint32)
    theta = np.zeros(packed.B, np.uint32)
    # the composition: level 1 writes behind the inputs in one pool, level 2 selects from it
    level1 = one_term_nodes(np.repeat(at + B, M), (np.repeat(fn, M) * M + np.tile(np.arange(M, dtype=np.uint32), nodes)))
    first = 2 * B + np.arange(nodes, dtype=np.uint32) * M
    level2 = tfhe_amd.LutNodes(np.arange(nodes + 1), at, np.ones(nodes), np.zeros(nodes), np.zeros(nodes))
    sel_src = (first[:, None] + np.arange(M, dtype=np.uint32)).reshape(-1).astype(np.uint32)
    sel_konst = np.zeros(nodes * M, np.uint32)
    t_pool = torch.zeros((2 * B + nodes * M, n1), dtype=torch.int32, device="cuda:0")
    t_pool[:2 * B] = dev_i32(inputs)
    t_out = {k: torch.zeros((nodes, n1), dtype=torch.int32, device="cuda:0") for k in ("circuit", "apply2", "composed")}
    u32p = tfhe_amd.u32p
    level1_out = t_pool.data_ptr() + 2 * B * n1 * 4

    def composed():
        ctx.lut_apply_dev(ls, t_pool.data_ptr(), 2 * B, level1, level1_out)
        ctx.check(ctx.lib.tfhe_gpu_lut_select_dev(ctx.h, key.h, M, tfhe_amd.vp(t_pool.data_ptr()), t_pool.shape[0],
                                                  *level2.pointers()[:4], sel_src.ctypes.data_as(u32p),
                                                  sel_konst.ctypes.data_as(u32p), tfhe_amd.vp(t_out["composed"].data_ptr()),
                                                  nodes), "lut_select_dev")

    forms = {
        "circuit": lambda: ctx.lut_circuit_eval_select_dev(ls, key, M, t_pool.data_ptr(), 2 * B, packed, theta, sel, ow,
                                                           t_out["circuit"].data_ptr()),
        "apply2": lambda: ctx.lut_apply2_dev(ls, key, M, t_pool.data_ptr(), 2 * B, (fn, at, at + B),
                                             t_out["apply2"].data_ptr()),
        "composed": composed,
    }

    def check():
        outs = {k: host_u32(t) for k, t in t_out.items()}
        dec = sk.decrypt_lwe_message(outs["circuit"], M)
        want = np.concatenate([(xv * yv) % M, (xv * yv) // M])
        return (int((dec != want).sum()), np.array_equal(outs["circuit"], outs["apply2"]),
                np.array_equal(outs["circuit"], outs["composed"]))

    return forms, check, ls


def mixed(ctx, sk, key, args):
    """-> (forms, check): `levels` levels of 8 ordinary and 8 select nodes, as one circuit and composed per level."""
    L, n1, p = args.levels, ctx.n1, ctx.params
    ls = tfhe_amd.LutSet(ctx, np.array([tfhe_amd.lut_generate(p, M, lambda x, j=j: (x + j) % M) for j in range(8)]))
    inputs = sk.encrypt_lwe_message(np.random.default_rng(13).integers(0, M, 16).astype(np.uint32), M, seed0=80_000)
    circ = tfhe_amd.LutCircuit()
    prev = [circ.input() for _ in range(16)]
    for _ in range(L):
        nxt = [circ.node(j, [(prev[j], 1)]) for j in range(8)]
        nxt += [circ.select([(prev[8 + j], 1)], prev[j:] + prev[:j]) for j in range(8)]
        prev = nxt
    circ.output(*prev)
    packed, sel, ow = circ.packed(), circ.select_arrays(), np.array(circ.outputs, np.uint32)
    theta = np.zeros(packed.B, np.uint32)
    # per level over the 16 ciphertexts of the level before: 8 ordinary nodes into rows 0..7, 8 select nodes into 8..15
    ordinary = one_term_nodes(np.arange(8, dtype=np.uint32), np.arange(8, dtype=np.uint32))
    digits = tfhe_amd.LutNodes(np.arange(9), np.arange(8, 16), np.ones(8), np.zeros(8), np.zeros(8))
    sel_src = np.array([(j + i) % 16 for j in range(8) for i in range(16)], np.uint32)
    sel_konst = np.zeros(8 * 16, np.uint32)
    t_lv = [dev_i32(inputs)] + [torch.zeros((16, n1), dtype=torch.int32, device="cuda:0") for _ in range(L)]
    t_circ = torch.zeros((16, n1), dtype=torch.int32, device="cuda:0")
    u32p = tfhe_amd.u32p

    def composed():
        for lv in range(L):
            src, dst = t_lv[lv].data_ptr(), t_lv[lv + 1].data_ptr()
            ctx.lut_apply_dev(ls, src, 16, ordinary, dst)
            ctx.check(ctx.lib.tfhe_gpu_lut_select_dev(ctx.h, key.h, M, tfhe_amd.vp(src), 16, *digits.pointers()[:4],
                                                      sel_src.ctypes.data_as(u32p), sel_konst.ctypes.data_as(u32p),
                                                      tfhe_amd.vp(dst + 8 * n1 * 4), 8), "lut_select_dev")

    forms = {
        "circuit": lambda: ctx.lut_circuit_eval_select_dev(ls, key, M, t_lv[0].data_ptr(), 16, packed, theta, sel, ow,
                                                           t_circ.data_ptr()),
        "composed": composed,
    }
    return forms, (lambda: np.array_equal(host_u32(t_circ), host_u32(t_lv[L]))), ls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed device work per form, at least")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lut_select_bench.py: no GPU (a rate is measured on the MI355X or not at all)")
    ctx = tfhe_amd.Context("uint4", 0)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    key = tfhe_amd.PackingKey.generate(ctx, sk, seed0=50_000)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    prod_forms, prod_check, ls_p = products(ctx, sk, key, args)
    mix_forms, mix_check, ls_m = mixed(ctx, sk, key, args)
    kernels = {}
    for name, fn in list(prod_forms.items()) + [("mixed_" + k, f) for k, f in mix_forms.items()]:
        fn()
        kernels[name] = ctx.last_kernels()
    ctx.sync()
    wrong, eq_apply2, eq_composed = prod_check()
    eq_mixed = mix_check()
    if wrong or not (eq_apply2 and eq_composed and eq_mixed):
        raise SystemExit(f"lut_select_bench.py: {wrong} of {2 * args.pairs} digits wrong, circuit == apply2: {eq_apply2}, "
                         f"circuit == composed: {eq_composed}, mixed circuit == composed: {eq_mixed}; nothing timed")
    print("outputs equal and correct; timing the products", file=sys.stderr, flush=True)
    ms = alternate(prod_forms, args.seconds, args.warmup)
    print("products timed; timing the mixed circuit", file=sys.stderr, flush=True)
    mms = alternate(mix_forms, args.seconds, args.warmup)
    ctx.sync()
    ctx.set_stream(None)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    mmed = {k: float(np.median(v)) for k, v in mms.items()}
    line = {"metric": f"LUT circuit of node2 over lut_apply2 (UINT4, {args.pairs} products, both digits, m = {M}, "
                      "device-resident) on one MI355X",
            "value": round(med["circuit"] / med["apply2"], 4), "unit": "x",
            "pairs": args.pairs, "m": M, "bootstraps_per_call": 2 * args.pairs * (M + 1),
            "forms": {k: dict(stats(v), kernels=kernels[k]) for k, v in ms.items()},
            "circuit_over_apply2": round(med["circuit"] / med["apply2"], 4),
            "circuit_over_composed": round(med["circuit"] / med["composed"], 4),
            "mixed": {"levels": args.levels, "ordinary_per_level": 8, "select_per_level": 8,
                      "forms": {k: dict(stats(v), kernels=kernels["mixed_" + k]) for k, v in mms.items()},
                      "circuit_over_composed": round(mmed["circuit"] / mmed["composed"], 4),
                      "ms_saved_per_level": round((mmed["composed"] - mmed["circuit"]) / args.levels, 4)},
            "outputs_equal_and_correct": True,
            "timing": f"device events around each call, the forms alternating, >= {args.seconds} s per form after "
                      f"{args.warmup} warm-up calls; medians", "build_id": tfhe_amd.build_id()}
    for x in (ls_p, ls_m, key):
        x.close()
    ctx.close()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
