#!/usr/bin/env python3
"""Extended nodes inside the LUT-circuit evaluator against the flat calls they replace, on one MI355X: one JSON line.

mixed: a circuit of --levels (4) levels of --items (1,024) nodes each at UINT4, every level reading the one before
it.  A level holds 320 ordinary nodes at eta = 0, 320 at eta = 1 and 256 at eta = 2, and 64 select nodes of m = 32
entries at eta = 1 and 64 at eta = 2 (the shares scale with --items).  Two forms:

  circuit      one LutCircuit (run_dev): per level one combination launch, one pack over the 128 select nodes, the
               eta = 0 launch, one k_blind_rotate_ext launch per eta, one extraction and one key switch
  composed     the same work per level from the flat entries: lut_apply_dev, lut_apply_ext_dev (eta = 1, 2) and
               lut_select_ext_dev (eta = 1, 2)

table: --items (1,024) reads of a 64-entry table of encrypted 6-bit words, each by its own encrypted address:

  ext          one select node of m = 64 entries at eta = 2 per read: 1 bootstrap and 1 pack
  nested       the reach of eta = 0: the address as two base-8 digits, 8 select nodes of m = 8 over the low digit and
               one over the high digit per read: 9 bootstraps and 9 packs, depth 2

The mixed forms' outputs are compared word for word before anything is timed; the table forms are different
computations, so each is decrypted and its wrong reads are counted.  Times are device events on torch's stream around
each call, the forms alternating call by call, medians of at least --seconds of warmed work per form.

    python tools/lut_circuit_ext_bench.py [--out profiles/lut_circuit_ext_bench.json]
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

M_MIX, M_TAB = 32, 64


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


def shares(items):
    """(eta 0, eta 1, eta 2 ordinary, eta 1, eta 2 select) node counts of a level of `items` nodes."""
    s1 = s2 = max(1, items // 16)
    o2 = items // 4
    o0 = o1 = (items - o2 - s1 - s2) // 2
    return o0 + (items - o0 - o1 - o2 - s1 - s2), o1, o2, s1, s2


def mixed(ctx, sk, key, args):
    """-> (forms, check, set, description): `levels` levels of mixed nodes as one circuit and composed per level."""
    L, B, n1, p, m = args.levels, args.items, ctx.n1, ctx.params, M_MIX
    o0, o1, o2, s1, s2 = shares(B)
    fs = [lambda x: (3 * x + 1) % m, lambda x: (x * x + 5) % m]
    ls = tfhe_amd.LutSet(ctx, np.concatenate([tfhe_amd.lut_generate_ext(p, 2, m, f) for f in fs]))  # 8 entries
    inputs = sk.encrypt_lwe_message(np.random.default_rng(13).integers(0, m, B).astype(np.uint32), m, seed0=80_000)
    ents = lambda j: [(j + 7 * i) % B for i in range(m)]  # noqa: E731  (rows of the level before)
    circ = tfhe_amd.LutCircuit()
    prev = [circ.input() for _ in range(B)]
    for _ in range(L):
        nxt, j = [], 0
        for count, eta, luts in ((o0, 0, 8), (o1, 1, 4), (o2, 2, 2)):
            for _k in range(count):
                nxt.append(circ.node(j % luts, [(prev[j], 1)], eta=eta))
                j += 1
        for count, eta in ((s1, 1), (s2, 2)):
            for _k in range(count):
                nxt.append(circ.select([(prev[j], 1)], [prev[e] for e in ents(j)], eta=eta))
                j += 1
        prev = nxt
    circ.output(*prev)
    packed, sel, ow = circ.packed(), circ.select_arrays(), np.array(circ.outputs, np.uint32)
    theta = np.zeros(packed.B, np.uint32)
    # the composition: five flat calls per level over the B ciphertexts of the level before, rows in the same order
    bounds = np.cumsum([0, o0, o1, o2, s1, s2])
    rows = [np.arange(bounds[k], bounds[k + 1], dtype=np.uint32) for k in range(5)]
    flat = [tfhe_amd.LutNodes(np.arange(r.size + 1), r, np.ones(r.size), np.zeros(r.size), r % luts)
            for r, luts in zip(rows[:3], (8, 4, 2))]
    # the select calls' arrays built once: the timed calls go straight to the C entries
    sel_nodes = [tfhe_amd._select_nodes([([(int(j), 1)], ents(int(j))) for j in r], m) for r in rows[3:]]
    u32p, eta_arr = tfhe_amd.u32p, np.array(circ.eta, np.uint32)
    t_lv = [dev_i32(inputs)] + [torch.zeros((B, n1), dtype=torch.int32, device="cuda:0") for _ in range(L)]
    t_circ = torch.zeros((B, n1), dtype=torch.int32, device="cuda:0")

    def select_ext(eta, src, nodes, dst):
        d, ssrc, skonst = nodes
        ctx.check(ctx.lib.tfhe_gpu_lut_select_ext_dev(ctx.h, key.h, m, eta, tfhe_amd.vp(src), B, *d.pointers()[:4],
                                                      ssrc.ctypes.data_as(u32p), skonst.ctypes.data_as(u32p),
                                                      tfhe_amd.vp(dst), d.B), "lut_select_ext_dev")

    def composed():
        for lv in range(L):
            src, dst = t_lv[lv].data_ptr(), t_lv[lv + 1].data_ptr()
            at = lambda k: dst + int(bounds[k]) * n1 * 4  # noqa: E731
            ctx.lut_apply_dev(ls, src, B, flat[0], at(0))
            ctx.lut_apply_ext_dev(ls, 1, src, B, flat[1], at(1))
            ctx.lut_apply_ext_dev(ls, 2, src, B, flat[2], at(2))
            select_ext(1, src, sel_nodes[0], at(3))
            select_ext(2, src, sel_nodes[1], at(4))

    forms = {
        "circuit": lambda: ctx.lut_circuit_eval_ext_dev(ls, key, m, t_lv[0].data_ptr(), B, packed, theta, sel, eta_arr,
                                                        ow, t_circ.data_ptr()),
        "composed": composed,
    }
    desc = {"levels": L, "nodes_per_level": B, "m": m, "ordinary_eta0": o0, "ordinary_eta1": o1, "ordinary_eta2": o2,
            "select_eta1": s1, "select_eta2": s2}
    return forms, (lambda: np.array_equal(host_u32(t_circ), host_u32(t_lv[L]))), ls, desc


def table(ctx, sk, key, args):
    """-> (forms, check, set): `items` reads of a 64-entry encrypted table, by one extended select node each and by
    the nested select nodes of eta = 0."""
    B, n1, p, m = args.items, ctx.n1, ctx.params, M_TAB
    g = np.random.default_rng(14)
    words, addr = g.integers(0, m, m).astype(np.uint32), g.integers(0, m, B).astype(np.uint32)
    ls = tfhe_amd.LutSet(ctx, tfhe_amd.lut_generate(p, m, lambda x: x))  # neither circuit has an ordinary node
    t_words = sk.encrypt_lwe_message(words, m, seed0=90_000)
    in_ext = np.concatenate([t_words, sk.encrypt_lwe_message(addr, m, seed0=91_000)])
    in_nest = np.concatenate([t_words, sk.encrypt_lwe_message(addr // 8, 8, seed0=92_000),
                              sk.encrypt_lwe_message(addr % 8, 8, seed0=93_000)])
    ext = tfhe_amd.LutCircuit()
    w = [ext.input() for _ in range(m + B)]
    ext.output(*[ext.select([(w[m + i], 1)], w[:m], eta=2) for i in range(B)])
    nest = tfhe_amd.LutCircuit()
    v = [nest.input() for _ in range(m + 2 * B)]
    for i in range(B):
        rows = [nest.select([(v[m + B + i], 1)], v[8 * r:8 * r + 8]) for r in range(8)]
        nest.output(nest.select([(v[m + i], 1)], rows))
    t_in = {"ext": dev_i32(in_ext), "nested": dev_i32(in_nest)}
    t_out = {k: torch.zeros((B, n1), dtype=torch.int32, device="cuda:0") for k in t_in}
    packs = {k: (c.packed(), c.select_arrays(), np.array(c.outputs, np.uint32), np.zeros(len(c.nodes), np.uint32))
             for k, c in (("ext", ext), ("nested", nest))}
    eta_arr = np.array(ext.eta, np.uint32)
    forms = {
        "ext": lambda: ctx.lut_circuit_eval_ext_dev(ls, key, m, t_in["ext"].data_ptr(), m + B, packs["ext"][0],
                                                    packs["ext"][3], packs["ext"][1], eta_arr, packs["ext"][2],
                                                    t_out["ext"].data_ptr()),
        "nested": lambda: ctx.lut_circuit_eval_select_dev(ls, key, 8, t_in["nested"].data_ptr(), m + 2 * B,
                                                          packs["nested"][0], packs["nested"][3], packs["nested"][1],
                                                          packs["nested"][2], t_out["nested"].data_ptr()),
    }

    def check():
        return {k: int((sk.decrypt_lwe_message(host_u32(t), m) != words[addr]).sum()) for k, t in t_out.items()}

    return forms, check, ls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1024)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed device work per form, at least")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lut_circuit_ext_bench.py: no GPU (a rate is measured on the MI355X or not at all)")
    if args.items < 64:
        raise SystemExit("lut_circuit_ext_bench.py: --items is at least 64")
    ctx = tfhe_amd.Context("uint4", 0)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    key = tfhe_amd.PackingKey.generate(ctx, sk, seed0=50_000)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    mix_forms, mix_check, ls_m, mix_desc = mixed(ctx, sk, key, args)
    tab_forms, tab_check, ls_t = table(ctx, sk, key, args)
    kernels = {}
    for name, fn in [("mixed_" + k, f) for k, f in mix_forms.items()] + [("table_" + k, f) for k, f in tab_forms.items()]:
        fn()
        kernels[name] = ctx.last_kernels()
    ctx.sync()
    eq_mixed, wrong = mix_check(), tab_check()
    if not eq_mixed or wrong["ext"] > args.items // 100:
        raise SystemExit(f"lut_circuit_ext_bench.py: mixed circuit == composed: {eq_mixed}, wrong reads {wrong} of "
                         f"{args.items}; nothing timed")
    print(f"mixed outputs equal, wrong reads {wrong}; timing the mixed circuit", file=sys.stderr, flush=True)
    mms = alternate(mix_forms, args.seconds, args.warmup)
    print("mixed circuit timed; timing the table reads", file=sys.stderr, flush=True)
    tms = alternate(tab_forms, args.seconds, args.warmup)
    ctx.sync()
    ctx.set_stream(None)
    mmed = {k: float(np.median(v)) for k, v in mms.items()}
    tmed = {k: float(np.median(v)) for k, v in tms.items()}
    line = {"metric": f"LUT circuit with extended nodes over its composition from the flat entries (UINT4, "
                      f"{args.levels} levels of {args.items} nodes, device-resident) on one MI355X",
            "value": round(mmed["circuit"] / mmed["composed"], 4), "unit": "x",
            "mixed": dict(mix_desc, forms={k: dict(stats(v), kernels=kernels["mixed_" + k]) for k, v in mms.items()},
                          circuit_over_composed=round(mmed["circuit"] / mmed["composed"], 4),
                          ms_saved_per_level=round((mmed["composed"] - mmed["circuit"]) / args.levels, 4),
                          outputs_equal=True),
            "table": {"reads": args.items, "entries": M_TAB,
                      "forms": {k: dict(stats(v), kernels=kernels["table_" + k], wrong_reads=wrong[k])
                                for k, v in tms.items()},
                      "bootstraps_per_read": {"ext": 1, "nested": 9},
                      "ext_over_nested": round(tmed["ext"] / tmed["nested"], 4)},
            "timing": f"device events around each call, the forms alternating, >= {args.seconds} s per form after "
                      f"{args.warmup} warm-up calls; medians", "build_id": tfhe_amd.build_id()}
    for x in (ls_m, ls_t, key):
        x.close()
    ctx.close()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
