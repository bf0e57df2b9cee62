#!/usr/bin/env python3
"""The extended LUT bootstrap against the ordinary one at equal external products, on one MI355X: one JSON line.

UINT4, --items (1,024) device-resident inputs, in four forms:

  ext1 / ext2      Context.lut_apply_ext_dev with eta = 1 (m = 32) and eta = 2 (m = 64): one node per input, one term
                   each; the combination launch, k_blind_rotate_ext<1,E>, the extraction and the key switch
  yard1 / yard2    Context.bootstrap_lut_batch_dev over E * items inputs in the octo form: the same number of external
                   products (E * items * n), run by the tuned blind rotation, and E times the key switches

Before anything is timed every extended output is decrypted against f(x) and the first items are compared word for
word with the stage entry's acc_0, extracted and key-switched; the yardstick's outputs are decrypted too.  Times are
device events on torch's stream around each call, the forms alternating call by call, medians of at least --seconds
of warmed work per form.

    python tools/lut_ext_bench.py [--out profiles/lut_ext_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed device work per form, at least")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lut_ext_bench.py: no GPU (a rate is measured on the MI355X or not at all)")
    ctx = tfhe_amd.Context("uint4", 0)
    sk, _ = ctx.keygen(secret_seed=42, cloud_seed=43)
    p, B, n1 = ctx.params, args.items, ctx.n1
    g = np.random.default_rng(14)

    forms, checks, kernels, keep = {}, {}, {}, []
    for eta in (1, 2):
        E, m = 1 << eta, 16 << eta
        f = lambda x, m=m: (7 * x + 3) % m  # noqa: E731
        tv = tfhe_amd.lut_generate_ext(p, eta, m, f)
        ls = tfhe_amd.LutSet(ctx, tv)
        msgs = g.integers(0, m, B).astype(np.uint32)
        cts = sk.encrypt_lwe_message(msgs, m, seed0=90_000 * eta)
        nodes = tfhe_amd.LutNodes(np.arange(B + 1), np.arange(B), np.ones(B), np.zeros(B), np.zeros(B))
        t_in, t_out = dev_i32(cts), torch.zeros((B, n1), dtype=torch.int32, device="cuda:0")
        forms[f"ext{eta}"] = (lambda ls=ls, eta=eta, t_in=t_in, nodes=nodes, t_out=t_out:
                              ctx.lut_apply_ext_dev(ls, eta, t_in.data_ptr(), B, nodes, t_out.data_ptr()))
        # the yardstick: E * B ordinary bootstraps at m = 16
        ym = g.integers(0, 16, E * B).astype(np.uint32)
        y_in = dev_i32(sk.encrypt_lwe_message(ym, 16, seed0=95_000 * eta))
        y_tv = dev_i32(tfhe_amd.lut_generate(p, 16, lambda x: (7 * x + 3) % 16))
        y_out = torch.zeros((E * B, n1), dtype=torch.int32, device="cuda:0")
        forms[f"yard{eta}"] = (lambda y_in=y_in, y_tv=y_tv, y_out=y_out, E=E:
                               ctx.bootstrap_lut_batch_dev(y_in.data_ptr(), y_tv.data_ptr(), y_out.data_ptr(), E * B))

        def check(eta=eta, m=m, f=f, tv=tv, cts=cts, msgs=msgs, t_out=t_out, ym=ym, y_out=y_out):
            out = host_u32(t_out)
            wrong = int((sk.decrypt_lwe_message(out, m) != np.array([f(int(x)) for x in msgs], np.uint32)).sum())
            acc = ctx.blind_rotate_ext(eta, cts[:8], tv)
            same = np.array_equal(out[:8], ctx.sample_extract(acc[:, 0], [0], key_switch=True).reshape(8, n1))
            ywrong = int((sk.decrypt_lwe_message(host_u32(y_out), 16) != (7 * ym + 3) % 16).sum())
            return wrong, same, ywrong
        checks[eta] = check
        keep.append(ls)

    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    with ctx.options(br_form="octo"):
        for name, fn in forms.items():
            fn()
            kernels[name] = ctx.last_kernels()
        ctx.sync()
        ctx.set_stream(None)
        for eta, check in checks.items():
            wrong, same, ywrong = check()
            if wrong or ywrong or not same:
                raise SystemExit(f"lut_ext_bench.py: eta = {eta}: {wrong} of {B} digits wrong, first items equal the "
                                 f"stage composition: {same}, {ywrong} yardstick digits wrong; nothing timed")
        print("outputs equal and correct; timing", file=sys.stderr, flush=True)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ms = alternate(forms, args.seconds, args.warmup)
        ctx.sync()
        ctx.set_stream(None)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    steps = {eta: B * p.n * (1 << eta) for eta in (1, 2)}  # external products per call, both forms
    line = {"metric": f"extended LUT bootstrap over the ordinary one at equal external products (UINT4, {B} items, "
                      "eta = 2 against 4x the items in the octo form, device-resident) on one MI355X",
            "value": round(med["ext2"] / med["yard2"], 4), "unit": "x", "items": B,
            "forms": {k: dict(stats(v), kernels=kernels[k]) for k, v in ms.items()},
            "ext_over_yardstick": {f"eta{eta}": round(med[f"ext{eta}"] / med[f"yard{eta}"], 4) for eta in (1, 2)},
            "ns_per_external_product": {k: round(med[k] * 1e6 / steps[int(k[-1])], 4) for k in med},
            "external_products_per_s": {k: round(steps[int(k[-1])] / (med[k] * 1e-3)) for k in med},
            "us_per_item": {k: round(med[k] * 1e3 / B, 3) for k in ("ext1", "ext2")},
            "outputs_equal_and_correct": True,
            "timing": f"device events around each call, the forms alternating, >= {args.seconds} s per form after "
                      f"{args.warmup} warm-up calls; medians; a call is the whole entry (ext: combination, blind "
                      "rotation, extraction, key switch; yardstick: blind rotation, key switch over E x the items)",
            "build_id": tfhe_amd.build_id()}
    for x in keep:
        x.close()
    ctx.close()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
