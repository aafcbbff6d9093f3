#!/usr/bin/env python
"""One optimiser step of the layer-wise rules over the ViT-B/16 parameters (bf16 parameters, fp32
masters and states, bucketed as the DDP engine buckets them), next to the rules they extend, in
one process:

  momentum, lars (fold in the apply kernel's prologue), lars (fold as a launch of its own),
  adam,     lamb (prologue),                            lamb (launch)

Each engine's ``DDP.step`` on preset gradients is captured in a HIP graph and the replays are timed
with device events (no host launch gaps); the variants are alternated over the rounds so that drift
of a shared machine hits all alike. The kernels are bandwidth-bound. Per element Momentum moves 20
bytes (gradient 2, master 4 + 4, velocity 4 + 4, parameter 2) and Adam 28; LARS adds a statistics
pass over the gradient and the master (6: 26 in all); LAMB's statistics pass reads the gradient, the
master and both moments and writes the moments (22) and its apply pass reads the moments and the
master and writes the master and the parameter (18: 40 in all). The 1-D leaves (biases, norm scales)
take Momentum's / Adam's kernel. ``expected_us`` is the base rule's time scaled by the bytes. One
JSON line per variant.

usage: python scripts/bench_layerwise.py [--out profiles/layerwise_vit_b16.jsonl] [--rounds 5] [--iters 20]
       rocprofv3 --kernel-trace --stats ... -- python scripts/bench_layerwise.py --trace lars,lamb
         (20 eager steps of each named rule and nothing else: per-kernel times)
       python scripts/bench_layerwise.py --fold-sweep 256,576,1024,... [--out profiles/layerwise_fold_sweep.jsonl]
         (one leaf of that many 4096-element chunks through ops.optim.lars_ / lamb_, both fold variants:
          where the prologue's re-read of the leaf's partials starts to cost more than a launch)
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluxmpi_amd import optimisers as O  # noqa: E402
from fluxmpi_amd.parallel.ddp import DDP  # noqa: E402
from scripts.bench_rules import graphed, model_bf16, set_grads, timed  # noqa: E402

# name -> (rule, base rule's name, bytes per adapted element, per 1-D element, fold variant)
VARIANTS = {
    "momentum": (lambda: O.Momentum(0.1, 0.9), "momentum", 20, 20, None),
    "lars/prologue": (lambda: O.LARS(0.1, 0.9, trust=0.001, decay=1e-4), "momentum", 26, 20, "prologue"),
    "lars/launch": (lambda: O.LARS(0.1, 0.9, trust=0.001, decay=1e-4), "momentum", 26, 20, "launch"),
    "adam": (lambda: O.Adam(1e-3), "adam", 28, 28, None),
    "lamb/prologue": (lambda: O.LAMB(1e-3), "adam", 40, 28, "prologue"),
    "lamb/launch": (lambda: O.LAMB(1e-3), "adam", 40, 28, "launch"),
}


def fold_sweep(a):
    """One leaf per call, the engine's layout (bf16 parameter and gradient, fp32 master and states)."""
    from fluxmpi_amd.ops import optim
    out = a.out if a.out != DEFAULT_OUT else os.path.join("profiles", "layerwise_fold_sweep.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    with open(out, "w") as f:
        for chunks in [int(c) for c in a.fold_sweep.split(",")]:
            n = chunks * 4096
            fns, keep = {}, []
            for rule in ("lars", "lamb"):
                for fold in ("prologue", "launch"):
                    w = torch.randn(n, device="cuda", generator=gen)
                    p, g = [w.bfloat16()], [(torch.randn(n, device="cuda", generator=gen) * 1e-2).bfloat16()]
                    m, v = [torch.zeros_like(w)], [torch.zeros_like(w)]
                    q, ws = torch.ones(1, device="cuda"), torch.empty(2 * chunks, device="cuda")
                    if rule == "lars":
                        hyper = torch.tensor([0.1], device="cuda")
                        step = lambda p=p, g=g, m=m, w=w, q=q, ws=ws, hyper=hyper: optim.lars_(  # noqa: E731
                            p, g, m, lr=0.1, momentum=0.9, trust=0.001, weight_decay=1e-4, masters=[w],
                            dev_hyper=hyper, ratios=q, workspace=ws)
                    else:
                        hyper = torch.tensor([1e-3, 0.9, 0.999], device="cuda")
                        step = lambda p=p, g=g, m=m, v=v, w=w, q=q, ws=ws, hyper=hyper: optim.lamb_(  # noqa: E731
                            p, g, m, v, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-6, bt1=0.0, bt2=0.0, weight_decay=0.01,
                            masters=[w], dev_hyper=hyper, ratios=q, workspace=ws)
                    os.environ["FLUXMPI_LAYERWISE_FOLD"] = fold
                    fns[f"{rule}/{fold}"] = graphed(step)
                    keep.append((p, g, m, v, w, q, ws, hyper))
            os.environ["FLUXMPI_LAYERWISE_FOLD"] = "auto"
            us = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    us[k].append(timed(fn, a.iters))
            for rule in ("lars", "lamb"):
                pro, lau = statistics.median(us[f"{rule}/prologue"]), statistics.median(us[f"{rule}/launch"])
                line = json.dumps({"rule": rule, "chunks": chunks, "elements": n, "prologue_us": round(pro, 1),
                                   "launch_us": round(lau, 1), "launch_minus_prologue_us": round(lau - pro, 1),
                                   "partials_reread_per_workgroup_bytes": 8 * chunks, "rounds": a.rounds,
                                   "iters": a.iters})
                print(line, flush=True)
                f.write(line + "\n")
            del fns, keep
            torch.cuda.empty_cache()
    return 0


DEFAULT_OUT = os.path.join("profiles", "layerwise_vit_b16.jsonl")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--trace", default="", help="rules (momentum, lars, adam, lamb) to step eagerly 20 times, "
                                                "for a kernel trace; nothing is timed")
    ap.add_argument("--fold-sweep", default="", help="leaf sizes in chunks: time one leaf with both fold variants")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_layerwise.py needs a GPU", file=sys.stderr)
        return 2
    if a.fold_sweep:
        return fold_sweep(a)
    if a.trace:
        for name in a.trace.split(","):
            m = model_bf16(0)
            d = DDP(m, VARIANTS[name if name in VARIANTS else name + "/prologue"][0](), average=True, overlap_opt=False)
            set_grads(m, 1)
            for _ in range(20):
                d.step(zero_grad=False)
            torch.cuda.synchronize()
        return 0
    fns, info, keep = {}, {}, []
    for name, (rule, base, per, per_1d, fold) in VARIANTS.items():
        m = model_bf16(0)
        d = DDP(m, rule(), average=True, overlap_opt=False)
        set_grads(m, 1)
        # the fold variant is chosen when the kernels are enqueued, i.e. at capture
        os.environ["FLUXMPI_LAYERWISE_FOLD"] = fold or "auto"
        fns[name] = graphed(lambda d=d: d.step(zero_grad=False))
        keep.append(d)
        n1 = sum(p.numel() for b in d.buckets for i, p in enumerate(b.params) if fold and i in b.plain)
        nad = d.num_parameters() - n1
        info[name] = {"base": base, "elements": d.num_parameters(), "elements_1d": n1, "buckets": len(d.buckets),
                      "leaves": sum(len(b.params) for b in d.buckets),
                      "largest_leaf_chunks": max((p.numel() + 4095) // 4096 for b in d.buckets for p in b.params),
                      "bytes_per_element": per, "bytes": nad * per + n1 * per_1d}
    os.environ["FLUXMPI_LAYERWISE_FOLD"] = "auto"
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            us[k].append(timed(fn, a.iters))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for k, v in us.items():
            med = statistics.median(v)
            r = {"rule": k, "us": round(med, 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                 "rounds": a.rounds, "iters": a.iters, **info[k]}
            b = info[r["base"]]
            r["TBps"] = round(r["bytes"] / med / 1e6, 2)
            r["expected_us"] = round(statistics.median(us[r["base"]]) * r["bytes"] / b["bytes"], 1)
            r["vs_expected_pct"] = round(100.0 * (med - r["expected_us"]) / r["expected_us"], 1)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
