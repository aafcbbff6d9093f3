#!/usr/bin/env python
"""Cost of gradient clipping in one optimiser step over the ViT-B/16 parameters (bf16 parameters,
fp32 masters and Adam moments, bucketed as the DDP engine buckets them), four variants alternated
in one process:

  adam            fused Adam, no clipping (one launch per bucket)
  clipnorm_adam   DDP(OptimiserChain(ClipNorm(1.0), Adam)): the two-launch sum of squares over
                  the leaves of all buckets + the global sum, then the fused updates with
                  per-leaf scales
  global_adam     DDP(Adam, clip_global_norm=1.0): the same sums of squares, then the updates
                  reading one device scalar
  per_leaf_chain  OptimiserChain(ClipNorm(1.0), Adam()) through the generic per-leaf
                  ``AbstractRule.apply_batch`` (what the chain cost before the fused form)

Each engine variant is timed eagerly (``DDP.step`` on preset gradients, device events) and as a
HIP-graph replay of the same step (no host launch gaps). Bytes are computed from the shapes: the
update moves the gradient, master, m, v (read), master, m, v and the parameter (written); the clip
adds one read of the gradient. One JSON line per variant.

usage: python scripts/bench_clip.py [--out profiles/clip_vit_b16.jsonl] [--rounds 5] [--iters 20] [--no-per-leaf]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluxmpi_amd import optimisers as O  # noqa: E402
from fluxmpi_amd.models.vit import vit_b16  # noqa: E402
from fluxmpi_amd.parallel.ddp import DDP  # noqa: E402


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def model_bf16(seed):
    torch.manual_seed(seed)
    m = vit_b16().cuda()
    for p in m.parameters():
        p.data = p.data.to(torch.bfloat16)
    return m


def set_grads(model, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for p in model.parameters():
        p.grad = (torch.randn(p.shape, device="cuda", generator=g) * 1e-2).to(p.dtype)


def graphed(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        step()
    return gr.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "clip_vit_b16.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-per-leaf", action="store_true", help="skip the per-leaf chain (short kernel traces)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_clip.py needs a GPU", file=sys.stderr)
        return 2
    engines = {
        "adam": lambda m: DDP(m, O.Adam(1e-3), average=True, overlap_opt=False),
        "clipnorm_adam": lambda m: DDP(m, O.OptimiserChain(O.ClipNorm(1.0), O.Adam(1e-3)), average=True,
                                       overlap_opt=False),
        "global_adam": lambda m: DDP(m, O.Adam(1e-3), average=True, clip_global_norm=1.0),
    }
    fns, info = {}, {}
    for name, make in engines.items():
        m = model_bf16(0)
        d = make(m)
        set_grads(m, 1)
        step = (lambda d=d: d.step(zero_grad=False))
        fns[name] = step
        fns[name + "/graph"] = graphed(step)
        n = d.num_parameters()
        leaves = sum(len(b.params) for b in d.buckets)
        upd = sum(b.numel * (2 * b.flat_grad.element_size() + (2 * 4 if b.master is not None else b.flat_grad.element_size())
                             + 4 * b.exp_avg.element_size()) for b in d.buckets)
        clip = 0 if name == "adam" else sum(p.numel() * p.element_size() for b in d.buckets for p in b.params)
        info[name] = info[name + "/graph"] = {"elements": n, "leaves": leaves, "buckets": len(d.buckets),
                                              "bytes_update": upd, "bytes_clip": clip}
    # the generic per-leaf path of the same chain (bf16 leaves, Optimisers.jl zero(x) state)
    m = model_bf16(0)
    set_grads(m, 1)
    chain = O.OptimiserChain(O.ClipNorm(1.0), O.Adam(1e-3))
    items = [(O.Leaf(chain, chain.init(p.data)), p.data, p.grad) for p in m.parameters()]

    def per_leaf():
        with torch.no_grad():
            for (_, x, _), dx in zip(items, O.AbstractRule.apply_batch(chain, items)):
                x.sub_(dx.to(x.dtype))

    if not a.no_per_leaf:
        fns["per_leaf_chain"] = per_leaf
        info["per_leaf_chain"] = {"elements": sum(p.numel() for p in m.parameters()), "leaves": len(items)}

    for fn in fns.values():  # warm-up of every variant
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(a.rounds):  # alternate the variants: drift of the shared machine hits all alike
        for k, fn in fns.items():
            us[k].append(timed(fn, a.iters if k != "per_leaf_chain" else max(2, a.iters // 5)))
    base = statistics.median(us["adam/graph"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for k, v in us.items():
            med = statistics.median(v)
            r = {"variant": k, "us": round(med, 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                 "rounds": a.rounds, "iters": a.iters, **info[k]}
            if "bytes_update" in r:
                r["TBps"] = round((r["bytes_update"] + r["bytes_clip"]) / med / 1e6, 2)
                # what one more read of the gradient should cost at the plain update's rate
                r["clip_expected_pct"] = round(100.0 * r["bytes_clip"] / r["bytes_update"], 1)
                if k.endswith("/graph"):
                    r["over_adam_graph_pct"] = round(100.0 * (med - base) / base, 1)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
