#!/usr/bin/env python
"""Cost of loss scaling in one optimiser step over the ViT-B/16 parameters (bf16 parameters, fp32
masters and Adam moments, bucketed as the DDP engine buckets them), four variants alternated in
one process:

  adam               fused Adam (one launch per bucket)
  adam_ls            DDP(Adam, loss_scale=2^16): one multi-tensor non-finite check over every
                     bucket's gradient, the updates reading the skip flag and the inverse scale,
                     the scaler update
  global_adam        DDP(Adam, clip_global_norm=1.0): sums of squares, the fold, the updates
  global_adam_ls     the same with loss_scale=2^16: the check rides in the sum-of-squares pass, so
                     the scaler update is the one launch it adds

Each variant is timed eagerly (gradients handed over, ``DDP.step``; device events) and as a
HIP-graph replay of the same step (no host launch gaps). Bytes are computed from the shapes: the
update moves the gradient, master, m, v (read), master, m, v and the parameter (written); the check
and the norm pass each add one read of the gradient. One JSON line per variant; the check pass's
own time is the difference adam_ls - adam of the graph replays, set against its bytes.

usage: python scripts/bench_loss_scale.py [--out profiles/loss_scale_vit_b16.jsonl] [--rounds 5] [--iters 20]
                                          [--only adam]   (one variant: A/B runs against another build)
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


def preset_grads(model, seed, mult):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [((torch.randn(p.shape, device="cuda", generator=g) * 1e-2) * mult).to(p.dtype) for p in model.parameters()]


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
    ap.add_argument("--out", default=os.path.join("profiles", "loss_scale_vit_b16.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default=None, help="time one variant only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_loss_scale.py needs a GPU", file=sys.stderr)
        return 2
    scale = 2.0 ** 16
    engines = {
        "adam": (lambda m: DDP(m, O.Adam(1e-3), average=True, overlap_opt=False), 1.0),
        "adam_ls": (lambda m: DDP(m, O.Adam(1e-3), average=True, loss_scale=scale), scale),
        "global_adam": (lambda m: DDP(m, O.Adam(1e-3), average=True, clip_global_norm=1.0), 1.0),
        "global_adam_ls": (lambda m: DDP(m, O.Adam(1e-3), average=True, clip_global_norm=1.0, loss_scale=scale), scale),
    }
    if a.only is not None:
        engines = {a.only: engines[a.only]}
    fns, info, keep = {}, {}, []
    for name, (make, mult) in engines.items():
        m = model_bf16(0)
        d = make(m)
        grads = preset_grads(m, 1, mult)
        params = list(m.parameters())

        def step(d=d, params=params, grads=grads):
            for p, g in zip(params, grads):  # host-side hand-over (no kernel): the same for every variant
                p.grad = g
            d.step()

        fns[name] = step
        fns[name + "/graph"] = graphed(step)
        keep.append(d)
        n = d.num_parameters()
        leaves = sum(len(b.params) for b in d.buckets)
        upd = sum(b.numel * (2 * b.flat_grad.element_size() + (2 * 4 if b.master is not None else b.flat_grad.element_size())
                             + 4 * b.exp_avg.element_size()) for b in d.buckets)
        read = sum(p.numel() * p.element_size() for b in d.buckets for p in b.params)
        extra = 0 if name == "adam" else read  # one more read of the gradient: the check or the norm pass
        info[name] = info[name + "/graph"] = {"elements": n, "leaves": leaves, "buckets": len(d.buckets),
                                              "bytes_update": upd, "bytes_extra_read": extra}
    for fn in fns.values():  # warm-up of every variant
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for d in keep:
        if getattr(d, "_ls", None) is not None:
            assert int(d.skipped_steps()) == 0, "the timed steps must be applied steps"
    us = {k: [] for k in fns}
    for _ in range(a.rounds):  # alternate the variants: drift of the shared machine hits all alike
        for k, fn in fns.items():
            us[k].append(timed(fn, a.iters))
    med = {k: statistics.median(v) for k, v in us.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for k, v in us.items():
            r = {"variant": k, "us": round(med[k], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                 "rounds": a.rounds, "iters": a.iters, **info[k]}
            r["TBps"] = round((r["bytes_update"] + r["bytes_extra_read"]) / med[k] / 1e6, 2)
            if k.endswith("/graph"):
                if "adam/graph" in med:
                    r["over_adam_graph_us"] = round(med[k] - med["adam/graph"], 1)
                if k == "adam_ls/graph" and "adam/graph" in med:
                    # the check pass (+ the scaler launch) against one read of the bf16 gradient
                    r["check_TBps"] = round(r["bytes_extra_read"] / max(med[k] - med["adam/graph"], 1e-3) / 1e6, 2)
                if k == "global_adam_ls/graph" and "global_adam/graph" in med:
                    r["over_global_adam_graph_us"] = round(med[k] - med["global_adam/graph"], 1)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
