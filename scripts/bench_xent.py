#!/usr/bin/env python
"""The fused softmax cross-entropy (``ops.xent.softmax_cross_entropy``: forward, finish and backward
kernels) against the PyTorch composition it replaces, forward + backward of the loss alone.

Sizes: ``[256, 1000]`` bf16 (a ResNet-50 head at batch 256: bound by launches) and ``[50432, 1000]`` bf16
(large enough to be bound by bandwidth). Variants, alternated in one process, each a HIP-graph replay:

  hard        fused, integer labels            / torch_hard        F.cross_entropy(x.float(), y)
  hard_eps    fused, label_smoothing=0.1       / torch_hard_eps    the same call with label_smoothing=0.1
  mixed       fused, two labels and lam        / torch_mixed       mix_targets + F.cross_entropy(x.float(), soft)
  dense       fused, prebuilt fp32 targets     / torch_dense       F.cross_entropy(x.float(), soft), soft prebuilt

Each step computes the loss and the gradient of the bf16 logits. Bytes of the fused route: the logits
read twice and written once, plus the dense targets read twice where there are any. ``launches``: the
device kernels of one eager step, counted with the PyTorch profiler (``null`` where it is unavailable).
One JSON line per variant and size; ``faster_than_torch_worst_case`` compares the fused variant's slowest
round with the composition's fastest.

usage: python scripts/bench_xent.py [--out profiles/xent_resnet50.jsonl] [--rounds 7] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluxmpi_amd.ops.augment import mix_targets  # noqa: E402
from fluxmpi_amd.ops.xent import softmax_cross_entropy  # noqa: E402

EPS, LAM = 0.1, 0.3


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


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
        out = step()
    return gr.replay, out


def launches(step):
    """Device kernels of one eager step."""
    try:
        from torch.profiler import ProfilerActivity, profile
        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return n or None
    except Exception:
        return None


def variants(B, C):
    x = torch.randn(B, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)).bfloat16()
    x.requires_grad_()
    y = torch.randint(0, C, (B,), device="cuda")
    soft = mix_targets(y, C, LAM, EPS)

    def fb(loss_fn):
        def step():
            x.grad = None
            loss = loss_fn()
            loss.backward()
            return loss.detach(), x.grad
        return step

    return {
        "hard": fb(lambda: softmax_cross_entropy(x, y)),
        "torch_hard": fb(lambda: F.cross_entropy(x.float(), y)),
        "hard_eps": fb(lambda: softmax_cross_entropy(x, y, label_smoothing=EPS)),
        "torch_hard_eps": fb(lambda: F.cross_entropy(x.float(), y, label_smoothing=EPS)),
        "mixed": fb(lambda: softmax_cross_entropy(x, y, lam=LAM, label_smoothing=EPS)),
        "torch_mixed": fb(lambda: F.cross_entropy(x.float(), mix_targets(y, C, LAM, EPS))),
        "dense": fb(lambda: softmax_cross_entropy(x, soft)),
        "torch_dense": fb(lambda: F.cross_entropy(x.float(), soft)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "xent_resnet50.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", default="256x1000,50432x1000")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_xent.py needs a GPU", file=sys.stderr)
        return 2
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for size in a.sizes.split(","):
            B, C = (int(v) for v in size.split("x"))
            steps = variants(B, C)
            count = {k: launches(s) for k, s in steps.items()}
            fns, outs = {}, {}
            for k, s in steps.items():
                fns[k], outs[k] = graphed(s)
            for fn in fns.values():
                for _ in range(4):
                    fn()
            torch.cuda.synchronize()
            for k in ("hard", "hard_eps", "mixed", "dense"):  # the two routes compute one loss and one gradient
                dl = abs(float(outs[k][0]) - float(outs["torch_" + k][0]))
                dg = float((outs[k][1].float() - outs["torch_" + k][1].float()).abs().max())
                assert dl <= 1e-4 * abs(float(outs[k][0])) and dg <= 2.0 ** -7 / B, (k, dl, dg)
            us = {k: [] for k in fns}
            for _ in range(a.rounds):  # alternate the variants: drift of the shared machine hits all alike
                for k, fn in fns.items():
                    us[k].append(timed(fn, a.iters))
            med = {k: statistics.median(v) for k, v in us.items()}
            for k, v in us.items():
                r = {"variant": k, "size": [B, C], "dtype": "bf16", "us": round(med[k], 1), "us_min": round(min(v), 1),
                     "us_max": round(max(v), 1), "rounds": a.rounds, "iters": a.iters, "mode": "graph",
                     "launches": count[k]}
                if not k.startswith("torch_"):
                    r["bytes"] = B * C * 2 * 3 + (B * C * 4 * 2 if k == "dense" else 0)
                    r["TBps"] = round(r["bytes"] / med[k] / 1e6, 3)
                    t = "torch_" + k
                    r["torch_over_fused"] = round(med[t] / med[k], 2)
                    r["faster_than_torch_worst_case"] = bool(max(v) < min(us[t]))
                line = json.dumps(r)
                print(line, flush=True)
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
