#!/usr/bin/env python
"""Cost of the synchronised (deterministic) BatchNorm over the fused one at world size 1, on ResNet-50's nine
BatchNorm shapes at batch 256 in bf16 (NHWC): 112x112x64, 56x56x64, 56x56x256, 28x28x128, 28x28x512, 14x14x256,
14x14x1024, 7x7x512, 7x7x2048.

Two variants alternated in one process on one device:

  fused   ``FusedBatchNorm2d``: float atomics into 16 shards, finalize, apply | reduce, finalize, dx
  sync    ``SyncBatchNorm2d`` without a process group: per-workgroup partials, fold + finalize in one launch,
          apply | reduce, fold, dx (no collective at world size 1)

Each is a forward (+ReLU) and backward of one layer, timed as a HIP-graph replay (no host launch gaps), device
events around ``iters`` replays, ``rounds`` rounds, the variants alternated so that drift of a shared machine hits
both alike. Bytes are computed from the shapes: the fold reads the forward and the backward partials once each
(2 x blocks x 2 C fp32; the reductions wrote the same bytes), against the 5 activation reads and 2 writes of the
layer. One JSON line per shape. The cost at more than one rank (two small collectives per layer per step behind
the bucket allreduces on the in-order communication stream) is NOT measured here.

usage: python scripts/bench_syncbn.py [--out profiles/syncbn_resnet50.jsonl] [--batch 256] [--rounds 5] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluxmpi_amd.ops import _ext  # noqa: E402
from fluxmpi_amd.ops.batchnorm import FusedBatchNorm2d  # noqa: E402
from fluxmpi_amd.ops.syncbn import SyncBatchNorm2d  # noqa: E402

SHAPES = [(112, 64), (56, 64), (56, 256), (28, 128), (28, 512), (14, 256), (14, 1024), (7, 512), (7, 2048)]


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
        step()
    return gr.replay


def layer(cls, batch, hw, ch, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    bn = cls(ch).cuda()
    shape = (batch, hw, hw, ch)
    x = torch.randn(shape, device="cuda", generator=g).to(torch.bfloat16).permute(0, 3, 1, 2).requires_grad_()
    dy = torch.randn(shape, device="cuda", generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)

    def step():
        x.grad = bn.weight.grad = bn.bias.grad = None
        bn(x, relu=True).backward(dy)

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "syncbn_resnet50.jsonl"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_syncbn.py needs a GPU", file=sys.stderr)
        return 2
    ext = _ext.get(required=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for hw, ch in SHAPES:
            fns = {"fused": graphed(layer(FusedBatchNorm2d, a.batch, hw, ch, 1)),
                   "sync": graphed(layer(SyncBatchNorm2d, a.batch, hw, ch, 1))}
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            us = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    us[k].append(timed(fn, a.iters))
            rows = a.batch * hw * hw
            part = ext.bn_sync_workspace_floats(rows, ch) * 4
            act = rows * ch * 2
            med = {k: statistics.median(v) for k, v in us.items()}
            r = {"shape": f"{hw}x{hw}x{ch}", "rows": rows, "C": ch, "batch": a.batch, "dtype": "bf16",
                 "fused_us": round(med["fused"], 1), "sync_us": round(med["sync"], 1),
                 "ratio": round(med["sync"] / med["fused"], 3),
                 "fused_us_min_max": [round(min(us["fused"]), 1), round(max(us["fused"]), 1)],
                 "sync_us_min_max": [round(min(us["sync"]), 1), round(max(us["sync"]), 1)],
                 "partials": part // (8 * ch), "fold_read_bytes": 2 * part, "activation_bytes": 7 * act,
                 "partial_traffic_pct": round(100.0 * 4 * part / (7 * act), 2),
                 "fused_TBps": round(7 * act / med["fused"] / 1e6, 2), "rounds": a.rounds, "iters": a.iters}
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
            del fns
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
