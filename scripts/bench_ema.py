#!/usr/bin/env python
"""Cost of the weight EMA in one optimiser step over the ViT-B/16 parameters (bf16 parameters, fp32
masters and moments, bucketed as the DDP engine buckets them), four variants alternated in one
process, each a HIP-graph replay of ``DDP.step`` with the gradients handed over:

  adam               fused Adam (one launch per bucket)
  adam_ema           DDP(Adam, ema=0.9999): one mt_ema launch behind each bucket's update (reads the
                     fp32 master the update just wrote and the average, writes the average: 12 B per
                     element) and the one-thread ema_advance
  adam_ema_every4    the same with EMA(every=4): three steps of four the mt_ema launches return on the
                     block's hold word before they load tensor data
  momentum_ema       DDP(Momentum, ema=0.9999)

Bytes are computed from the shapes: Adam moves the gradient, master, m, v (read) and master, m, v and
the parameter (written): 28 B per element behind bf16 parameters with fp32 masters. The EMA's added
time (adam_ema - adam) is set against its bytes-based estimate, 12/28 of the same run's plain Adam
time: below it when the master read is served from the Infinity Cache. One JSON line per variant.

usage: python scripts/bench_ema.py [--out profiles/ema_vit_b16.jsonl] [--rounds 7] [--iters 20] [--only adam_ema]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluxmpi_amd import EMA, optimisers as O  # noqa: E402
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


def preset_grads(model, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [(torch.randn(p.shape, device="cuda", generator=g) * 1e-2).to(p.dtype) for p in model.parameters()]


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
    ap.add_argument("--out", default=os.path.join("profiles", "ema_vit_b16.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default=None, help="time one variant only (a kernel trace of its own)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_ema.py needs a GPU", file=sys.stderr)
        return 2
    kw = dict(average=True, overlap_opt=False)
    engines = {
        "adam": lambda m: DDP(m, O.Adam(1e-3), **kw),
        "adam_ema": lambda m: DDP(m, O.Adam(1e-3), ema=0.9999, **kw),
        "adam_ema_every4": lambda m: DDP(m, O.Adam(1e-3), ema=EMA(decay=0.9996, every=4), **kw),
        "momentum_ema": lambda m: DDP(m, O.Momentum(1e-2, 0.9), ema=0.9999, **kw),
    }
    if a.only is not None:
        engines = {a.only: engines[a.only]}
    fns, info, keep = {}, {}, []
    for name, make in engines.items():
        m = model_bf16(0)
        d = make(m)
        grads = preset_grads(m, 1)
        params = list(m.parameters())

        def step(d=d, params=params, grads=grads):
            for p, g in zip(params, grads):  # host-side hand-over (no kernel): the same for every variant
                p.grad = g
            d.step()

        fns[name] = graphed(step)
        # the captured step reads the preset gradients by address: they must outlive the capture (the
        # next capture empties the allocator's cache, which would unmap them)
        keep.append((d, grads))
        flat = sum(b.numel for b in d.buckets)
        states = 2 if name.startswith("adam") else 1
        # gradient + parameter (bf16), master read + written, every state read + written
        upd = sum(b.numel * (2 * b.flat_grad.element_size() + 2 * 4 + 2 * states * 4) for b in d.buckets)
        # per step: an EMA(every=k) engine moves the average's bytes on one step of k
        ema = sum(b.numel * 3 * b.ema.element_size() for b in d.buckets) // d._ema.every if d._ema is not None else 0
        info[name] = {"elements": d.num_parameters(), "flat_elements": flat, "buckets": len(d.buckets),
                      "launches_ema": len(d.buckets) + 1 if ema else 0, "bytes_update": upd, "bytes_ema": ema}
    for fn in fns.values():  # warm-up of every variant
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(a.rounds):  # alternate the variants: drift of the shared machine hits all alike
        for k, fn in fns.items():
            us[k].append(timed(fn, a.iters))
    for d, _ in keep:
        assert all(bool(torch.isfinite(b.master).all()) for b in d.buckets), "the timed steps must be real steps"
        if d.buckets[0].ema is not None:
            assert int(d.ema_updates()) > 0 and all(bool(torch.isfinite(b.ema).all()) for b in d.buckets)
    med = {k: statistics.median(v) for k, v in us.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for k, v in us.items():
            r = {"variant": k, "us": round(med[k], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                 "rounds": a.rounds, "iters": a.iters, "mode": "graph", **info[k]}
            r["TBps"] = round((r["bytes_update"] + r["bytes_ema"]) / med[k] / 1e6, 2)
            if k != "adam" and "adam" in med and k.startswith("adam"):
                added = med[k] - med["adam"]
                r["ema_added_us"] = round(added, 1)
                # 12 B per element on top of Adam's 28, at the bandwidth plain Adam reached in this run
                r["ema_estimate_us"] = round(med["adam"] * r["bytes_ema"] / info["adam"]["bytes_update"], 1)
                r["ema_TBps"] = round(r["bytes_ema"] / max(added, 1e-3) / 1e6, 2)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
