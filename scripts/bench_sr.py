#!/usr/bin/env python
"""Cost of stochastic rounding in one optimiser step over the ViT-B/16 parameters (bf16, bucketed as the
DDP engine buckets them), Adam and Momentum three ways each, alternated in one process, each a HIP-graph
replay of ``DDP.step`` with the gradients handed over:

  *_master   bf16 parameters, fp32 masters and moments (Adam: 28 B per element)
  *_rn       master_weights=False: bf16 parameters and moments, round to nearest (Adam: 14 B)
  *_sr       the same with stochastic_rounding=0: Philox4x32-10 inside the update kernel, one call per
             8 elements and bf16 store (Adam: three), and the one-thread sr_advance (same bytes)

Bytes are computed from the shapes. The yardsticks of ``*_sr`` are its round-to-nearest twin of the same
run (``sr_over_rn``: the generator's cost) and the bytes-based estimate from the master variant of the
same run (``estimate_us``: the master variant's time scaled by the bytes moved). One JSON line per variant.

usage: python scripts/bench_sr.py [--out profiles/sr_vit_b16.jsonl] [--rounds 7] [--iters 20] [--only adam_sr]
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
    ap.add_argument("--out", default=os.path.join("profiles", "sr_vit_b16.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default=None, help="time one variant only (a kernel trace of its own)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_sr.py needs a GPU", file=sys.stderr)
        return 2
    kw = dict(average=True, overlap_opt=False)
    rules = {"adam": lambda: O.Adam(1e-3), "momentum": lambda: O.Momentum(1e-2, 0.9)}
    layouts = {"master": dict(master_weights=True), "rn": dict(master_weights=False),
               "sr": dict(master_weights=False, stochastic_rounding=0)}
    engines = {f"{r}_{l}": (lambda m, r=r, l=l: DDP(m, rules[r](), **layouts[l], **kw)) for r in rules for l in layouts}
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
        # the captured step reads the preset gradients by address: they must outlive the capture
        keep.append((d, grads))
        states = 2 if name.startswith("adam") else 1
        upd = 0
        for b in d.buckets:
            esz = b.flat_grad.element_size()
            if b.master is not None:  # gradient, parameter written; master and every state read + written
                upd += b.numel * (2 * esz + 2 * 4 + 2 * states * 4)
            else:  # gradient; parameter and every state read + written, in the bucket's dtype
                upd += b.numel * (esz + 2 * esz + 2 * states * b.exp_avg.element_size())
        info[name] = {"elements": d.num_parameters(), "flat_elements": sum(b.numel for b in d.buckets),
                      "buckets": len(d.buckets), "bytes_update": upd,
                      "bytes_per_element": round(upd / sum(b.numel for b in d.buckets), 2)}
    for fn in fns.values():  # warm-up of every variant
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(a.rounds):  # alternate the variants: drift of the shared machine hits all alike
        for k, fn in fns.items():
            us[k].append(timed(fn, a.iters))
    for d, _ in keep:
        assert all(bool(torch.isfinite(b.flat_param.float()).all()) for b in d.buckets), "the timed steps must be real steps"
        if d._sr_seed is not None:
            assert int(d.sr_step()) > 0
    med = {k: statistics.median(v) for k, v in us.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for k, v in us.items():
            r = {"variant": k, "us": round(med[k], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                 "rounds": a.rounds, "iters": a.iters, "mode": "graph", **info[k]}
            r["TBps"] = round(r["bytes_update"] / med[k] / 1e6, 2)
            rule = k.split("_")[0]
            if not k.endswith("_master") and f"{rule}_master" in med:
                # the same bandwidth as the master variant of this run reached, on this variant's bytes
                r["estimate_us"] = round(med[f"{rule}_master"] * r["bytes_update"] / info[f"{rule}_master"]["bytes_update"], 1)
            if k.endswith("_sr") and f"{rule}_rn" in med:
                r["sr_added_us"] = round(med[k] - med[f"{rule}_rn"], 1)
                r["sr_over_rn"] = round(med[k] / med[f"{rule}_rn"], 3)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
