#!/usr/bin/env python
"""One optimiser step of every fused rule over the ViT-B/16 parameters (bf16 parameters, fp32
masters and states, bucketed as the DDP engine buckets them), next to plain fused Adam in the same
process:

  adam, rmsprop, adagrad, lion, adamax, amsgrad, nadam, adabelief, adadelta

Each engine's ``DDP.step`` on preset gradients is captured in a HIP graph and the replays are timed
with device events (no host launch gaps); the variants are alternated over the rounds so that drift
of a shared machine hits all alike. The kernels are bandwidth-bound: per element an update reads
the gradient (2 B), the master (4 B) and its states (4 B each) and writes the master, the states
and the parameter (2 B), i.e. 12 + 8 * states bytes. ``expected_us`` is Adam's time scaled by the
bytes per element. One JSON line per rule.

usage: python scripts/bench_rules.py [--out profiles/rules_vit_b16.jsonl] [--rounds 5] [--iters 20] [--rules adam,lion,...]
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

RULES = {
    "adam": lambda: O.Adam(1e-3),
    "rmsprop": lambda: O.RMSProp(1e-3),
    "adagrad": lambda: O.AdaGrad(1e-2),
    "lion": lambda: O.Lion(1e-4),
    "adamax": lambda: O.AdaMax(1e-3),
    "amsgrad": lambda: O.AMSGrad(1e-3),
    "nadam": lambda: O.NAdam(1e-3),
    "adabelief": lambda: O.AdaBelief(1e-3),
    "adadelta": lambda: O.AdaDelta(),
}


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
    ap.add_argument("--out", default=os.path.join("profiles", "rules_vit_b16.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rules", default=",".join(RULES),
                    help="rules to time, in construction order (adam is always timed; a repeated name gets a "
                         "#n suffix: the same kernel on other buffers shows what buffer placement alone does)")
    a = ap.parse_args()
    names = [n for n in a.rules.split(",") if n]
    if "adam" not in names:
        names.insert(0, "adam")
    if not torch.cuda.is_available():
        print("bench_rules.py needs a GPU", file=sys.stderr)
        return 2
    fns, info, keep = {}, {}, []
    for i, rule in enumerate(names):
        name = rule if rule not in names[:i] else f"{rule}#{names[:i].count(rule) + 1}"
        m = model_bf16(0)
        d = DDP(m, RULES[rule](), average=True, overlap_opt=False)
        set_grads(m, 1)
        fns[name] = graphed(lambda d=d: d.step(zero_grad=False))
        keep.append(d)
        states = sum(t is not None for t in (d.buckets[0].exp_avg, d.buckets[0].exp_avg_sq, d.buckets[0].state3))
        per = 2 * d.buckets[0].flat_grad.element_size() + 2 * 4 + 2 * 4 * states
        info[name] = {"elements": d.num_parameters(), "buckets": len(d.buckets), "states": states,
                      "bytes_per_element": per, "bytes": sum(b.numel for b in d.buckets) * per}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            us[k].append(timed(fn, a.iters))
    base = statistics.median(us["adam"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for k, v in us.items():
            med = statistics.median(v)
            r = {"rule": k, "us": round(med, 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                 "rounds": a.rounds, "iters": a.iters, **info[k]}
            r["TBps"] = round(r["bytes"] / med / 1e6, 2)
            r["expected_us"] = round(base * r["bytes_per_element"] / info["adam"]["bytes_per_element"], 1)
            r["vs_expected_pct"] = round(100.0 * (med - r["expected_us"]) / r["expected_us"], 1)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
