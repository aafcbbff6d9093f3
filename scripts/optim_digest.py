#!/usr/bin/env python
"""Bit-for-bit fingerprint of the fused optimiser kernels (optim.hip, optim_rules.hip,
optim_layerwise.hip): one line ``case sha256`` over the raw bytes of every tensor a case writes
(parameters, masters, states, sums, scales, ratios, the clip slot). The kernels use no atomics and
reduce in fixed orders, so two builds that compute the same thing print the same file; a refactor
that lets the compiler contract an expression differently does not. Compare with
``profiles/optim_walker_digests.txt`` (same GPU model, seeded inputs; a few seconds).

Every update case runs one call over these leaves: 0, 1, 7, 8, 9, 4095, 4096, 4097 and 2*4096+5
elements (chunk and vector edges), 4097 elements at storage offset 1 (every tensor misaligned),
a leaf whose gradient alone is misaligned, and sixteen 33-element leaves (27 leaves: a second launch).

usage: python scripts/optim_digest.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluxmpi_amd.ops import optim  # noqa: E402

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
COMBOS = [(F32, F32, F32, False), (F32, BF16, F32, False), (BF16, BF16, BF16, False), (BF16, BF16, F32, False),
          (BF16, BF16, F32, True), (BF16, F32, F32, True), (F16, F16, F16, False), (F16, F16, F32, False),
          (F16, F16, F32, True), (F16, F32, F32, True), (F64, F64, F64, False)]
SHORT = {F32: "f32", BF16: "bf16", F16: "f16", F64: "f64"}
# (elements, parameter/state/master at storage offset 1, gradient at storage offset 1)
LEAVES = [(n, False, False) for n in (0, 1, 7, 8, 9, 4095, 4096, 4097, 2 * 4096 + 5)] + \
         [(4097, True, True), (4097, False, True)] + [(33, False, False)] * 16
DEV = torch.device("cuda")


def values(role: str) -> list:
    """fp64 CPU values of one role of every leaf, the same in every case (states are >= 0: roots)."""
    g = torch.Generator().manual_seed({"p": 1, "g": 2, "s0": 3, "s1": 4, "s2": 5}[role])
    out = []
    for n, _, _ in LEAVES:
        v = torch.randn(n, generator=g, dtype=F64)
        out.append(v * 1e-2 if role == "g" else (v.abs() * 1e-3 if role.startswith("s") else v))
    return out


VALUES = {r: values(r) for r in ("p", "g", "s0", "s1", "s2")}


def leaves(role: str, dtype, grad: bool = False) -> list:
    out = []
    for v, (n, off_all, off_grad) in zip(VALUES[role], LEAVES):
        off = 1 if (off_grad if grad else off_all) else 0
        t = torch.empty(n + off, dtype=dtype, device=DEV)[off:]
        t.copy_(v)
        out.append(t)
    return out


def setup(pd, gd, sd, master, ns):
    p = leaves("p", pd)
    w = None
    if master:  # the master holds what the parameter was rounded from
        w = leaves("p", F32)
    return p, leaves("g", gd, grad=True), [leaves(f"s{k}", sd) for k in range(ns)], w


def digest(tensors) -> str:
    h = hashlib.sha256()
    torch.cuda.synchronize()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def combo_name(pd, gd, sd, master):
    return f"{SHORT[pd]}-{SHORT[gd]}-{SHORT[sd]}-{'master' if master else 'nomaster'}"


def acc(pd):
    return F64 if pd == F64 else F32


def clip_args(pd):
    """tscale, clip_delta and dev_gscale, all active."""
    g = torch.Generator().manual_seed(9)
    return {"tscale": (0.5 + torch.rand(len(LEAVES), generator=g, dtype=F64)).to(acc(pd)).to(DEV),
            "clip_delta": 5e-3, "dev_gscale": torch.tensor([0.75], device=DEV)}


BT1, BT2 = 0.9 ** 3, 0.999 ** 3
RULE_HYPER = {"lr": 1e-3, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "bt1": BT1, "bt2": BT2, "weight_decay": 0.01,
              "grad_scale": 0.5}


def cases():
    for combo in COMBOS:
        for wd in (0.0, 0.01):
            for dev in (False, True):
                p, g, (m, v), w = setup(*combo, 2)
                hyper = torch.tensor([1e-3, BT1, BT2], device=DEV) if dev else None
                optim.adam_(p, g, m, v, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, bc1=1 - BT1, bc2=1 - BT2,
                            weight_decay=wd, grad_scale=0.5, masters=w, dev_hyper=hyper)
                yield f"adam/{combo_name(*combo)}/wd{wd}/{'dev' if dev else 'host'}", p + m + v + (w or [])
    for combo in COMBOS:
        for mode, (mom, nest) in {"descent": (0.0, False), "momentum": (0.9, False), "nesterov": (0.9, True)}.items():
            if mom == 0.0 and combo[3]:
                continue  # without momentum the state counts as the parameter's dtype: no such combination
            p, g, (b,), w = setup(*combo, 1)
            optim.sgd_(p, g, b, lr=0.1, momentum=mom, nesterov=nest, weight_decay=0.01, grad_scale=0.5, masters=w)
            yield f"sgd/{mode}/{combo_name(*combo)}", p + b + (w or [])
    for kind, (_, ns, _) in optim.RULES.items():
        for combo in COMBOS:
            p, g, st, w = setup(*combo, ns)
            optim.rule_(kind, p, g, st, masters=w, **RULE_HYPER)
            yield f"{kind}/{combo_name(*combo)}", p + sum(st, []) + (w or [])
    for fold in ("prologue", "launch"):
        os.environ["FLUXMPI_LAYERWISE_FOLD"] = fold  # read at every call
        for combo in COMBOS:
            p, g, (b,), w = setup(*combo, 1)
            r = torch.zeros(len(p), dtype=acc(combo[0]), device=DEV)
            optim.lars_(p, g, b, lr=0.1, momentum=0.9, trust=1e-3, weight_decay=1e-4, eps=1e-9, grad_scale=0.5,
                        masters=w, ratios=r)
            yield f"lars/{fold}/{combo_name(*combo)}", p + b + (w or []) + [r]
            p, g, (m, v), w = setup(*combo, 2)
            r = torch.zeros(len(p), dtype=acc(combo[0]), device=DEV)
            optim.lamb_(p, g, m, v, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-6, bt1=BT1, bt2=BT2, weight_decay=0.01,
                        grad_scale=0.5, masters=w, ratios=r)
            yield f"lamb/{fold}/{combo_name(*combo)}", p + m + v + (w or []) + [r]
    del os.environ["FLUXMPI_LAYERWISE_FOLD"]
    for gd in (F32, BF16, F16, F64):
        g = leaves("g", gd, grad=True)
        sums, scales = (torch.zeros(len(g), dtype=acc(gd), device=DEV) for _ in range(2))
        optim.sumsq_(g, sums, scales=scales, omega=0.5, grad_scale=0.5)
        yield f"sumsq/{SHORT[gd]}", [sums, scales]
        for accumulate in (False, True):
            slot = torch.tensor([0.25, 0.0, 0.0], device=DEV)
            optim.clip_total_(sums, slot, accumulate=accumulate, omega=0.5, grad_scale=0.5)
            yield f"clip_total/{SHORT[gd]}/{'accumulate' if accumulate else 'fresh'}", [slot]
    combo = (BF16, BF16, F32, True)
    p, g, (m, v), w = setup(*combo, 2)
    optim.adam_(p, g, m, v, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, bc1=1 - BT1, bc2=1 - BT2, weight_decay=0.01,
                grad_scale=0.5, masters=w, **clip_args(BF16))
    yield f"adam/{combo_name(*combo)}/clip", p + m + v + w
    p, g, st, w = setup(*combo, 2)
    optim.rule_("nadam", p, g, st, masters=w, **RULE_HYPER, **clip_args(BF16))
    yield f"nadam/{combo_name(*combo)}/clip", p + sum(st, []) + w
    combo = (F64, F64, F64, False)
    p, g, (b,), w = setup(*combo, 1)
    optim.sgd_(p, g, b, lr=0.1, momentum=0.9, nesterov=True, weight_decay=0.01, grad_scale=0.5, **clip_args(F64))
    yield f"sgd/nesterov/{combo_name(*combo)}/clip", p + b


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("optim_digest.py needs a GPU", file=sys.stderr)
        return 2
    lines = [f"{name} {digest(tensors)}" for name, tensors in cases()]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
