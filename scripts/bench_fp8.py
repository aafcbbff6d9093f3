#!/usr/bin/env python
"""The fp8 path (``ops.fp8``: ``csrc/kernels/fp8_quant.hip``, ``gemm_fp8.hip``) against the bf16 kernels it would
replace, at the ViT-B/16 shapes (50432 tokens = batch 256).

Variants, alternated in one process, each a HIP-graph replay:

  gemm_{fwd,dgrad}_{qkv,proj,fc1,fc2}_{fp8,bf16}   the GEMM alone: ``fp8.gemm`` on images made beforehand against
                                                   ``ops.linear.fwd`` / ``dgrad`` (gemm_nt.hip, else hipBLASLt)
  quant_x_{current,delayed}                        the activation's cast passes alone ([50432, 768], e4m3)
  qkv_fwdbwd_{bf16,fp8_current,fp8_delayed,fp8_mx} ``Linear`` / ``Fp8Linear`` forward + backward (dx, dW, db)
  gemm_{fwd,dgrad}_*_fp8_mx, quant_x_mx, quant_w_mx the MX block-scaled counterparts (``mx_gemm.hip``, ``mx_quant.hip``:
                                                   one launch per cast; ``quant_w_mx`` is W [2304, 768], both images)

One JSON line per variant with the median of the rounds and min-max; fp8 lines carry ``bf16_over_fp8`` and the
GEMM lines the achieved PFLOP/s (2 M N K over the median).

``--wgrad`` measures the MX weight gradient (``mx_wgrad.hip``) instead, at qkv's shape, the same way:

  mx_wgrad_s{n}                        ``fp8.mx_wgrad`` (kernel + reduce) at the default split count, half and double it
  wgrad_bf16                           ``ops.linear.weight_grad`` (wgrad256.hip + reduce) on the bf16 operands
  quant_x_mx_t, quant_dy_mx_t          the two casts with their token-blocked images (one launch each)
  qkv_fwdbwd_{bf16,fp8_mx,fp8_mx_wgrad} ``Linear`` / ``Fp8Linear(scaling="mx")`` with ``wgrad="bf16"`` and ``"mx"``
  vit_b16_step_{bf16,mx,mx_wgrad}      ``bench.py --model vit_b16 --force-comm`` as child processes with ``FLUXMPI_FP8``
                                       unset / ``mx`` / ``mx+wgrad``, alternated: img/s and ``pack_copies_per_step``

``--fp4`` measures the fp4 (e2m1) MX path (``mx4_quant.hip``, ``mx4_gemm.hip``) against the e4m3 MX one and bf16:

  quant_{x,w}_{mx4,mx}                 the cast of x [tokens, 768] (row-wise image) and of W [2304, 768] (both images)
  gemm_fwd_{layer}_{mx4,mx,bf16}       the forward GEMM alone: e2m1 x e2m1, e4m3 x e4m3, ``ops.linear.fwd``
  gemm_dgrad_{layer}_{mx4,mx,bf16}     the input-gradient GEMM alone: e4m3 dy x e2m1 W^T, e4m3 x e4m3, ``ops.linear.dgrad``
  qkv_fwdbwd_{bf16,fp8_mx,fp8_mx4}     ``Linear`` / ``Fp8Linear(scaling="mx")`` with ``fwd="e4m3"`` and ``"e2m1"``
  vit_b16_step_{bf16,mx,mx4}           ``bench.py`` child processes as under ``--wgrad``, into ``--ab-out``

``--fp6`` is ``--fp4`` with the fp6 MX path (``mx6_quant.hip``, ``mx6_gemm.hip``) beside both, all variants alternated in
one process: ``quant_{x,w}_mx6`` (e2m3) and ``quant_dy_mx6`` (e3m2), ``gemm_fwd_{layer}_mx6`` (e2m3 x e2m3),
``gemm_dgrad_{layer}_mx6`` (e3m2 dy x e2m3 W^T), ``qkv_fwdbwd_fp8_mx6`` and ``vit_b16_step_mx6``; its rows carry
``mx_over_mx6``, ``mx4_over_mx6`` and ``bf16_over_mx6``.

usage: python scripts/bench_fp8.py [--out profiles/fp8_vit_b16.jsonl] [--rounds 7] [--iters 20] [--tokens 50432]
       python scripts/bench_fp8.py --wgrad [--out profiles/mx_wgrad_vit_b16.jsonl] [--vit-steps 20] [--vit-rounds 2]
       python scripts/bench_fp8.py --fp4 [--out profiles/mx4_vit_b16.jsonl] [--ab-out profiles/mx4_bench_ab.jsonl]
       python scripts/bench_fp8.py --fp6 [--out profiles/mx6_vit_b16.jsonl] [--ab-out profiles/mx6_bench_ab.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluxmpi_amd.ops import fp8  # noqa: E402
from fluxmpi_amd.ops import linear as L  # noqa: E402
from scripts.bench_patch_embed import graphed, timed  # noqa: E402

LAYERS = {"qkv": (768, 2304), "proj": (768, 768), "fc1": (768, 3072), "fc2": (3072, 768)}  # name -> (n_in, n_out)


def measure(fns, a):
    """Median and min-max of ``a.rounds`` rounds of ``a.iters`` replays, the variants alternated."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            us[k].append(timed(fn, a.iters))
    return us


def vit_steps(a, keys=("bf16", "mx", "mx_wgrad")):
    """``bench.py --model vit_b16`` per ``FLUXMPI_FP8`` value in child processes, alternated ``a.vit_rounds`` times."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = {k: [] for k in keys}
    for _ in range(a.vit_rounds):
        for key in runs:
            env = dict(os.environ)
            env.pop("FLUXMPI_FP8", None)
            if key != "bf16":
                env["FLUXMPI_FP8"] = key.replace("_", "+")
            r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--model", "vit_b16", "--gpus", "1", "--steps",
                                str(a.vit_steps), "--warmup", "5", "--force-comm"], env=env, capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"bench.py failed for {key}:\n{r.stderr[-2000:]}")
            runs[key].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    return runs


def main_wgrad(a):
    M = a.tokens
    n_in, n_out = LAYERS["qkv"]
    torch.manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda").bfloat16()
    x, dy = rnd(M, n_in).requires_grad_(), rnd(M, n_out)
    xd = x.detach()
    xm, dym = fp8.mx_quantize(xd, fp8.E4M3, transpose=True), fp8.mx_quantize(dy, fp8.E4M3, transpose=True)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    s0 = fp8.mx_wgrad_splits(n_out, n_in, M, cus)
    fns, keep, flops = {}, [xm, dym], {}
    with torch.no_grad():
        for sp in sorted({max(1, s0 // 2), s0, 2 * s0}):
            fns[f"mx_wgrad_s{sp}"], out = graphed(lambda sp=sp: fp8.mx_wgrad(dym.t(), xm.t(), torch.bfloat16, splits=sp))
            keep.append(out)
        fns["wgrad_bf16"], out = graphed(lambda: L.weight_grad(dy, xd, torch.bfloat16))
        keep.append(out)
        for key, t in (("quant_x_mx_t", xd), ("quant_dy_mx_t", dy)):
            fns[key], out = graphed(lambda t=t: fp8.mx_quantize(t, fp8.E4M3, transpose=True))
            keep.append(out)
    for k in fns:
        if "wgrad" in k:
            flops[k] = 2.0 * M * n_in * n_out
    for key, lin in (("bf16", L.Linear(n_in, n_out)), ("fp8_mx", fp8.Fp8Linear(n_in, n_out, scaling="mx")),
                     ("fp8_mx_wgrad", fp8.Fp8Linear(n_in, n_out, scaling="mx", wgrad="mx"))):
        lin = lin.cuda().bfloat16()

        def fwdbwd(lin=lin):
            lin.weight.grad = lin.bias.grad = x.grad = None
            lin(x).backward(dy)
            return x.grad, lin.weight.grad, lin.bias.grad

        fns[f"qkv_fwdbwd_{key}"], out = graphed(fwdbwd)
        keep += [lin, fwdbwd, out]
    us = measure(fns, a)
    med = {k: statistics.median(v) for k, v in us.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(r):
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")

        for k, v in us.items():
            r = {"variant": k, "us": round(med[k], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                 "rounds": a.rounds, "iters": a.iters, "mode": "graph", "tokens": M}
            if k in flops:
                r["pflops"] = round(flops[k] / med[k] * 1e-9, 3)
            if k.startswith("mx_wgrad_s"):
                r["splits"], r["default_splits"], r["bf16_over_fp8"] = int(k[10:]), s0, round(med["wgrad_bf16"] / med[k], 2)
            if k.startswith("qkv_fwdbwd_fp8"):
                r["bf16_over_fp8"] = round(med["qkv_fwdbwd_bf16"] / med[k], 2)
            emit(r)
        del fns, keep
        torch.cuda.empty_cache()
        if a.vit_rounds > 0:
            for key, rs in vit_steps(a).items():
                emit({"variant": f"vit_b16_step_{key}", "value": [r.get("value") for r in rs], "unit": rs[0].get("unit"),
                      "pack_copies_per_step": [r.get("config", {}).get("pack_copies_per_step") for r in rs], "steps": a.vit_steps})
    return 0


def main_fp4(a, fp6=False):
    M = a.tokens
    six = (("mx6", fp8.E2M3),) if fp6 else ()
    torch.manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda").bfloat16()
    fns, keep, flops = {}, [], {}
    with torch.no_grad():
        for name, (n_in, n_out) in LAYERS.items():
            x, w, dy = rnd(M, n_in), rnd(n_out, n_in) * n_in ** -0.5, rnd(M, n_out)
            dy8 = fp8.mx_quantize(dy, fp8.E4M3)
            for key, fmt in six + (("mx4", fp8.E2M1), ("mx", fp8.E4M3)):
                xq, wq = fp8.mx_quantize(x, fmt), fp8.mx_quantize(w, fmt, transpose=True)
                dyq = fp8.mx_quantize(dy, fp8.E3M2) if key == "mx6" else dy8
                fns[f"gemm_fwd_{name}_{key}"], o1 = graphed(lambda xq=xq, wq=wq: fp8.mx_gemm(xq, wq))
                fns[f"gemm_dgrad_{name}_{key}"], o2 = graphed(lambda wq=wq, dyq=dyq: fp8.mx_gemm(dyq, wq.t()))
                keep += [xq, wq, dyq, o1, o2]
                if name == "qkv" and key == "mx6":
                    fns["quant_dy_mx6"], o1 = graphed(lambda dy=dy: fp8.mx_quantize(dy, fp8.E3M2))
                    keep.append(o1)
                if name == "qkv":
                    fns[f"quant_x_{key}"], o1 = graphed(lambda x=x, fmt=fmt: fp8.mx_quantize(x, fmt))
                    fns[f"quant_w_{key}"], o2 = graphed(lambda w=w, fmt=fmt: fp8.mx_quantize(w, fmt, transpose=True))
                    keep += [o1, o2]
            fns[f"gemm_fwd_{name}_bf16"], o1 = graphed(lambda x=x, w=w: L.fwd(x, w, None))
            fns[f"gemm_dgrad_{name}_bf16"], o2 = graphed(lambda dy=dy, w=w: L.dgrad(dy, w))
            keep += [x, w, dy, dy8, o1, o2]
            for k in fns:
                if k.startswith(("gemm_fwd_" + name, "gemm_dgrad_" + name)):
                    flops[k] = 2.0 * M * n_in * n_out
    n_in, n_out = LAYERS["qkv"]
    x, dy = rnd(M, n_in).requires_grad_(), rnd(M, n_out)
    for key, lin in (("bf16", L.Linear(n_in, n_out)), ("fp8_mx", fp8.Fp8Linear(n_in, n_out, scaling="mx")),
                     ("fp8_mx4", fp8.Fp8Linear(n_in, n_out, scaling="mx", fwd="e2m1"))) + (
                         (("fp8_mx6", fp8.Fp8Linear(n_in, n_out, scaling="mx", fwd="e2m3")),) if fp6 else ()):
        lin = lin.cuda().bfloat16()

        def fwdbwd(lin=lin):
            lin.weight.grad = lin.bias.grad = x.grad = None
            lin(x).backward(dy)
            return x.grad, lin.weight.grad, lin.bias.grad

        fns[f"qkv_fwdbwd_{key}"], out = graphed(fwdbwd)
        keep += [lin, fwdbwd, out]
    us = measure(fns, a)
    med = {k: statistics.median(v) for k, v in us.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for k, v in us.items():
            r = {"variant": k, "us": round(med[k], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                 "rounds": a.rounds, "iters": a.iters, "mode": "graph", "tokens": M}
            if k in flops:
                r["pflops"] = round(flops[k] / med[k] * 1e-9, 3)
            if k.endswith("_mx6") and k != "quant_dy_mx6":
                r["mx_over_mx6"], r["mx4_over_mx6"] = round(med[k[:-1]] / med[k], 2), round(med[k[:-1] + "4"] / med[k], 2)
                other = k[:-3] + "bf16" if k.startswith("gemm") else "qkv_fwdbwd_bf16" if k.startswith("qkv") else None
                if other:
                    r["bf16_over_mx6"] = round(med[other] / med[k], 2)
            if k.endswith("_mx4"):
                r["mx_over_mx4"] = round(med[k[:-1]] / med[k], 2)
                other = k[:-3] + "bf16" if k.startswith("gemm") else "qkv_fwdbwd_bf16" if k.startswith("qkv") else None
                if other:
                    r["bf16_over_mx4"] = round(med[other] / med[k], 2)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    del fns, keep
    torch.cuda.empty_cache()
    if a.vit_rounds > 0:
        os.makedirs(os.path.dirname(os.path.abspath(a.ab_out)), exist_ok=True)
        with open(a.ab_out, "w") as f:
            for key, rs in vit_steps(a, ("bf16", "mx", "mx4") + (("mx6",) if fp6 else ())).items():
                line = json.dumps({"variant": f"vit_b16_step_{key}", "value": [r.get("value") for r in rs],
                                   "unit": rs[0].get("unit"), "steps": a.vit_steps})
                print(line, flush=True)
                f.write(line + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fp4", action="store_true", help="the fp4 (e2m1) MX rows (module docstring)")
    ap.add_argument("--fp6", action="store_true", help="the fp4 rows with the fp6 (e2m3 / e3m2) MX rows beside them")
    ap.add_argument("--ab-out", default=None)
    ap.add_argument("--wgrad", action="store_true", help="the MX weight-gradient rows (module docstring)")
    ap.add_argument("--vit-steps", type=int, default=20)
    ap.add_argument("--vit-rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tokens", type=int, default=50432)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_fp8.py needs a GPU", file=sys.stderr)
        return 2
    a.ab_out = a.ab_out or os.path.join("profiles", "mx6_bench_ab.jsonl" if a.fp6 else "mx4_bench_ab.jsonl")
    a.out = a.out or os.path.join("profiles", "mx6_vit_b16.jsonl" if a.fp6 else "mx4_vit_b16.jsonl" if a.fp4 else
                                  "mx_wgrad_vit_b16.jsonl" if a.wgrad else "fp8_vit_b16.jsonl")
    if a.fp4 or a.fp6:
        return main_fp4(a, a.fp6)
    if a.wgrad:
        return main_wgrad(a)
    M = a.tokens
    torch.manual_seed(0)
    fns, flops, keep = {}, {}, []
    rnd = lambda *s: torch.randn(*s, device="cuda").bfloat16()
    for name, (n_in, n_out) in LAYERS.items():
        x, w, b, dy = rnd(M, n_in), rnd(n_out, n_in) * n_in ** -0.5, rnd(n_out), rnd(M, n_out)
        xq, wq, dyq = fp8.quantize(x, fp8.E4M3), fp8.quantize(w, fp8.E4M3, transpose=True), fp8.quantize(dy, fp8.E5M2)
        xm, wm, dym = fp8.mx_quantize(x, fp8.E4M3), fp8.mx_quantize(w, fp8.E4M3, transpose=True), fp8.mx_quantize(dy, fp8.E4M3)
        keep += [x, w, b, dy, xq, wq, dyq, xm, wm, dym]
        with torch.no_grad():
            for key, f in ((f"gemm_fwd_{name}_fp8", lambda xq=xq, wq=wq, b=b: fp8.gemm(xq, wq, b)),
                           (f"gemm_fwd_{name}_bf16", lambda x=x, w=w, b=b: L.fwd(x, w, b)),
                           (f"gemm_dgrad_{name}_fp8", lambda dyq=dyq, wq=wq: fp8.gemm(dyq, wq.t())),
                           (f"gemm_dgrad_{name}_bf16", lambda dy=dy, w=w: L.dgrad(dy, w)),
                           (f"gemm_fwd_{name}_fp8_mx", lambda xm=xm, wm=wm, b=b: fp8.mx_gemm(xm, wm, b)),
                           (f"gemm_dgrad_{name}_fp8_mx", lambda dym=dym, wm=wm: fp8.mx_gemm(dym, wm.t()))):
                fns[key], out = graphed(f)
                flops[key] = 2.0 * M * n_in * n_out
                keep += [f, out]
        print(f"captured gemm {name}", file=sys.stderr, flush=True)
    n_in, n_out = LAYERS["qkv"]
    x, dy = rnd(M, n_in).requires_grad_(), rnd(M, n_out)
    blk = fp8.new_block("cuda")

    def delayed_cast():
        fp8.scale_update(blk, fp8.E4M3)
        return fp8.quantize(x.detach(), fp8.E4M3, blk)

    wqkv = rnd(n_out, n_in) * n_in ** -0.5
    for key, f in (("quant_x_current", lambda: fp8.quantize(x.detach(), fp8.E4M3)), ("quant_x_delayed", delayed_cast),
                   ("quant_x_mx", lambda: fp8.mx_quantize(x.detach(), fp8.E4M3)),
                   ("quant_w_mx", lambda: fp8.mx_quantize(wqkv, fp8.E4M3, transpose=True))):
        fns[key], out = graphed(f)
        keep += [f, out]
    for key, lin in (("bf16", L.Linear(n_in, n_out)), ("fp8_current", fp8.Fp8Linear(n_in, n_out)),
                     ("fp8_delayed", fp8.Fp8Linear(n_in, n_out, scaling="delayed")),
                     ("fp8_mx", fp8.Fp8Linear(n_in, n_out, scaling="mx"))):
        lin = lin.cuda().bfloat16()

        def fwdbwd(lin=lin):
            lin.weight.grad = lin.bias.grad = x.grad = None
            lin(x).backward(dy)
            return x.grad, lin.weight.grad, lin.bias.grad

        fns[f"qkv_fwdbwd_{key}"], out = graphed(fwdbwd)
        keep += [lin, fwdbwd, out]
        print(f"captured qkv {key}", file=sys.stderr, flush=True)
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(a.rounds):  # alternate the variants: drift of the shared machine hits all alike
        for k, fn in fns.items():
            us[k].append(timed(fn, a.iters))
    med = {k: statistics.median(v) for k, v in us.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for k, v in us.items():
            r = {"variant": k, "us": round(med[k], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                 "rounds": a.rounds, "iters": a.iters, "mode": "graph", "tokens": M}
            if k in flops:
                r["pflops"] = round(flops[k] / med[k] * 1e-9, 3)
            base = k.replace("_fp8_mx", "_bf16").replace("_fp8", "_bf16") if k.startswith("gemm_") else "qkv_fwdbwd_bf16"
            if "fp8" in k and base in med:
                r["bf16_over_fp8"] = round(med[base] / med[k], 2)
                r["faster_than_bf16_worst_case"] = bool(max(v) < min(us[base]))
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
