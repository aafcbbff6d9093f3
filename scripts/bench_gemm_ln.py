#!/usr/bin/env python
"""The Linear + residual add + LayerNorm forward as one launch (``csrc/kernels/gemm_ln.hip``) against today's
composition (``ops.linear.fwd`` + ``layernorm_fwd`` with the residual add), at the ViT shapes:

  proj      M = 50432, N = 768, K = 768          fc2      M = 50432, N = 768, K = 3072
  s_proj    M = 50432, N = 384, K = 384          s_fc2    M = 50432, N = 384, K = 1536

The two variants of a shape are alternated in one process; each timing is a pair of device events around enough
launches to fill ``--ms`` milliseconds; medians with min - max over ``--rounds`` rounds. One JSON line per variant.

usage: python scripts/bench_gemm_ln.py [--out profiles/gemm_ln_vit_b16.jsonl] [--rounds 7] [--ms 150]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluxmpi_amd.ops import layernorm as LN  # noqa: E402
from fluxmpi_amd.ops import linear  # noqa: E402

SHAPES = {"proj": (50432, 768, 768), "fc2": (50432, 768, 3072), "s_proj": (50432, 384, 384),
          "s_fc2": (50432, 384, 1536)}


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "gemm_ln_vit_b16.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ms", type=float, default=150.0, help="device time one timing should fill")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_gemm_ln.py needs a GPU", file=sys.stderr)
        return 2
    torch.manual_seed(0)
    rows = []
    for name, (M, N, K) in SHAPES.items():
        mk = lambda *s, scale=1.0: (torch.randn(*s, device="cuda") * scale).bfloat16()
        act, W, bias, x = mk(M, K, scale=0.5), mk(N, K, scale=K ** -0.5), mk(N, scale=0.1), mk(M, N)
        lw, lb = (torch.rand(N, device="cuda") + 0.5).bfloat16(), mk(N, scale=0.1)
        assert LN._fused_fwd_ok(act, W, bias, x, lw, lb)
        fns = {"fused": lambda: LN._fused_fwd(act, W, bias, x, lw, lb, 1e-6),
               "composition": lambda: LN._fwd(x, linear.fwd(act, W, bias), lw, lb, 1e-6)}
        hf, yf = fns["fused"]()[:2]
        hc, yc = fns["composition"]()[:2]
        for got, ref in ((hf, hc), (yf, yc)):  # one rounding against two: a bf16 ulp or so apart
            assert float((got.float() - ref.float()).norm() / ref.float().norm()) < 1e-2
        iters = {k: max(3, int(a.ms * 1e3 / timed(f, 5))) for k, f in fns.items()}
        us = {k: [] for k in fns}
        for _ in range(a.rounds):  # alternate the variants: drift of the shared machine hits both alike
            for k, f in fns.items():
                us[k].append(timed(f, iters[k]))
        med = {k: statistics.median(v) for k, v in us.items()}
        for k, v in us.items():
            r = {"shape": name, "M": M, "N": N, "K": K, "variant": k, "us": round(med[k], 1), "us_min": round(min(v), 1),
                 "us_max": round(max(v), 1), "rounds": a.rounds, "iters": iters[k], "dtype": "bf16"}
            if k == "fused":
                r["composition_over_fused"] = round(med["composition"] / med[k], 3)
                r["tflops"] = round(2.0 * M * N * K / med[k] * 1e-6, 1)
            rows.append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(r) + "\n" for r in rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
