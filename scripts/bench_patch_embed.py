#!/usr/bin/env python
"""The ViT patch embedding as one implicit GEMM (``ops.patch_embed``, ``csrc/kernels/patch_embed.hip``)
against today's composition (the unfold copy + ``Linear`` + ``cls_pos``, and its backward).

Case: ViT-B/16 front end, batch 256, 224 x 224, p = 16, D = 768, bf16 ``channels_last`` input with 3 and
with 4 channels (the composition reads ``x[:, :3]`` of the 4-channel batch). Variants, alternated in one
process, each a HIP-graph replay:

  fused_c3_fwd / fused_c4_fwd         pack + patch_embed_fwd
  unfold_c3_fwd / unfold_c4_fwd       reshape-permute-reshape copy, Linear forward, cls_pos
  fused_c3_fwdbwd / fused_c4_fwdbwd   the above + patch_embed_wgrad, the slab reduce, one batch sum of dy
  unfold_c3_fwdbwd / unfold_c4_fwdbwd the above + the Linear's weight / bias gradient, _ClsPos' two sums

One JSON line per variant; ``faster_than_unfold_worst_case`` compares the fused path's slowest round
with the composition's fastest.

usage: python scripts/bench_patch_embed.py [--out profiles/patch_embed_vit_b16.jsonl] [--rounds 7] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluxmpi_amd.models.vit import PatchEmbed, _ClsPos, cls_pos  # noqa: E402
from fluxmpi_amd.ops.patch_embed import patch_embed  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "patch_embed_vit_b16.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_patch_embed.py needs a GPU", file=sys.stderr)
        return 2
    B, S, p, D = a.batch, 224, 16, 768
    n = (S // p) ** 2
    torch.manual_seed(0)
    emb = PatchEmbed(S, p, 3, D).cuda().bfloat16()
    cls = torch.nn.Parameter(torch.randn(1, 1, D, device="cuda").bfloat16())
    pos = torch.nn.Parameter((torch.randn(1, n + 1, D, device="cuda") * 0.02).bfloat16())
    params = [emb.proj.weight, emb.proj.bias, cls, pos]
    dy = torch.randn(B, n + 1, D, device="cuda").bfloat16()
    fns, outs, keep = {}, {}, []
    for C in (3, 4):
        x = torch.randn(B, C, S, S, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
        # a captured kernel reads the batch by address: it must outlive the capture, not just this iteration
        keep.append(x)

        def fused(x=x):
            return patch_embed(x, emb.proj.weight, emb.proj.bias, cls, pos, p)

        def unfold(x=x):
            t = emb(x[:, :3])
            return _ClsPos.apply(t, cls, pos) if torch.is_grad_enabled() else cls_pos(t, cls, pos)

        for name, f in (("fused", fused), ("unfold", unfold)):
            def fwd(f=f):
                with torch.no_grad():
                    return f()

            def fwdbwd(f=f):
                for q in params:
                    q.grad = None
                f().backward(dy)
                return [q.grad for q in params]

            keep += [f, fwd, fwdbwd]
            fns[f"{name}_c{C}_fwd"], outs[f"{name}_c{C}_fwd"] = graphed(fwd)
            fns[f"{name}_c{C}_fwdbwd"], outs[f"{name}_c{C}_fwdbwd"] = graphed(fwdbwd)
            print(f"captured {name}_c{C}", file=sys.stderr, flush=True)
    for fn in fns.values():
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    print("replayed", file=sys.stderr, flush=True)
    # after several replays the two routes agree (one rounding against two in the forward; bf16 sums)
    for C in (3, 4):
        d = (outs[f"fused_c{C}_fwd"].float() - outs[f"unfold_c{C}_fwd"].float()).abs().max().item()
        assert d <= 0.07, (C, d)
        for gf, gu in zip(outs[f"fused_c{C}_fwdbwd"], outs[f"unfold_c{C}_fwdbwd"]):
            rel = ((gf.float() - gu.float()).abs().max() / gu.float().abs().max()).item()
            assert rel <= 0.02, (C, rel)
    us = {k: [] for k in fns}
    for _ in range(a.rounds):  # alternate the variants: drift of the shared machine hits all alike
        for k, fn in fns.items():
            us[k].append(timed(fn, a.iters))
    med = {k: statistics.median(v) for k, v in us.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for k, v in us.items():
            r = {"variant": k, "us": round(med[k], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                 "rounds": a.rounds, "iters": a.iters, "mode": "graph", "batch": B, "image": [S, S], "patch": p,
                 "dim": D, "dtype": "bf16"}
            if k.startswith("fused_"):
                t = "unfold_" + k[6:]
                r["unfold_over_fused"] = round(med[t] / med[k], 2)
                r["faster_than_unfold_worst_case"] = bool(max(v) < min(us[t]))
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
