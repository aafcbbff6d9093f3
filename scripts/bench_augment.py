#!/usr/bin/env python
"""The device input pipeline (``ops.augment.augment_batch``, one kernel) against what a user composes
today from PyTorch ops on the device, and against the stem's pad pass that ``channels=4`` removes.

Case: batch 256, uint8 256 x 256 -> random 224 x 224 crop, flip, ImageNet normalisation, bf16 NHWC.
Variants, alternated in one process, each a HIP-graph replay:

  aug_c4 / aug_c4_mixup / aug_c4_cutmix / aug_c3      the kernel
  torch_c4 / torch_c4_mixup / torch_c4_cutmix / torch_c3
      the same transform from PyTorch ops: one advanced-index gather of the crop (the index tensors of
      the step's draws are built outside the timed region, in the composition's favour), float,
      (x / 255 - mean) / std, the mix, the bf16 cast, and for 4 channels ``pad_c3_to_c4``
  pad_c3_to_c4                                         the stem's pad pass alone on the same batch

Bytes moved by the kernel: the cropped region read once (twice when mixing), the output written once.
One JSON line per variant; ``faster_than_torch_worst_case`` compares the kernel's slowest round with
the composition's fastest.

usage: python scripts/bench_augment.py [--out profiles/augment_resnet50.jsonl] [--rounds 7] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluxmpi_amd.ops import augment as A  # noqa: E402
from fluxmpi_amd.ops.pool import pad_c3_to_c4  # noqa: E402


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


def torch_compose(u8, size, channels, mix, seed, step):
    """The composition a user writes today, as a closure over the step's index tensors."""
    B, H, W, _ = u8.shape
    h, w = size
    ox, oy, fl = A.sample_draws(B, seed, 0, step, 0, W - w + 1, H - h + 1)
    dev = u8.device
    ox, oy, fl = (torch.from_numpy(v).to(dev) for v in (ox, oy, fl))
    j = torch.arange(w, device=dev)
    rows = (oy[:, None] + torch.arange(h, device=dev))[:, :, None]
    cols = (torch.where(fl[:, None] == 1, w - 1 - j, j) + ox[:, None])[:, None, :]
    bidx = torch.arange(B, device=dev)[:, None, None]
    mean = torch.tensor(A.IMAGENET_MEAN, device=dev)
    std = torch.tensor(A.IMAGENET_STD, device=dev)
    y0, x0, y1, x1 = mix.box

    def run():
        y = (u8[bidx, rows, cols].float() / 255.0 - mean) / std  # [B, h, w, 3]
        if mix.mode == 1:
            y = mix.lam * y + (1.0 - mix.lam) * y.flip(0)
        elif mix.mode == 2:
            yp = y.flip(0)
            y = y.clone()
            y[:, y0:y1, x0:x1] = yp[:, y0:y1, x0:x1]
        x = y.to(torch.bfloat16).permute(0, 3, 1, 2)
        return pad_c3_to_c4(x) if channels == 4 else x

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "augment_resnet50.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_augment.py needs a GPU", file=sys.stderr)
        return 2
    B, H, W, size, seed, step = a.batch, 256, 256, (224, 224), 0, 0
    h, w = size
    g = torch.Generator(device="cuda").manual_seed(0)
    u8 = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    mixes = {"": A.MixDraw(), "_mixup": A.MixDraw(1, 0.3), "_cutmix": A.MixDraw(2, 0.75, (56, 56, 168, 168))}
    cases = [(4, ""), (4, "_mixup"), (4, "_cutmix"), (3, "")]
    fns, outs, info, keep = {}, {}, {}, []
    for C, m in cases:
        mix = mixes[m]
        out = torch.empty(B, h, w, C, dtype=torch.bfloat16, device="cuda")
        name = f"c{C}{m}"
        fns[f"aug_{name}"], outs[f"aug_{name}"] = graphed(
            lambda C=C, mix=mix, out=out: A.augment_batch(u8, size=size, channels=C, seed=seed, step=step, mix=mix,
                                                          out=out))
        # a captured gather reads its index tensors by address: the closure that owns them must outlive
        # the capture
        keep.append(torch_compose(u8, size, C, mix, seed, step))
        fns[f"torch_{name}"], outs[f"torch_{name}"] = graphed(keep[-1])
        moved = B * h * w * 3 * (2 if mix.mode else 1) + B * h * w * C * 2
        info[f"aug_{name}"] = {"bytes": moved}
        info[f"torch_{name}"] = {}
    x3 = outs["aug_c3"]
    fns["pad_c3_to_c4"], _ = graphed(lambda: pad_c3_to_c4(x3))
    info["pad_c3_to_c4"] = {"bytes": B * h * w * (3 + 4) * 2}
    for fn in fns.values():
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    # the two routes compute the same transform (the composition's formula differs in the last bits)
    for C, m in cases:
        d = (outs[f"aug_c{C}{m}"].float() - outs[f"torch_c{C}{m}"].float()).abs().max().item()
        assert d <= 0.04, (C, m, d)  # 2 bf16 ulp at |x| < 4
    us = {k: [] for k in fns}
    for _ in range(a.rounds):  # alternate the variants: drift of the shared machine hits all alike
        for k, fn in fns.items():
            us[k].append(timed(fn, a.iters))
    med = {k: statistics.median(v) for k, v in us.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for k, v in us.items():
            r = {"variant": k, "us": round(med[k], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                 "rounds": a.rounds, "iters": a.iters, "mode": "graph", "batch": B, "input": [H, W], "size": list(size),
                 "dtype": "bf16", **info[k]}
            if "bytes" in r:
                r["TBps"] = round(r["bytes"] / med[k] / 1e6, 2)
            if k.startswith("aug_"):
                t = "torch_" + k[4:]
                r["torch_over_aug"] = round(med[t] / med[k], 2)
                r["faster_than_torch_worst_case"] = bool(max(v) < min(us[t]))
                r["us_minus_pad_pass"] = round(med[k] - med["pad_c3_to_c4"], 1)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
