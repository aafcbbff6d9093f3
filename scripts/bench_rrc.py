#!/usr/bin/env python
"""The resampling form of the device input pipeline (``ops.augment.resized_crop_batch``, one kernel)
against the translation-crop kernel on the same batch and against the same transform composed from
PyTorch ops on the device.

Case: batch 256, uint8 256 x 256 -> ``RandomResizedCrop(224)`` boxes of one fixed step, flip, ImageNet
normalisation, bf16 NHWC. Variants, alternated in one process, each a HIP-graph replay:

  rrc_c4 / rrc_c4_mixup / rrc_c4_cutmix / rrc_c3        the new kernel on a device table of boxes
  aug_c4 / aug_c4_mixup / aug_c4_cutmix / aug_c3        ``augment_batch`` (crop by translation): it writes
      the same bytes and reads fewer, so it is the reference point for what the resampling costs
  torch_c4 / torch_c4_mixup / torch_c4_cutmix / torch_c3
      the resized crop from PyTorch ops: a float NCHW copy of the batch, one batched ``affine_grid`` +
      ``grid_sample`` (bilinear, ``align_corners=False``; the thetas of the step's boxes are built outside
      the timed region, in the composition's favour), (x / 255 - mean) / std, the mix, the bf16 cast, and
      for 4 channels ``pad_c3_to_c4``

Bytes moved by the new kernel: every box read once (the partner's too when mixing), the output written
once. Host costs per step are recorded too: ``rrc_boxes`` for the batch and the upload of the table.
One JSON line per variant; ``faster_than_torch_worst_case`` compares the kernel's slowest round with the
composition's fastest.

usage: python scripts/bench_rrc.py [--out profiles/rrc_resnet50.jsonl] [--rounds 7] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

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


def torch_compose(u8, boxes, size, channels, mix):
    """The composition a user writes today, as a closure over the step's thetas."""
    B, H, W, _ = u8.shape
    h, w = size
    dev = u8.device
    t = torch.from_numpy(boxes).to(dev).double()
    top, left, bh, bw, flip = t.unbind(1)
    theta = torch.zeros(B, 2, 3, dtype=torch.float64, device=dev)
    theta[:, 0, 0] = (bw / W) * (1 - 2 * flip)  # source x = half-width * (+-x_out) + centre, in [-1, 1] units
    theta[:, 0, 2] = (2 * left + bw) / W - 1
    theta[:, 1, 1] = bh / H
    theta[:, 1, 2] = (2 * top + bh) / H - 1
    theta = theta.float()
    mean = torch.tensor(A.IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(A.IMAGENET_STD, device=dev).view(1, 3, 1, 1)
    y0, x0, y1, x1 = mix.box

    def run():
        grid = F.affine_grid(theta, (B, 3, h, w), align_corners=False)
        y = F.grid_sample(u8.permute(0, 3, 1, 2).float(), grid, mode="bilinear", padding_mode="border",
                          align_corners=False)  # [B, 3, h, w]
        y = (y / 255.0 - mean) / std
        if mix.mode == 1:
            y = mix.lam * y + (1.0 - mix.lam) * y.flip(0)
        elif mix.mode == 2:
            yp = y.flip(0)
            y = y.clone()
            y[:, :, y0:y1, x0:x1] = yp[:, :, y0:y1, x0:x1]
        x = y.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        return pad_c3_to_c4(x) if channels == 4 else x

    return run


def host_costs(B, H, W, table, reps=30):
    """Median host microseconds of a step's box draws and of the table's upload (the call, and the call
    with the wait for the copy)."""
    draw, call, done = [], [], []
    for i in range(reps):
        t0 = time.perf_counter()
        boxes = A.rrc_boxes(B, H, W, seed=0, step=i)
        t1 = time.perf_counter()
        table.copy_(torch.from_numpy(boxes))
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        draw.append((t1 - t0) * 1e6), call.append((t2 - t1) * 1e6), done.append((t3 - t1) * 1e6)
    return [statistics.median(v) for v in (draw, call, done)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "rrc_resnet50.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_rrc.py needs a GPU", file=sys.stderr)
        return 2
    B, H, W, size, seed, step = a.batch, 256, 256, (224, 224), 0, 0
    h, w = size
    g = torch.Generator(device="cuda").manual_seed(0)
    u8 = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    # neighbouring pixels of a real image are alike: smooth the noise, so that the two routes' weights
    # (11 bits here, fp32 there) give values the check below can compare
    u8 = F.avg_pool2d(u8.permute(0, 3, 1, 2).float(), 5, 1, 2).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    boxes = A.rrc_boxes(B, H, W, seed=seed, step=step)
    table = torch.from_numpy(boxes).cuda()
    area = boxes[:, 2].astype("int64") * boxes[:, 3]
    mixes = {"": A.MixDraw(), "_mixup": A.MixDraw(1, 0.3), "_cutmix": A.MixDraw(2, 0.75, (56, 56, 168, 168))}
    cases = [(4, ""), (4, "_mixup"), (4, "_cutmix"), (3, "")]
    fns, outs, info, keep = {}, {}, {}, []
    for C, m in cases:
        mix = mixes[m]
        name = f"c{C}{m}"
        out = torch.empty(B, h, w, C, dtype=torch.bfloat16, device="cuda")
        fns[f"rrc_{name}"], outs[f"rrc_{name}"] = graphed(
            lambda C=C, mix=mix, out=out: A.resized_crop_batch(u8, table, size=size, channels=C, mix=mix, out=out))
        out2 = torch.empty(B, h, w, C, dtype=torch.bfloat16, device="cuda")
        fns[f"aug_{name}"], outs[f"aug_{name}"] = graphed(
            lambda C=C, mix=mix, out=out2: A.augment_batch(u8, size=size, channels=C, seed=seed, step=step, mix=mix,
                                                           out=out))
        keep.append(torch_compose(u8, boxes, size, C, mix))  # the closure owns the captured thetas
        fns[f"torch_{name}"], outs[f"torch_{name}"] = graphed(keep[-1])
        written = B * h * w * C * 2
        # cutmix reads the partner's rows of the mixing box alone; counted as the whole box: an upper bound
        info[f"rrc_{name}"] = {"bytes": int(area.sum()) * 3 * (2 if mix.mode else 1) + written,
                               "mean_box_area_over_output": round(float(area.mean()) / (h * w), 3)}
        info[f"aug_{name}"] = {"bytes": B * h * w * 3 * (2 if mix.mode else 1) + written}
        info[f"torch_{name}"] = {}
    for fn in fns.values():
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    # the two routes compute the same transform: the composition's fp32 weights against 11-bit ones (one
    # byte level = 0.02 after normalisation, 2 bf16 ulp at |x| < 4 = 0.03), and grid_sample reads the
    # image's pixels beyond a box's edge where this op clamps to the box, so the edges are left out
    for C, m in cases:
        d = (outs[f"rrc_c{C}{m}"].float() - outs[f"torch_c{C}{m}"].float())[:, :3, 8:-8, 8:-8].abs()
        assert d.median().item() <= 0.02 and (d <= 0.06).float().mean().item() >= 0.99, (C, m, d.median(), d.max())
    us = {k: [] for k in fns}
    for _ in range(a.rounds):  # alternate the variants: drift of the shared machine hits all alike
        for k, fn in fns.items():
            us[k].append(timed(fn, a.iters))
    med = {k: statistics.median(v) for k, v in us.items()}
    draw_us, upload_call_us, upload_done_us = host_costs(B, H, W, table)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for k, v in us.items():
            r = {"variant": k, "us": round(med[k], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                 "rounds": a.rounds, "iters": a.iters, "mode": "graph", "batch": B, "input": [H, W], "size": list(size),
                 "dtype": "bf16", **info[k]}
            if "bytes" in r:
                r["TBps"] = round(r["bytes"] / med[k] / 1e6, 2)
            if k.startswith("rrc_"):
                t, c = "torch_" + k[4:], "aug_" + k[4:]
                r["torch_over_rrc"] = round(med[t] / med[k], 2)
                r["faster_than_torch_worst_case"] = bool(max(v) < min(us[t]))
                r["rrc_over_crop_kernel"] = round(med[k] / med[c], 2)
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
        line = json.dumps({"variant": "host_per_step", "batch": B, "rrc_boxes_us": round(draw_us, 1),
                           "table_upload_call_us": round(upload_call_us, 1),
                           "table_upload_until_done_us": round(upload_done_us, 1), "table_bytes": B * 20})
        print(line, flush=True)
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
