"""Host enqueue time of one ResNet-50 forward + backward (``conv_impl="hybrid"``, batch 32, bf16 NHWC): a host
clock from the first launch to the return of ``backward()``, no synchronise inside, one before and one after.
What the Python launch layer costs per step, apart from the kernels; one JSON line (median of ``--iters``)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    from fluxmpi_amd.models import resnet50
    from fluxmpi_amd.ops.conv_choice import freeze_choices
    freeze_choices()  # the deterministic defaults: both trees launch the same kernels
    dev = torch.device("cuda", 0)
    model = resnet50(num_classes=1000, conv_impl="hybrid", norm="fused").to(dev, memory_format=torch.channels_last)
    for m in model.modules():
        if not isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            for p in m.parameters(recurse=False):
                p.data = p.data.to(torch.bfloat16)
    x = torch.randn(args.batch, 3, 224, 224, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 1000, (args.batch,), device=dev)
    enqueue, total = [], []
    for i in range(args.warmup + args.iters):
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        F.cross_entropy(model(x).float(), y).backward()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= args.warmup:
            enqueue.append((t1 - t0) * 1e3)
            total.append((t2 - t0) * 1e3)
    print(json.dumps({"what": "resnet50 hybrid fwd+bwd host enqueue", "tag": args.tag, "batch": args.batch,
                      "iters": args.iters, "enqueue_ms_median": round(statistics.median(enqueue), 3),
                      "enqueue_ms_min": round(min(enqueue), 3), "enqueue_ms_max": round(max(enqueue), 3),
                      "fwd_bwd_ms_median": round(statistics.median(total), 3)}))


if __name__ == "__main__":
    main()
