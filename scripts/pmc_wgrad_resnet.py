"""Two ResNet-50 (batch 256) weight gradients on gemm_wgrad for rocprofv3 --pmc passes: the 1x1
256 -> 1024 at 14x14 and the 3x3 256 at 14x14, after a warm-up 5 calls each, in the (variant, target
workgroups) configurations given as arguments ("2,512 2,1024": one per shape; default: the shipped
table's). Counters as for scripts/pmc_wgrad.py; summarise with scripts/pmc_summary.py."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluxmpi_amd.ops import conv_choice as CC  # noqa: E402
from fluxmpi_amd.ops import gemm as G  # noqa: E402

cfgs = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:3]] or [(2, 512), (2, 1024)]
if len(cfgs) == 1:
    cfgs = cfgs * 2
n, h, w = 256, 14, 14
dy1 = (torch.rand(n * h * w, 1024, device="cuda") - 0.5).bfloat16()
x1 = (torch.rand(n * h * w, 256, device="cuda") - 0.5).bfloat16()
dy3 = (torch.rand(n, 256, h, w, device="cuda") - 0.5).bfloat16().contiguous(memory_format=torch.channels_last)
x3 = (torch.rand(n, 256, h, w, device="cuda") - 0.5).bfloat16().contiguous(memory_format=torch.channels_last)
ops = [(cfgs[0], lambda: G.conv1x1_wgrad_v2(dy1, x1)), (cfgs[1], lambda: G.conv3x3_wgrad(dy3, x3))]
for cfg, fn in ops:
    CC._with_cfg(cfg, fn)
torch.cuda.synchronize()
for cfg, fn in ops:
    for _ in range(5):
        CC._with_cfg(cfg, fn)
torch.cuda.synchronize()
print("pmc_wgrad_resnet done", cfgs)
