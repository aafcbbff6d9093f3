"""Training from a uint8 image set: a rank's shard of the bytes goes through the device input pipeline
(random crop, flip, normalise, NHWC bf16, the stem's 4-channel format, mixup) in one kernel per batch, then
through ResNet under the DDP engine. The mixed labels go to the fused loss as two integer labels and lam
(no dense target); the running loss and top-1 / top-5 counts stay on the device and are read every 10 steps.

Run:  torchrun --nproc-per-node 8 examples/train_augment.py --model resnet50 --batch 256 --steps 100
      python -m fluxmpi_amd.launch -n 2 examples/train_augment.py --model resnet_tiny --batch 8 --image 32 (CPU)

The image set here is random bytes (what a decoded, resized data set looks like in memory); decoding
and host loading are not this example's subject.
"""
import argparse
import time

import torch

import fluxmpi_amd as FluxMPI
from fluxmpi_amd import optimisers as O
from fluxmpi_amd.models import build_model
from fluxmpi_amd.parallel.ddp import DDP

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="resnet50")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--image", type=int, default=224, help="the crop fed to the model; the stored images are 8/7 of it")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--items", type=int, default=None, help="images in the whole set (default: 4 batches per rank)")
ap.add_argument("--mixup", type=float, default=0.2)
ap.add_argument("--cutmix", type=float, default=0.0)
ap.add_argument("--smoothing", type=float, default=0.1)
ap.add_argument("--crop", choices=("pad", "resized"), default="pad",
                help="pad: a crop of the stored image by translation; resized: RandomResizedCrop(scale=(0.08, 1), "
                     "ratio=(3/4, 4/3)) resampled bilinearly, the ImageNet recipe (evaluation: Resize + CenterCrop)")
args = ap.parse_args()

FluxMPI.Init()
dev = FluxMPI.device()
classes = 10 if args.model == "resnet_tiny" else 1000
kw = {"norm": "fused"} if args.model.startswith("resnet") and dev.type == "cuda" else {}
model = build_model(args.model, **kw).to(dev)
if dev.type == "cuda":
    model = model.to(memory_format=torch.channels_last)
    for m in model.modules():
        if not isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            for p in m.parameters(recurse=False):
                p.data = p.data.bfloat16()
ddp = DDP(model, O.AdamW(1e-3, decay=1e-4), average=True)

# the whole set, the same on every rank; each rank keeps its contiguous shard of images and labels
stored = args.image * 8 // 7
items = args.items or 4 * args.batch * FluxMPI.total_workers()
g = torch.Generator().manual_seed(0)
images = torch.randint(0, 256, (items, stored, stored, 3), dtype=torch.uint8, generator=g)
labels = torch.randint(0, classes, (items,), generator=g)
shard_x = FluxMPI.DistributedDataContainer(images)
shard_y = FluxMPI.DistributedDataContainer(labels)
per_epoch = max(1, len(shard_x) // args.batch)

# channels=4: the ResNet stem's own input format, so the stem runs no pad pass; every rank draws
# different crops from the one seed (sample_offset = local_rank * batch)
aug = FluxMPI.DeviceAugment(args.image, channels=4 if dev.type == "cuda" else 3,
                            dtype=torch.bfloat16, seed=0, mixup_alpha=args.mixup, cutmix_alpha=args.cutmix,
                            label_smoothing=args.smoothing, num_classes=classes, targets="labels", crop=args.crop)
meter = FluxMPI.ClassificationMeter(topk=(1, 5))

t0 = time.time()
for step in range(args.steps):
    lo = (step % per_epoch) * args.batch
    u8 = shard_x[lo:lo + args.batch].to(dev, non_blocking=True)  # the bytes: 1/4 of the bf16 batch
    y = shard_y[lo:lo + args.batch].to(dev, non_blocking=True)
    x, target = aug(u8, y)  # [B, C, h, w] channels_last; MixedLabels(labels, lam, smoothing)
    if dev.type != "cuda":
        x = x.float()
    loss = FluxMPI.softmax_cross_entropy(ddp(x), target, meter=meter)  # the meter takes the batch in on the device
    loss.backward()
    ddp.step()
    if step % 10 == 9 or step == args.steps - 1:  # the only host read of the loop
        r = meter.read()
        FluxMPI.fluxmpi_println(f"step {step} loss {r['loss']:.4f} top1 {r['top1']:.3f} top5 {r['top5']:.3f} "
                                f"over {r['rows']} samples (mix {aug.draw(step)})")
        meter.reset()

model.eval()
with torch.no_grad():  # evaluation: the centre crop, no flip, no mix
    x, y = aug.eval()(shard_x[0:args.batch].to(dev), shard_y[0:args.batch].to(dev))
    meter.reset()
    FluxMPI.softmax_cross_entropy(ddp(x if dev.type == "cuda" else x.float()), y, meter=meter)
    r = meter.read(reduce=True)  # summed over the ranks
FluxMPI.fluxmpi_println(f"centre-crop on a training batch: loss {r['loss']:.4f} top1 {r['top1']:.3f} "
                        f"top5 {r['top5']:.3f} over {r['rows']} samples")
if FluxMPI.local_rank() == 0:
    print(f"{args.steps * args.batch * FluxMPI.total_workers() / (time.time() - t0):.1f} samples/s")
FluxMPI.Finalize()
