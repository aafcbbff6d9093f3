"""Fused ResNet stem tail: BatchNorm (batch statistics) + ReLU + max-pool, NHWC.

``bn_relu_maxpool(x, bn, k=3, s=2, p=1)`` == ``max_pool2d(relu(bn(x)), k, s, p)`` in
training mode, with the normalised full-resolution activation never written:
one statistics pass over the conv output, then one kernel that normalises,
rectifies and pools (``csrc/kernels/pool.hip``) and records a 1-byte window
index per pooled element. The backward gathers the pooled gradient back to full
resolution (no zero fill, no atomics) and runs the fused BatchNorm backward.

Compared with conv -> BN -> ReLU -> MaxPool2d this removes a write and a read of
the 112x112x64 activation and the pool's int64 index tensor (8 B per pooled
element vs 1 B here).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _ext
from ._launch import nhwc, stream
from .batchnorm import launch_bwd, launch_finalize
from .fused_block import _empty_nhwc
from .multi_tensor import DTYPE_CODE


def _out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


class _BNReluMaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, k, s, p, nbt=None):
        C = _ext.get(required=True)
        x = nhwc(x)
        n, ch, h, w = x.shape
        w32 = weight.float() if weight is not None else torch.ones(ch, device=x.device)
        b32 = bias.float() if bias is not None else torch.zeros(ch, device=x.device)
        mean, inv, scale, shift = launch_finalize(x, w32, b32, running_mean, running_var, momentum, eps, nbt,
                                                  pending=False, affine=True)
        oh, ow = _out(h, k, s, p), _out(w, k, s, p)
        y = _empty_nhwc(n, ch, oh, ow, x)
        idx = torch.empty(n * oh * ow * ch, device=x.device, dtype=torch.uint8)
        C.bn_relu_maxpool_fwd(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(), idx.data_ptr(), n, h, w,
                              ch, k, s, p, DTYPE_CODE[x.dtype], stream(x))
        ctx.geo = (k, s, p)
        ctx.wdtype = weight.dtype if weight is not None else None
        ctx.has_affine = (weight is not None, bias is not None)
        ctx.save_for_backward(x, idx, w32, b32, mean, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = _ext.get(required=True)
        x, idx, w32, b32, mean, inv = ctx.saved_tensors
        dy = nhwc(dy)
        n, ch, h, w = x.shape
        k, s, p = ctx.geo
        dz = torch.empty_like(x)  # gradient of the pre-ReLU normalised activation
        C.maxpool_bwd(dy.data_ptr(), idx.data_ptr(), dz.data_ptr(), n, h, w, ch, k, s, p, DTYPE_CODE[x.dtype],
                      stream(x))
        dx, _, dw, db = launch_bwd(dz, x, None, w32, b32, mean, inv, False)
        has_w, has_b = ctx.has_affine
        return (dx, dw.to(ctx.wdtype) if has_w else None, db.to(ctx.wdtype) if has_b else None,
                None, None, None, None, None, None, None, None)


def pad_c3_to_c4(x: torch.Tensor) -> torch.Tensor:
    """NHWC ``[N, H, W, 3]`` -> ``[N, H, W, 4]`` with a zero 4th channel (16-bit dtypes), one HIP
    pass (``csrc/kernels/pool.hip``); returned as the NCHW-shaped channels_last view."""
    C = _ext.get(required=True)
    n, c, h, w = x.shape
    xp = x.permute(0, 2, 3, 1)
    if c != 3 or not xp.is_contiguous() or x.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("pad_c3_to_c4: needs a channels_last bf16/fp16 [N, 3, H, W] tensor")
    y = torch.empty(n, h, w, 4, device=x.device, dtype=x.dtype)
    C.pad_c3_to_c4(xp.data_ptr(), y.data_ptr(), n * h * w, DTYPE_CODE[x.dtype], stream(x))
    return y.permute(0, 3, 1, 2)


def geometry_supported(k: int, s: int, p: int) -> bool:
    """Window geometries both kernels run: the 1-byte index holds ``k * k <= 255`` taps, the padding
    is smaller than the window, and the backward gathers from at most 3 x 3 windows per input
    position (``ceil(k / s) <= 3``). Anything else takes the reference composition in the forward
    (the forward kernel alone would accept ``k = 4, s = 1`` and the backward then raise mid-autograd)."""
    return 1 <= k and k * k <= 255 and s >= 1 and 0 <= p < k and -(-k // s) <= 3


def supported(x: torch.Tensor, k: int = 3, s: int = 2, p: int = 1) -> bool:
    if not (x.is_cuda and x.dim() == 4 and x.dtype in (torch.bfloat16, torch.float16, torch.float32)
            and x.shape[1] % 8 == 0 and 8 <= x.shape[1] <= 2048 and geometry_supported(k, s, p)):
        return False
    return _out(x.shape[2], k, s, p) >= 1 and _out(x.shape[3], k, s, p) >= 1


def bn_relu_maxpool(x: torch.Tensor, bn, k: int = 3, s: int = 2, p: int = 1) -> torch.Tensor:
    """``max_pool2d(relu(bn(x)), k, s, p)`` for a training-mode BatchNorm module ``bn``."""
    from .batchnorm import bn_counter
    mom, nbt = bn_counter(bn)
    if not (bn.training and supported(x, k, s, p)):
        if nbt is not None:
            nbt.add_(1)
        y = F.batch_norm(x.float(), bn.running_mean, bn.running_var,
                         bn.weight.float() if bn.weight is not None else None,
                         bn.bias.float() if bn.bias is not None else None,
                         bn.training or not bn.track_running_stats, mom, bn.eps)
        return F.max_pool2d(F.relu(y), k, s, p).to(x.dtype)
    rm = bn.running_mean if bn.track_running_stats else None
    rv = bn.running_var if bn.track_running_stats else None
    return _BNReluMaxPool.apply(x, bn.weight, bn.bias, rm, rv, mom, bn.eps, k, s, p, nbt)


__all__ = ["bn_relu_maxpool", "pad_c3_to_c4"]
