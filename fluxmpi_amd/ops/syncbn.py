"""Synchronised BatchNorm: batch statistics over every rank's shard, on the fused NHWC kernels.

``FusedBatchNorm2d`` normalises with the statistics of the local shard. Here the BatchNorm of
``csrc/kernels/batchnorm.hip`` is stopped at its two seams and one small SUM-allreduce is put in each:

forward   statistics pass -> fold -> **allreduce(msg_f)** -> finalize from the message -> apply pass
backward  reduce pass     -> fold -> **allreduce(msg_b)** -> dx pass

Messages (fp32, always fp32 on the wire):

``msg_f [2C + 2] = (sum x [C], sum x^2 [C], n_hi, n_lo)`` of the local rows, ``n = 4096 n_hi + n_lo``,
``msg_b [2C]     = (sum g [C], sum g xhat [C])`` with g the (ReLU-masked) output gradient.

Sums, not means: a SUM of per-shard sums IS the sum of the concatenated batch whatever the shard sizes
(uneven and empty shards need no weights), and sums of small integers stay exact, which the tests use.
Two count slots: one fp32 slot is exact only below 2^24 rows, and ResNet-50's first BatchNorm at batch
256 over 8 ranks has 25.7 M; ``n_lo < 4096`` per rank and ``n_hi < rows / 4096`` stay exact under a SUM
over any realistic world. The count is read on the device: nothing here reads it back to the host.

The reductions are deterministic: every workgroup stores its own ``[2][C]`` partial and a fold kernel
sums the partials in an order that depends on (rows, C) alone. There are no float atomics, so two runs
agree to the bit, and at world size 1 (or without ``Init``) the path doubles as a run-to-run
repeatable BatchNorm, with no collective and the fold and the finalize in one launch.

The parameter gradients ``dw`` / ``db`` stay LOCAL sums: the data-parallel engine's SUM-allreduce of the
gradients completes them, and the result is the gradient of ``sum_r L_r``.

The op-level functions (:func:`forward_message`, :func:`apply_from_message`, :func:`backward_message`,
:func:`dx_from_message`) are public, so one process can play W ranks by summing messages itself. CPU
tensors and layouts the kernels do not cover run the same protocol in PyTorch, so every rank always
enters the same collectives.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _ext
from ._launch import nhwc as _nhwc, ptr as _p, stream as _stream
from .batchnorm import (GradLink, _grad_out, _rows_c, bn_counter, finish_bwd, fused_batch_norm, hands_masked,
                        launch_apply)
from .multi_tensor import DTYPE_CODE

COUNT_RADIX = 4096  # == kCountRadix in csrc/kernels/batchnorm.hip


def split_count(n: int):
    """``(n_hi, n_lo)`` with ``n = 4096 n_hi + n_lo`` and ``n_lo < 4096``: both exact in fp32 up to 2^36 rows."""
    return n // COUNT_RADIX, n % COUNT_RADIX


def join_count(n_hi, n_lo) -> int:
    """The row count of a (summed) message's two count slots."""
    return int(n_hi) * COUNT_RADIX + int(n_lo)


def kernel_covers(x: torch.Tensor) -> bool:
    """The layouts of the HIP path (an empty shard included: it launches nothing)."""
    if not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float16, torch.float32) or x.dim() not in (2, 4):
        return False
    return x.shape[1] % 8 == 0 and 8 <= x.shape[1] <= 2048


_PART: dict = {}
_PART_MIN = 1 << 18


def _partials(x: torch.Tensor, rows: int, ch: int) -> torch.Tensor:
    """The persistent partial buffer of a (device, stream), grown on demand. Every workgroup writes its
    whole partial before the fold reads it, so it is never zeroed and nothing stale can be read."""
    need = _ext.get(required=True).bn_sync_workspace_floats(rows, ch)
    key = (x.device.index, torch.cuda.current_stream(x.device).cuda_stream)
    buf = _PART.get(key)
    if buf is None or buf.numel() < need:
        buf = torch.empty(max(need, _PART_MIN), device=x.device, dtype=torch.float32)
        _PART[key] = buf
    return buf


def _rows2d(x: torch.Tensor) -> torch.Tensor:
    """``[rows, C]`` view / copy of a 2-D or 4-D (NCHW-shaped) tensor."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]) if x.dim() == 4 else x


def _shaped(t2: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    if like.dim() == 4:
        n, c, h, w = like.shape
        return t2.reshape(n, h, w, c).permute(0, 3, 1, 2)
    return t2


def _count_of(msg_or_count: torch.Tensor) -> torch.Tensor:
    """int64 row count (0-d, on the message's device) of the last two slots."""
    return msg_or_count[-2].to(torch.int64) * COUNT_RADIX + msg_or_count[-1].to(torch.int64)


# ------------------------------------------------------------------------------------- op level

def forward_message(x: torch.Tensor) -> torch.Tensor:
    """``[2C + 2]`` fp32: (sum x, sum x^2, n_hi, n_lo) of this shard (zeros for an empty one)."""
    rows, ch = _rows_c(x)
    if rows == 0:
        return torch.zeros(2 * ch + 2, device=x.device, dtype=torch.float32)
    if kernel_covers(x):
        x = _nhwc(x)
        msg = torch.empty(2 * ch + 2, device=x.device, dtype=torch.float32)
        _ext.get(required=True).bn_sync_stats(x.data_ptr(), _partials(x, rows, ch).data_ptr(), msg.data_ptr(), rows,
                                              ch, DTYPE_CODE[x.dtype], _stream(x), 0, 0, 0, 0, 0.0, 0.0, 0)
        return msg
    xf = _rows2d(x).float()
    hi, lo = split_count(rows)
    return torch.cat([xf.sum(0), (xf * xf).sum(0), torch.tensor([hi, lo], device=x.device, dtype=torch.float32)])


def stats_from_message(msg, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, num_batches_tracked=None):
    """``(save_mean, save_invstd)`` of the batch a (summed) forward message describes; updates the running
    statistics with the unbiased variance of that batch and increments ``num_batches_tracked``."""
    ch = (msg.numel() - 2) // 2
    if msg.is_cuda and ch % 8 == 0 and 8 <= ch <= 2048:
        sm = torch.empty(ch, device=msg.device, dtype=torch.float32)
        si = torch.empty(ch, device=msg.device, dtype=torch.float32)
        _ext.get(required=True).bn_sync_finalize_fwd(msg.data_ptr(), _p(running_mean), _p(running_var), sm.data_ptr(),
                                                     si.data_ptr(), ch, float(momentum), float(eps), _stream(msg),
                                                     _p(num_batches_tracked))
        return sm, si
    n = _count_of(msg)
    any_rows = n >= 1
    nf = n.clamp_min(1).float()
    inv_n = 1.0 / nf
    mean = msg[:ch] * inv_n
    var = (msg[ch:2 * ch] * inv_n - mean * mean).clamp_min(0)
    inv = torch.rsqrt(var + eps)
    if running_mean is not None:
        unbiased = torch.where(n > 1, var * nf / (n - 1).clamp_min(1).float(), var)
        with torch.no_grad():
            running_mean.copy_(torch.where(any_rows, (1 - momentum) * running_mean + momentum * mean, running_mean))
            running_var.copy_(torch.where(any_rows, (1 - momentum) * running_var + momentum * unbiased, running_var))
    if num_batches_tracked is not None:
        num_batches_tracked.add_(1)
    return mean, inv


def apply_stats(x, save_mean, save_invstd, weight=None, bias=None, relu=False, residual=None):
    """``(y, mask)``: the apply pass from finished statistics. ``mask`` is what the backward wants: the
    1-bit-per-element bytes of the kernels (kept only for ReLU after a residual; otherwise the kernels
    recompute it from x), or a bool tensor ``[rows, C]`` on the PyTorch path."""
    rows, ch = _rows_c(x)
    if kernel_covers(x):
        x = _nhwc(x)
        if rows == 0:
            return torch.empty_like(x), None
        return launch_apply(x, weight, bias, save_mean, save_invstd, relu, residual)
    scale = save_invstd if weight is None else weight.float() * save_invstd
    shift = -save_mean * scale if bias is None else bias.float() - save_mean * scale
    o = _rows2d(x).float() * scale + shift
    if residual is not None:
        o = o + _rows2d(residual).float()
    mask = None
    if relu:
        mask = o > 0
        o = torch.where(mask, o, torch.zeros_like(o))
    return _shaped(o.to(x.dtype), x), mask


def apply_from_message(x, msg, weight=None, bias=None, running_mean=None, running_var=None, momentum=0.1, eps=1e-5,
                       relu=False, residual=None, num_batches_tracked=None):
    """``(y, mask, save_mean, save_invstd)`` from a (summed) forward message. ``weight`` / ``bias`` fp32."""
    sm, si = stats_from_message(msg, running_mean, running_var, momentum, eps, num_batches_tracked)
    y, mask = apply_stats(x, sm, si, weight, bias, relu, residual)
    return y, mask, sm, si


def _g_fallback(dy, x, mask, weight, bias, save_mean, save_invstd, relu):
    g = _rows2d(dy).float()
    xf = _rows2d(x).float()
    if relu:
        if mask is None:  # no residual: the decision is that of the forward's x scale + shift
            scale = save_invstd if weight is None else weight.float() * save_invstd
            shift = -save_mean * scale if bias is None else bias.float() - save_mean * scale
            mask = (xf * scale + shift) > 0
        g = g * mask
    return g, xf


def backward_message(dy, x, mask, weight, bias, save_mean, save_invstd, relu=False, dw=None, db=None):
    """``(msg [2C], dw, db)``: (sum g, sum g xhat) of this shard, which are also its local ``db`` / ``dw``
    (written into the given buffers when present). Zeros for an empty shard."""
    rows, ch = _rows_c(x)
    dw = torch.empty(ch, device=x.device, dtype=torch.float32) if dw is None else dw
    db = torch.empty(ch, device=x.device, dtype=torch.float32) if db is None else db
    if rows == 0:
        dw.zero_()
        db.zero_()
        return torch.zeros(2 * ch, device=x.device, dtype=torch.float32), dw, db
    if kernel_covers(x):
        x, dy = _nhwc(x), _nhwc(dy)
        msg = torch.empty(2 * ch, device=x.device, dtype=torch.float32)
        _ext.get(required=True).bn_sync_bwd_reduce(dy.data_ptr(), x.data_ptr(), 0, _p(mask), _p(weight), _p(bias),
                                                   save_mean.data_ptr(), save_invstd.data_ptr(),
                                                   _partials(x, rows, ch).data_ptr(), msg.data_ptr(), dw.data_ptr(),
                                                   db.data_ptr(), rows, ch, int(relu), DTYPE_CODE[x.dtype],
                                                   _stream(x))
        return msg, dw, db
    g, xf = _g_fallback(dy, x, mask, weight, bias, save_mean, save_invstd, relu)
    msg = torch.cat([g.sum(0), (g * ((xf - save_mean) * save_invstd)).sum(0)])
    db.copy_(msg[:ch])
    dw.copy_(msg[ch:])
    return msg, dw, db


def dx_from_message(dy, x, mask, weight, bias, save_mean, save_invstd, msg, count=None, relu=False,
                    want_dres=False):
    """``(dx, dres)`` of this shard from a (summed) backward message. ``count``: the two count slots of the
    summed forward message (a ``[2]`` fp32 tensor), or None when ``msg`` holds this shard's sums alone."""
    rows, ch = _rows_c(x)
    if kernel_covers(x):
        x, dy = _nhwc(x), _nhwc(dy)
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if want_dres else None
        if rows == 0:
            return dx, dres
        coef = torch.empty(2 * ch, device=x.device, dtype=torch.float32) if count is not None else None
        _ext.get(required=True).bn_sync_bwd_dx(dy.data_ptr(), x.data_ptr(), 0, _p(mask), _p(weight), _p(bias),
                                               save_mean.data_ptr(), save_invstd.data_ptr(), msg.data_ptr(),
                                               _p(count), _p(coef), dx.data_ptr(), _p(dres), rows, ch, int(relu),
                                               DTYPE_CODE[x.dtype], _stream(x))
        return dx, dres
    g, xf = _g_fallback(dy, x, mask, weight, bias, save_mean, save_invstd, relu)
    n = _count_of(count).clamp_min(1).float() if count is not None else float(max(rows, 1))
    inv_n = 1.0 / n
    k2, k3 = msg[:ch] * inv_n, msg[ch:] * inv_n
    a = save_invstd if weight is None else weight.float() * save_invstd
    b = -a * save_invstd * k3
    d = a * (save_mean * save_invstd * k3 - k2)
    dx = _shaped((a * g + (b * xf + d)).to(x.dtype), x)
    return dx, (_shaped(g.to(x.dtype), x) if want_dres else None)


# ------------------------------------------------------------------------------------- autograd

def _world() -> int:
    from ..parallel import runtime
    if not runtime.Initialized() or runtime.Finalized():
        return 1
    return runtime.total_workers()


def _allreduce(msg: torch.Tensor) -> None:
    from ..parallel import runtime
    runtime.comm_for(msg).allreduce(msg)


class _SyncBN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, momentum, eps, relu, link, nbt):
        world = _world()
        use_k = kernel_covers(x)
        if world > 1 and x.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("sync_batch_norm: HIP-graph capture with more than one rank is not supported "
                               "(the statistics collectives are not captured); capture works at world size 1")
        if use_k:
            x = _nhwc(x)
        rows, ch = _rows_c(x)
        w32 = weight.float() if weight is not None else None
        b32 = bias.float() if bias is not None else None
        if world == 1 and use_k and rows > 0:
            # no collective: statistics pass, then fold + finalize in one launch
            msg = torch.empty(2 * ch + 2, device=x.device, dtype=torch.float32)
            sm = torch.empty(ch, device=x.device, dtype=torch.float32)
            si = torch.empty(ch, device=x.device, dtype=torch.float32)
            _ext.get(required=True).bn_sync_stats(x.data_ptr(), _partials(x, rows, ch).data_ptr(), msg.data_ptr(),
                                                  rows, ch, DTYPE_CODE[x.dtype], _stream(x), sm.data_ptr(),
                                                  si.data_ptr(), _p(running_mean), _p(running_var), float(momentum),
                                                  float(eps), _p(nbt))
            count = None
        else:
            msg = forward_message(x)
            if world > 1:
                _allreduce(msg)
            sm, si = stats_from_message(msg, running_mean, running_var, momentum, eps, nbt)
            count = msg[2 * ch:]
        y, mask = apply_stats(x, sm, si, w32, b32, relu, residual)
        ctx.relu, ctx.world, ctx.has_res = relu, world, residual is not None
        # off the kernels the link is ignored (as fused_batch_norm does): autograd gets the residual gradient
        ctx.link = link if (residual is not None and use_k) else None
        ctx.wdtype = weight.dtype if weight is not None else None
        ctx.has_bias = bias is not None
        ctx.params = (weight, bias)
        ctx.save_for_backward(x, mask, w32, b32, sm, si, count)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mask, w32, b32, sm, si, count = ctx.saved_tensors
        rows, ch = _rows_c(x)
        if kernel_covers(x):
            dy = _nhwc(dy)
        dw, db = (_grad_out(p, ch, x) for p in ctx.params)
        msg, dw, db = backward_message(dy, x, mask, w32, b32, sm, si, ctx.relu, dw, db)
        if ctx.world > 1:
            _allreduce(msg)
        hand_masked = hands_masked(ctx.link, mask, ctx.relu)  # (off the kernels the mask is a bool tensor)
        dx, dres = dx_from_message(dy, x, mask, w32, b32, sm, si, msg, count, ctx.relu,
                                   ctx.has_res and not hand_masked)
        dw, db, dres = finish_bwd(dw, db, ctx.wdtype, w32 is not None, ctx.has_bias, ctx.link, dy, mask, dres,
                                  hand_masked)
        return dx, dw, db, dres, None, None, None, None, None, None, None


def sync_batch_norm(x, weight, bias, running_mean, running_var, training=True, momentum=0.1, eps=1e-5, relu=False,
                    residual=None, link: GradLink | None = None, num_batches_tracked: torch.Tensor | None = None,
                    bnlink=None):
    """BatchNorm(+ReLU)(+residual add) with the statistics of every rank's rows (see the module docstring).

    While ``training``, every rank must call this the same number of times in the same order (an empty
    shard included): each call is one collective forward and one backward. Eval mode is the inference
    path of :func:`fused_batch_norm` and issues no collective. ``link`` / ``num_batches_tracked`` as there.
    """
    if bnlink is not None:
        raise ValueError("sync_batch_norm: bnlink (BatchNorm-backward sums from a GEMM epilogue) is not supported: "
                         "those sums are local to the rank")
    if not training:
        return fused_batch_norm(x, weight, bias, running_mean, running_var, False, momentum, eps, relu, residual)
    return _SyncBN.apply(x, weight, bias, residual, running_mean, running_var, momentum, eps, relu, link,
                         num_batches_tracked)


class SyncBatchNorm2d(nn.BatchNorm2d):
    """``nn.BatchNorm2d`` (same state-dict keys) whose training statistics run over every rank's shard,
    with the optional fused ReLU / residual add of :class:`FusedBatchNorm2d`."""

    def forward(self, x, relu: bool = False, residual: torch.Tensor | None = None, link: GradLink | None = None):
        rm = self.running_mean if self.track_running_stats else None
        rv = self.running_var if self.track_running_stats else None
        if not self.training:  # as in PyTorch, synchronised only while training
            return fused_batch_norm(x, self.weight, self.bias, rm, rv, not self.track_running_stats,
                                    0.1 if self.momentum is None else self.momentum, self.eps, relu, residual)
        mom, nbt = bn_counter(self)
        return sync_batch_norm(x, self.weight, self.bias, rm, rv, True, mom, self.eps, relu, residual, link, nbt)


def convert_sync_batchnorm(module: nn.Module) -> nn.Module:
    """Replace every ``nn.BatchNorm2d`` / ``FusedBatchNorm2d`` under ``module`` by a :class:`SyncBatchNorm2d`
    that SHARES its parameters and buffers (same tensors, same ``requires_grad``, same training flag);
    returns the module (or the replacement, when ``module`` itself is a BatchNorm)."""
    from ..models.resnet import ResNet

    nets = [m for m in module.modules() if isinstance(m, ResNet)]
    for m in nets:
        if m.conv_impl in ("fused", "hybrid"):
            raise ValueError(f"convert_sync_batchnorm: a ResNet with conv_impl={m.conv_impl!r} reads its BatchNorm "
                             "parameters past the modules' forward (fused blocks, stem) and would stay "
                             "unsynchronised; build it with conv_impl 'gemm' or 'miopen'")
    for m in nets:
        # norm="fused" sends the stem through the fused BN + ReLU + max-pool kernel, which reads bn1's parameters
        # and computes local statistics of its own: norm="sync" runs maxpool(bn1(conv, relu=True)) instead
        if m.norm_kind == "fused":
            m.norm_kind = "sync"
    return _convert(module)


def _convert(m: nn.Module) -> nn.Module:
    if isinstance(m, nn.BatchNorm2d) and not isinstance(m, SyncBatchNorm2d):
        new = SyncBatchNorm2d(m.num_features, m.eps, m.momentum, False, False)
        new.affine, new.track_running_stats = m.affine, m.track_running_stats
        for k, p in m._parameters.items():
            new._parameters[k] = p
        for k, b in m._buffers.items():
            new._buffers[k] = b
        new.training = m.training
        return new
    for name, child in m.named_children():
        setattr(m, name, _convert(child))
    return m


__all__ = ["SyncBatchNorm2d", "convert_sync_batchnorm", "sync_batch_norm", "forward_message", "stats_from_message",
           "apply_stats", "apply_from_message", "backward_message", "dx_from_message", "split_count", "join_count"]
