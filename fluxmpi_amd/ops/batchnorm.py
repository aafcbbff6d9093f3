"""Fused NHWC BatchNorm(+ReLU)(+residual add) — autograd wrapper of ``csrc/kernels/batchnorm.hip``.

``FusedBatchNorm2d(C)(x, relu=True, residual=r)`` computes
``relu(batch_norm(x) + r)`` in two memory passes forward and two backward on
channels_last activations (GPU), vs ~7 / ~10 passes for the eager sequence.
Parameters and running statistics are fp32; activations may be bf16/fp16/fp32.
On CPU (and for layouts the kernels do not cover) the module runs the
PyTorch reference composition, which is also the test oracle.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _ext
from . import graddst
from ._launch import nhwc, ptr, stream
from .multi_tensor import DTYPE_CODE


def _rows_c(x: torch.Tensor):
    if x.dim() == 4:
        n, c, h, w = x.shape
        return n * h * w, c
    if x.dim() == 2:
        return x.shape[0], x.shape[1]
    raise ValueError("fused batchnorm expects 2D [N,C] or 4D [N,C,H,W] input")


_nhwc = nhwc  # the name ops/syncbn.py and scripts import


_SHARDS = 64  # == kShards in csrc/kernels/{batchnorm,gemm}.hip
_MAXC = 2048
# [_SHARDS][2][_MAXC] shards (+ 64 floats of slack)
_WS_FLOATS = _SHARDS * 2 * _MAXC + 64
_WS: dict = {}
_LWS: dict = {}
_DWS: dict = {}


def _persistent(pool: dict, x: torch.Tensor) -> torch.Tensor:
    """The zeroed fp32 accumulator of x's (device, stream) in ``pool``, made on first use."""
    key = (x.device.index, torch.cuda.current_stream(x.device).cuda_stream)
    ws = pool.get(key)
    if ws is None:
        ws = pool[key] = torch.zeros(_WS_FLOATS, device=x.device, dtype=torch.float32)
    return ws


def _workspace(x: torch.Tensor) -> torch.Tensor:
    """Persistent zeroed [64][2][2048] fp32 accumulator per (device, stream).

    The kernels leave it zeroed after every call (the finalize — a kernel of its own, or the
    last workgroup of the reduction kernel — re-zeroes the shards it consumes), so there is no
    memset per BatchNorm launch.
    """
    return _persistent(_WS, x)


def _link_workspace(x: torch.Tensor) -> torch.Tensor:
    """A second persistent zeroed accumulator, for BatchNorm-backward reductions that a GEMM
    epilogue deposits for a LATER BatchNorm backward (:class:`BNStatsLink`). Autograd may run
    another BatchNorm backward in between (e.g. a ResNet downsample branch between conv2's
    dgrad and bn1's backward), which reduces into :func:`_workspace`; keeping the linked sums
    apart makes the two independent."""
    return _persistent(_LWS, x)


def _dual_workspace(x: torch.Tensor) -> torch.Tensor:
    """Third persistent zeroed accumulator: the downsample branch's sums of the dual
    (bn3 + downsample BN) backward, reduced in the same pass as bn3's into :func:`_workspace`."""
    return _persistent(_DWS, x)


def kernel_supported(x: torch.Tensor) -> bool:
    if not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        return False
    if x.dim() not in (2, 4):
        return False
    c = x.shape[1]
    return c % 8 == 0 and 8 <= c <= 2048 and x.numel() > 0


def _grad_out(p, ch, like):
    """fp32 [ch] output for the gradient of BatchNorm parameter ``p``: its DDP bucket slice when
    one is attached (``graddst``, fp32 parameters), else a fresh tensor."""
    t = graddst.take(p, (ch,), torch.float32)
    return t if t is not None else torch.empty(ch, device=like.device, dtype=torch.float32)


class GradLink:
    """Hands the residual-branch gradient of a block from the BatchNorm that adds the
    residual straight to the 1x1 convolution that also consumes the block input.

    Without it autograd sums the two gradients of the block input with a separate add
    kernel (a read-read-write pass over the largest activation of the block); with it
    the BatchNorm backward deposits ``dres`` here and the convolution's dgrad GEMM adds
    it in its epilogue. Autograd's data dependencies guarantee the order (the conv's
    backward needs gradients that pass through the BatchNorm's backward).
    """

    __slots__ = ("grad", "masked")

    def __init__(self, masked: bool = False):
        self.grad = None
        # masked: the consumer can take (dy, relu_mask) and apply the mask itself (the LDS-DMA
        # dgrad epilogue does), so the BatchNorm backward never writes dres = dy * mask
        self.masked = masked

    def take(self):
        """The residual gradient: a tensor, or ``(dy, mask)`` (1 bit per element) when masked."""
        g, self.grad = self.grad, None
        if g is None:
            raise RuntimeError("GradLink: the residual gradient was not produced before its consumer ran")
        return g


class SideGradLink:
    """Like :class:`GradLink`, for a producer that autograd does NOT order before the
    consumer by data dependency: the downsample convolution of a ResNet block, whose input
    gradient is the second summand of the block input's gradient (the first is conv1's
    dgrad). Autograd runs ready nodes newest-first, so the downsample branch (created after
    the main path) normally runs first and :meth:`offer` hands its gradient over; if the
    consumer ran first, it has closed the link and the producer returns its gradient to
    autograd as usual — correct either way, never dropped or double counted."""

    __slots__ = ("grad", "closed", "delivered")

    def __init__(self):
        self.grad = None
        self.closed = False
        self.delivered = False  # the consumer added the producer's gradient (diagnostics/tests)

    def offer(self, g: torch.Tensor) -> bool:
        if self.closed:
            return False
        self.grad = g
        return True

    def take(self):
        g, self.grad, self.closed = self.grad, None, True
        self.delivered = g is not None
        return g


class BNStatsLink:
    """Lets the kernel that produces a BatchNorm's output gradient (a dgrad GEMM) accumulate
    that BatchNorm's backward reductions — sum(dy_eff), sum(dy_eff * xhat) — in its epilogue,
    so the BatchNorm backward skips its reduce pass over (dy, x).

    The BatchNorm's forward binds its saved tensors; the consumer's backward runs the
    GEMM with the BN-backward epilogue into the shared statistics workspace and sets
    ``ready``; the BatchNorm's backward then only finalizes and applies. Valid only when the
    linked consumer's dgrad output IS the whole gradient of the BatchNorm output (a single
    consumer, or the residual sum handed over through a :class:`GradLink`); otherwise the
    link stays unused and the BatchNorm reduces as usual.
    """

    __slots__ = ("x", "mask", "w32", "b32", "mean", "inv", "relu", "ready")

    def __init__(self):
        self.x = self.mask = self.w32 = self.b32 = self.mean = self.inv = None
        self.relu = False
        self.ready = False

    def bind(self, x, mask, w32, b32, mean, inv, relu):
        self.x, self.mask, self.w32, self.b32, self.mean, self.inv, self.relu = x, mask, w32, b32, mean, inv, relu
        self.ready = False

    @property
    def bound(self) -> bool:
        return self.x is not None

    @property
    def relu_mode(self) -> int:
        """0: no ReLU; 2: mask recomputed from x; 3: saved 1-bit mask."""
        return 0 if not self.relu else (3 if self.mask is not None else 2)

    def release(self):
        self.x = self.mask = self.w32 = self.b32 = self.mean = self.inv = None
        self.ready = False


def bn_counter(bn):
    """(momentum, counter) for a training-mode BatchNorm module: the ``num_batches_tracked``
    tensor the finalize kernel increments (no launch of its own), or None when nothing is
    tracked / the cumulative average (momentum None) needs the host-side count now."""
    if not (bn.training and bn.track_running_stats):
        return (0.1 if bn.momentum is None else bn.momentum), None
    if bn.momentum is None:
        bn.num_batches_tracked.add_(1)
        return 1.0 / float(bn.num_batches_tracked), None
    return bn.momentum, bn.num_batches_tracked


# ---- the launch layer: one function per BatchNorm kernel. Each owns the allocation of what it returns, the
# null pointers, the dtype code and the stream; callers pass tensors and get tensors back.

def launch_finalize(x, w32, b32, running_mean, running_var, momentum, eps, nbt, pending, ws=None, affine=False):
    """Batch statistics of ``x`` -> ``(mean, invstd)``, with ``affine`` ``(mean, invstd, scale, shift)``
    (``scale = w * invstd``, ``shift = fma(-mean, scale, b)``: what a consumer applies on load). ``pending``:
    the per-channel sums already lie in the workspace ``ws`` (default :func:`_workspace`) from the epilogue
    of the kernel that produced ``x``; else a statistics pass over ``x`` comes first. Updates the running
    statistics and increments the counter ``nbt`` where given."""
    rows, ch = _rows_c(x)
    out = [torch.empty(ch, device=x.device, dtype=torch.float32) for _ in range(4 if affine else 2)]
    mean, inv, scale, shift = out if affine else (*out, None, None)
    ws = _workspace(x) if ws is None else ws
    _ext.get(required=True).bn_stats_finalize(
        x.data_ptr(), w32.data_ptr(), b32.data_ptr(), ptr(running_mean), ptr(running_var), mean.data_ptr(),
        inv.data_ptr(), ptr(scale), ptr(shift), ws.data_ptr(), rows, ch, float(momentum), float(eps), int(pending),
        DTYPE_CODE[x.dtype], stream(x), ptr(nbt))
    return out


def launch_apply(x, w32, b32, mean, inv, relu, residual=None):
    """``(y, mask)``: y = [relu](x * scale + shift [+ residual]) from finished statistics. ReLU after a
    residual add keeps a 1-bit mask (1/16 of y's bytes) for the backward; otherwise the backward kernels
    recompute the mask from x (bit-identical to the forward) and ``mask`` is None."""
    rows, ch = _rows_c(x)
    res = nhwc(residual) if residual is not None else None
    y = torch.empty_like(x)
    mask = torch.empty(x.numel() // 8, device=x.device, dtype=torch.uint8) if (relu and res is not None) else None
    _ext.get(required=True).bn_apply(x.data_ptr(), y.data_ptr(), ptr(res), ptr(w32), ptr(b32), mean.data_ptr(),
                                     inv.data_ptr(), rows, ch, int(relu), ptr(mask), DTYPE_CODE[x.dtype], stream(x))
    return y, mask


def launch_apply_conv1x1(x, scale, shift, weight, ws=None):
    """``(y, c)``: y = relu(x * scale + shift) (bit for bit :func:`launch_apply`'s from the same statistics;
    ``scale`` / ``shift``: :func:`launch_finalize` with ``affine``) and c = conv1x1(y, weight), from one read
    of ``x`` (``csrc/kernels/bn_relu_conv1x1_fwd.hip``: bf16 NHWC, 64 -> 256 or 128 -> 512 channels). The
    per-channel sums of c are left pending in ``ws`` (default :func:`_workspace`) for the next BatchNorm."""
    n, ch, h, w = x.shape
    co = weight.shape[0]
    y = torch.empty_like(x)
    c = torch.empty(n, h, w, co, device=x.device, dtype=x.dtype).permute(0, 3, 1, 2)
    ws = _workspace(x) if ws is None else ws
    _ext.get(required=True).bn_relu_conv1x1_fwd(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), weight.data_ptr(),
                                                y.data_ptr(), c.data_ptr(), ws.data_ptr(), n * h * w, ch, co, stream(x))
    return y, c


def launch_bwd(dy, x, mask, w32, b32, mean, inv, relu, want_dres=False, stats_ready=False, params=(None, None),
               want_dx=True):
    """The fused-BN backward; returns ``(dx, dres, dw, db)``, dw / db fp32: in the bucket slices of
    ``params`` (the (weight, bias) leaves) where attached (``graddst``). ``stats_ready``: the producer of
    dy already accumulated the two reductions into the link workspace, so the reduce pass is skipped.
    ``want_dx=False``: reduce + finalize only (the finished sums land in dw / db; a later kernel forms dx)."""
    rows, ch = _rows_c(x)
    dx = torch.empty_like(x) if want_dx else None
    dres = torch.empty_like(x) if want_dres else None
    # the finalize kernel always produces both reductions (they feed dx)
    dw, db = (_grad_out(p, ch, x) for p in params)
    ws = _link_workspace(x) if stats_ready else _workspace(x)
    _ext.get(required=True).bn_bwd(dy.data_ptr(), x.data_ptr(), 0, ptr(mask), ptr(w32), ptr(b32), mean.data_ptr(),
                                   inv.data_ptr(), ptr(dx), ptr(dres), dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                   rows, ch, int(relu), DTYPE_CODE[x.dtype], stream(x), int(stats_ready))
    return dx, dres, dw, db


def launch_bwd_dual(dy, mask, c3, cds, w32, mean, inv, w232, mean2, inv2, params, want_dx=True):
    """The backward of relu(bn(c3) + bn2(cds)): one reduce pass for both BatchNorms' sums, one pass writing both
    input gradients; returns ``(dx, dx2, dw, db, dw2, db2)`` (``params``: the four leaves, as in
    :func:`launch_bwd`). ``want_dx=False``: reduce + finalize only, dx = dx2 = None."""
    rows, ch = _rows_c(c3)
    dx, dx2 = (torch.empty_like(c3), torch.empty_like(cds)) if want_dx else (None, None)
    dw, db, dw2, db2 = (_grad_out(p, ch, c3) for p in params)
    _ext.get(required=True).bn_bwd_dual(
        dy.data_ptr(), mask.data_ptr(), c3.data_ptr(), cds.data_ptr(), w32.data_ptr(), mean.data_ptr(),
        inv.data_ptr(), w232.data_ptr(), mean2.data_ptr(), inv2.data_ptr(), ptr(dx), ptr(dx2), dw.data_ptr(),
        db.data_ptr(), dw2.data_ptr(), db2.data_ptr(), _workspace(c3).data_ptr(), _dual_workspace(c3).data_ptr(), rows,
        ch, DTYPE_CODE[c3.dtype], stream(c3))
    return dx, dx2, dw, db, dw2, db2


def hands_masked(link, mask, relu) -> bool:
    """A masked GradLink takes (dy, mask) instead of dres = dy * mask: one write pass less."""
    return bool(link is not None and link.masked and relu and mask is not None and mask.dtype == torch.uint8)


def finish_bwd(dw, db, wdtype, has_w, has_b, link, dy, mask, dres, hand_masked):
    """The tail of a BatchNorm backward: ``(dw, db, dres)`` as autograd gets them: dw / db in the
    parameters' dtype (None without affine), and the residual's gradient handed to ``link`` instead
    (as ``(dy, mask)`` when ``hand_masked``)."""
    dw = (dw if wdtype == torch.float32 else dw.to(wdtype)) if has_w else None
    db = (db if wdtype == torch.float32 else db.to(wdtype)) if has_b else None
    if link is not None:
        link.grad, dres = ((dy, mask) if hand_masked else dres), None
    return dw, db, dres


class _FusedBN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, momentum, eps, relu, link=None,
                nbt=None, bnlink=None):
        x = nhwc(x)
        res = nhwc(residual) if residual is not None else None
        rows, ch = _rows_c(x)
        y = torch.empty_like(x)
        w32 = weight.float() if weight is not None else None
        b32 = bias.float() if bias is not None else None
        save_mean = torch.empty(ch, device=x.device, dtype=torch.float32)
        save_inv = torch.empty(ch, device=x.device, dtype=torch.float32)
        ws = _workspace(x)
        # ReLU after a residual add: keep a 1-bit mask (1/16 of y's bytes) for the backward
        mask = torch.empty(x.numel() // 8, device=x.device, dtype=torch.uint8) if (relu and res is not None) \
            else None
        _ext.get(required=True).bn_fwd_train(
            x.data_ptr(), y.data_ptr(), ptr(res), ptr(w32), ptr(b32), ptr(running_mean), ptr(running_var),
            save_mean.data_ptr(), save_inv.data_ptr(), ws.data_ptr(), rows, ch, float(momentum), float(eps), int(relu),
            ptr(mask), DTYPE_CODE[x.dtype], stream(x), ptr(nbt))
        ctx.relu = relu
        ctx.has_res = residual is not None
        ctx.link = link if residual is not None else None
        ctx.wdtype = weight.dtype if weight is not None else None
        ctx.has_bias = bias is not None
        ctx.params = (weight, bias)
        # Without a residual the ReLU mask is recomputed from x in the backward
        # kernels (bit-identical to the forward); with one, the 1-bit mask is used.
        # Either way y is neither saved nor re-read.
        ctx.save_for_backward(x, mask, w32, b32, save_mean, save_inv)
        ctx.bnlink = bnlink
        if bnlink is not None:
            bnlink.bind(x, mask, w32 if w32 is not None else torch.ones(ch, device=x.device),
                        b32 if b32 is not None else torch.zeros(ch, device=x.device), save_mean, save_inv, relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mask, w32, b32, save_mean, save_inv = ctx.saved_tensors
        dy = nhwc(dy)
        # the producer of dy already accumulated this BN's reductions into the workspace
        stats_ready = ctx.bnlink is not None and ctx.bnlink.ready
        hand_masked = hands_masked(ctx.link, mask, ctx.relu)
        dx, dres, dw, db = launch_bwd(dy, x, mask, w32, b32, save_mean, save_inv, ctx.relu,
                                      ctx.has_res and not hand_masked, stats_ready, ctx.params)
        if ctx.bnlink is not None:
            ctx.bnlink.release()
        dw, db, dres = finish_bwd(dw, db, ctx.wdtype, w32 is not None, ctx.has_bias, ctx.link, dy, mask, dres,
                                  hand_masked)
        return dx, dw, db, dres, None, None, None, None, None, None, None, None


def batch_norm_reference(x, weight, bias, running_mean, running_var, training, momentum, eps, relu=False,
                         residual=None):
    """PyTorch composition with the same semantics (fp32 math)."""
    y = F.batch_norm(x.float(), running_mean, running_var, weight.float() if weight is not None else None,
                     bias.float() if bias is not None else None, training, momentum, eps)
    if residual is not None:
        y = y + residual.float()
    if relu:
        y = F.relu(y)
    return y.to(x.dtype)


def fused_batch_norm(x, weight, bias, running_mean, running_var, training=True, momentum=0.1, eps=1e-5,
                     relu=False, residual=None, link: GradLink | None = None,
                     num_batches_tracked: torch.Tensor | None = None, bnlink: BNStatsLink | None = None):
    """``link``: deliver the residual's gradient through a :class:`GradLink` instead of
    returning it to autograd (training with the fused kernels only; otherwise ignored).
    ``num_batches_tracked``: counter incremented once (inside the finalize kernel)."""
    if training and kernel_supported(x):
        return _FusedBN.apply(x, weight, bias, residual, running_mean, running_var, momentum, eps, relu, link,
                              num_batches_tracked, bnlink)
    if num_batches_tracked is not None and training:
        num_batches_tracked.add_(1)
    if (not training) and kernel_supported(x) and not torch.is_grad_enabled():
        x = nhwc(x)
        rows, ch = _rows_c(x)
        y = torch.empty_like(x)
        res = nhwc(residual) if residual is not None else None
        w32 = weight.float() if weight is not None else None
        b32 = bias.float() if bias is not None else None
        _ext.get(required=True).bn_fwd_infer(x.data_ptr(), y.data_ptr(), ptr(res), ptr(w32), ptr(b32),
                                             running_mean.data_ptr(), running_var.data_ptr(), rows, ch, float(eps),
                                             int(relu), DTYPE_CODE[x.dtype], stream(x))
        return y
    return batch_norm_reference(x, weight, bias, running_mean, running_var, training, momentum, eps, relu, residual)


class FusedBatchNorm2d(nn.BatchNorm2d):
    """``nn.BatchNorm2d`` with optional fused ReLU / residual add (NHWC HIP kernels on GPU)."""

    def forward(self, x, relu: bool = False, residual: torch.Tensor | None = None, link: GradLink | None = None,
                bnlink: BNStatsLink | None = None):
        mom, nbt = bn_counter(self)
        use_batch = self.training or not self.track_running_stats
        return fused_batch_norm(x, self.weight, self.bias,
                                self.running_mean if self.track_running_stats else None,
                                self.running_var if self.track_running_stats else None,
                                use_batch, mom, self.eps, relu, residual, link, nbt, bnlink)


def __getattr__(name):
    # the synchronised variants live in ops/syncbn.py (which imports this module): exported here too
    if name in ("SyncBatchNorm2d", "convert_sync_batchnorm", "sync_batch_norm"):
        from . import syncbn
        return getattr(syncbn, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
