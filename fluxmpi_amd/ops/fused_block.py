"""Producer/consumer fusion of 1x1 convolutions with BatchNorm for bottleneck blocks.

Built on the MFMA GEMM (``csrc/kernels/gemm.hip``) and the split fused-BN
kernels (``csrc/kernels/batchnorm.hip``). Per ResNet bottleneck:

=========================  ===================================================
op                         what disappears compared with conv -> BN -> ReLU
=========================  ===================================================
``conv1x1_stats``          the BatchNorm statistics pass over the conv output
                           (sums come from the GEMM epilogue)
``bn_relu_conv1x1``        the normalised activation: BN + ReLU are applied to
                           the GEMM's A operand while staging (forward) and to
                           the wgrad B operand (backward); never written to HBM
``bn_from_stats``          (consumer of the above) finalize + normalise pass only
``GradLink``               the residual-gradient add of the block input: the
                           BN backward hands ``dres`` to the conv1 dgrad GEMM,
                           which adds it in its epilogue
``conv1x1_hybrid``         MIOpen forward/wgrad, our dgrad (+ linked residual)
=========================  ===================================================

All three are autograd Functions; activations are bf16 NHWC (channels_last),
weights bf16, BatchNorm parameters / statistics fp32. Numerics: the BN affine
applied inside the GEMM is computed exactly like the fused-BN kernels'
(``scale = w * invstd``, ``shift = fma(-mean, scale, b)``), so ReLU masks
recomputed in the backward match the forward bit for bit.
"""
from __future__ import annotations

import os

import torch

from . import _ext
from . import graddst
from ._launch import conv_backward, nhwc, stream as _stream  # noqa: F401 (_stream: imported by tests)
from .batchnorm import (BNStatsLink, GradLink, SideGradLink, _dual_workspace, _link_workspace,  # noqa: F401 (links re-exported)
                        _workspace, bn_counter, finish_bwd, hands_masked, launch_apply, launch_apply_conv1x1, launch_bwd,
                        launch_bwd_dual, launch_finalize)
from . import gemm as G
from . import gemm_nt as _NT
from . import groupnorm as _GN
from .conv_choice import (_DGRAD_CHOICE, _DS_CHOICE, _FWD1_CHOICE, _FWD_CHOICE, _FWD_ENGINE, _S2_CHOICE,  # noqa: F401
                          _WG_CHOICE, FWD_ENGINES, choices_frozen, dump_choices, freeze_choices,
                          load_choice_lines, load_choices, no_measure as _no_measure, stats_choice,
                          time_us as _time_us, w256_ok as _w256_ok, w3n_configs, wgrad_best)
from .gemm import conv1x1_dgrad, conv1x1_wgrad, conv3x3_dgrad, conv3x3_fwd, gemm, note_filter
from .multi_tensor import DTYPE_CODE


# 3x3 / stride-1 convolutions of the bottlenecks: "ours" = forward (+ the next BatchNorm's
# statistics in the epilogue) and input gradient on the implicit-GEMM MFMA kernel, weight
# gradient on MIOpen; "dgrad" = only the input gradient ours; "miopen" = all MIOpen
CONV3X3 = "ours"
# 1x1 forward of the bottlenecks: "ours" = our GEMM + statistics epilogue where measured faster
# than MIOpen + the statistics pass; "miopen" = always MIOpen
CONV1X1 = "ours"
# downsample blocks: bn3 and the downsample branch's BatchNorm as one dual kernel pair
# (relu(bn3(c3) + bn_ds(c_ds)) without materialising bn_ds(c_ds); see dual_bn_relu)
DUAL_BN = True
# downsample 1x1 forward: "ours" = our GEMM (stride 2 gathers the even pixels in the A staging)
# with the downsample BatchNorm's sums in its epilogue where measured faster than MIOpen + the
# statistics pass (dual-BN blocks only); "force" = ours wherever supported; "miopen" = always MIOpen
DS_FWD = "ours"
# weight gradients of the downsample 1x1 and the stride-2 3x3 convolutions: MIOpen vs our split-K
# kernel (stride-2 B-row gather / implicit stride-2 im2col), measured per shape
DS_WGRAD = True
# stride-2 3x3 forward: our implicit GEMM (+ statistics epilogue) where measured faster (0: MIOpen)
S2_FWD = True


def _nhwc2d(x: torch.Tensor) -> torch.Tensor:
    """[N,C,H,W] channels_last -> [N*H*W, C] view (copy if not channels_last)."""
    x = nhwc(x)
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c)


def _empty_nhwc(n, c, h, w, like):
    return torch.empty(n, h, w, c, device=like.device, dtype=like.dtype).permute(0, 3, 1, 2)


def _fwd1x1_stats(x, weight, stats):
    """c = conv1x1(x, W) (NHWC) with the output's BatchNorm sums into ``stats``: on the 256x256
    persistent kernel (``gemm_nt``, statistics epilogue) where the shape qualifies (``gemm_nt.gemm_ok``:
    enough tiles and K), else on the LDS-DMA GEMM."""
    n, ci, h, w = x.shape
    co = weight.shape[0]
    c = _empty_nhwc(n, co, h, w, x)
    x2, w2 = _nhwc2d(x), weight.reshape(co, ci)
    if G.ENGINE != 1 and _NT.gemm_ok(n * h * w, co, ci, x2, w2):
        _NT.gemm_plain(x2, w2, _nhwc2d(c), stats)
    else:
        gemm(x2, w2, c, M=n * h * w, N=co, K=ci, lda=ci, ldb=ci, ldc=co, a_kmajor=True, b_kmajor=True, mode=1,
             stats=stats)
    return c


_bn_bwd = launch_bwd  # (dy, x, mask, w32, b32, mean, inv, relu, has_res, stats_ready, params) -> (dx, dres, dw, db)


def _wgrad1x1_candidates(dc, x, weight, stride=1, ours=True):
    """The weight-gradient implementations of a 1x1 convolution that ``wgrad_best`` chooses from: MIOpen;
    with ``ours`` our split-K kernel (stride 2: B rows gathered from the even pixels) and, at stride 1
    where it takes the shape, the 256x256-tile kernel."""
    co, ci = weight.shape[0], weight.shape[1]
    impls = {"miopen": lambda: conv_backward(dc, x, weight, stride, 0, False, True)[1]}
    if ours and stride == 1:
        impls["ours"] = lambda: G.conv1x1_wgrad_v2(_nhwc2d(dc), _nhwc2d(x), out_dtype=weight.dtype).view(co, ci, 1, 1)
        if _w256_ok(co, ci, dc):
            from .linear import weight_grad
            impls["w256"] = lambda: weight_grad(_nhwc2d(dc), _nhwc2d(x), weight.dtype).view(co, ci, 1, 1)
    elif ours and stride == 2:
        impls["ours"] = lambda: G.conv1x1_wgrad_s2(_nhwc2d(dc), x, out_dtype=weight.dtype).view(co, ci, 1, 1)
    return impls


class _Conv1x1Stats(torch.autograd.Function):
    """c = conv1x1(x, W); the output's per-channel sum/sumsq go to the BN workspace."""

    @staticmethod
    def forward(ctx, x, weight, link=None, bnlink=None):
        x = nhwc(x)
        ctx.link, ctx.bnlink = link, bnlink
        note_filter(weight)
        c = _fwd1x1_stats(x, weight, _workspace(x))
        ctx.save_for_backward(x, weight)
        return c

    @staticmethod
    def backward(ctx, dc):
        x, weight = ctx.saved_tensors
        co, ci = weight.shape[0], weight.shape[1]
        dc2 = _nhwc2d(dc)
        # weight gradient first, on the side stream: it overlaps the input-gradient chain
        with graddst.into(weight):  # into the DDP bucket slice when one is attached
            dw = conv1x1_wgrad(dc2, _nhwc2d(x), out_dtype=weight.dtype).view_as(weight)
        dx = _dgrad_nhwc(dc2, weight, x, ctx.link, ctx.bnlink) if ctx.needs_input_grad[0] else None
        return dx, dw, None, None


class Stride2Grad:
    """The input gradient of a stride-2 1x1 convolution in compact form ([N, C, ceil(H/2),
    ceil(W/2)]: only the even positions of the full-resolution gradient are nonzero), as handed
    through a :class:`SideGradLink`; the consumer's dgrad epilogue adds it at even (h, w)."""

    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t

    def expand(self, shape):
        n, c, h, w = shape
        full = _empty_nhwc(n, c, h, w, self.t).zero_()
        full[:, :, ::2, ::2] = self.t
        return full


def _dgrad_nhwc(dc2, weight, x, link, bnlink=None):
    """dX (NHWC, x's shape) = dC @ W [+ the residual gradient delivered through ``link``]; with a
    bound ``bnlink`` the epilogue also accumulates the backward reductions of the BatchNorm
    that produced x (whose output gradient dX is), so that BatchNorm skips its reduce pass."""
    co, ci = weight.shape[0], weight.shape[1]
    n, _, h, w = x.shape
    dx = _empty_nhwc(n, ci, h, w, x)
    res = res_mask = res_sub = None
    if link is not None:
        g = link.take()  # SideGradLink: None if its producer has not run (it then returns its own)
        if isinstance(g, tuple):  # masked GradLink: (dy, 1-bit ReLU mask), masked in the epilogue
            res, res_mask = _nhwc2d(g[0]), g[1]
        elif isinstance(g, Stride2Grad):  # compact gradient of a stride-2 1x1 conv's input
            res, res_sub = _nhwc2d(g.t), (h, w)
        elif g is not None:
            res = _nhwc2d(g)
    bn = stats = None
    if bnlink is not None and bnlink.bound and bnlink.x.shape == x.shape and \
            bnlink.x.is_contiguous(memory_format=torch.channels_last):
        bn = (_nhwc2d(bnlink.x), bnlink.w32, bnlink.b32, bnlink.mean, bnlink.inv, bnlink.mask, bnlink.relu_mode)
        stats = _link_workspace(dx)
    conv1x1_dgrad(dc2, weight.reshape(co, ci), residual=res, out=_nhwc2d(dx), bn_bwd=bn, stats=stats, w4d=weight,
                  residual_mask=res_mask, residual_sub=res_sub)
    if bn is not None:
        bnlink.ready = True
    return dx


class _Conv1x1Hybrid(torch.autograd.Function):
    """1x1 convolution: forward and weight gradient on MIOpen (fastest there), input
    gradient on our MFMA GEMM (faster than MIOpen's on every ResNet-50 shape measured)
    with the block's residual gradient added in its epilogue (``link``)."""

    @staticmethod
    def forward(ctx, x, weight, link=None, bnlink=None, ours_stats=False, c=None):
        x = nhwc(x)
        ctx.link, ctx.bnlink = link, bnlink
        note_filter(weight)
        ctx.save_for_backward(x, weight)
        if c is not None:
            # already computed, its BatchNorm's sums pending in the workspace (bn_relu_conv3)
            return c
        if ours_stats:
            # our GEMM, the next BatchNorm's statistics accumulated in its epilogue
            return _fwd1x1_stats(x, weight, _workspace(x))
        return torch.nn.functional.conv2d(x, weight)

    @staticmethod
    def backward(ctx, dc):
        x, weight = ctx.saved_tensors
        dc = nhwc(dc)
        dw = None
        if ctx.needs_input_grad[1]:
            dw = wgrad_best(("1x1", tuple(x.shape), weight.shape[0]), _wgrad1x1_candidates(dc, x, weight), param=weight)
        dx = _dgrad_nhwc(_nhwc2d(dc), weight, x, ctx.link, ctx.bnlink) if ctx.needs_input_grad[0] else None
        return dx, dw, None, None, None, None


def _ds_fwd_ours(x, weight, stride, stats):
    """The downsample convolution on our GEMM (stride 2: A rows gathered from the even pixels,
    no strided copy), its BatchNorm's per-channel sums into ``stats``."""
    n, ci, h, w = x.shape
    co = weight.shape[0]
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    c = _empty_nhwc(n, co, ho, wo, x)
    gemm(_nhwc2d(x), weight.reshape(co, ci), c, M=n * ho * wo, N=co, K=ci, lda=ci, ldb=ci, ldc=co, mode=1,
         stats=stats, a_sub=(h, w) if stride == 2 else None)
    return c


def ds_forward_supported(x, weight, stride) -> bool:
    return (DS_FWD in ("ours", "force") and G.ENGINE != 1 and x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4
            and weight.dtype == torch.bfloat16 and stride in (1, 2) and x.shape[1] % 8 == 0
            and weight.shape[0] % 8 == 0 and x.numel() // x.shape[1] < 2 ** 31)


def ds_forward_is_ours(x, weight, stride) -> bool:
    """Per-shape choice of the downsample forward, measured once: our GEMM with the statistics
    epilogue vs MIOpen plus the statistics pass its BatchNorm then needs (one read of the output
    at 5 TB/s)."""
    if not ds_forward_supported(x, weight, stride):
        return False
    if DS_FWD == "force":
        return True
    def make():
        xs, w = x.detach().contiguous(memory_format=torch.channels_last), weight.detach()
        n, _, h, wd = x.shape
        ws = torch.zeros_like(_workspace(xs))
        return (lambda: _ds_fwd_ours(xs, w, stride, ws), lambda: torch.nn.functional.conv2d(xs, w, None, stride),
                n * ((h + stride - 1) // stride) * ((wd + stride - 1) // stride) * w.shape[0] * x.element_size())
    return stats_choice(_DS_CHOICE, (tuple(x.shape), weight.shape[0], stride), make)


class _Conv1x1Downsample(torch.autograd.Function):
    """The downsample 1x1 convolution (stride 1 or 2) of a ResNet block: forward on MIOpen, or
    (``stats``) on our GEMM with its BatchNorm's sums left pending in ``stats`` (the dual BN
    consumes them); weight gradient on MIOpen. Its input gradient (our dgrad GEMM; at stride 2
    over the output pixels only, in the compact :class:`Stride2Grad` form) is handed to the
    block's conv1 through a :class:`SideGradLink`, whose dgrad epilogue adds it: no separate add
    kernel over the block input's gradient, and at stride 2 no zero-filled full-resolution
    gradient either."""

    @staticmethod
    def forward(ctx, x, weight, stride, link, stats=None):
        x = nhwc(x)
        ctx.stride, ctx.link = stride, link
        note_filter(weight)
        ctx.save_for_backward(x, weight)
        if stats is not None:
            return _ds_fwd_ours(x, weight, stride, stats)
        return torch.nn.functional.conv2d(x, weight, None, stride)

    @staticmethod
    def backward(ctx, dc):
        x, weight = ctx.saved_tensors
        dc = nhwc(dc)
        s = ctx.stride
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = dw = None
        if s == 1 and need_x:
            dx = _dgrad_nhwc(_nhwc2d(dc), weight, x, None)
        elif s == 2 and need_x and ctx.link is not None and G.ENGINE != 1 and x.shape[1] % 8 == 0:
            # compact: the GEMM over the strided output pixels only; conv1's dgrad epilogue adds it
            # at the even positions (no zero-filled full-resolution gradient is written or read)
            n, co, ho, wo = dc.shape
            ci = weight.shape[1]
            dxc = _empty_nhwc(n, ci, ho, wo, dc)
            conv1x1_dgrad(_nhwc2d(dc), weight.reshape(co, ci), out=_nhwc2d(dxc), w4d=weight)
            if ctx.link.offer(Stride2Grad(dxc)):
                dxc = None
                need_x = False  # delivered
            else:
                dx = Stride2Grad(dxc).expand(x.shape)
        if need_w and not (need_x and dx is None):
            dw = _ds_wgrad(dc, x, weight, s)
        elif need_w or (need_x and dx is None):
            dx_m, dw = conv_backward(dc, x, weight, s, 0, need_x and dx is None, need_w)
            dx = dx if dx is not None else dx_m
        if dx is not None and ctx.link is not None and ctx.link.offer(dx):
            dx = None  # delivered to conv1's dgrad epilogue
        return dx, dw, None, None, None


def _ds_wgrad(dc, x, weight, s):
    """The downsample convolution's weight gradient: the fastest (measured once per shape) of
    MIOpen and our split-K kernel (stride 2: B rows gathered from the even pixels)."""
    co, ci = weight.shape[0], weight.shape[1]
    impls = _wgrad1x1_candidates(dc, x, weight, s, ours=bool(
        DS_WGRAD and dc.dtype == torch.bfloat16 and ci % 8 == 0 and co % 8 == 0 and G.ENGINE != 1))
    if "ours" not in impls:
        return impls["miopen"]()
    return wgrad_best(("ds", tuple(x.shape), co, s), impls, param=weight)


def conv1x1_downsample(x, weight, stride, link=None, ours_stats=False):
    """``ours_stats`` (see :func:`ds_forward_is_ours`): forward on our GEMM with the output's
    BatchNorm sums pending in the dual workspace, for ``dual_bn_relu(..., ds_stats_ready=True)``."""
    return _Conv1x1Downsample.apply(x, weight, stride, link, _dual_workspace(x) if ours_stats else None)


def _bn_fwd_from_stats(x, weight, bias, residual, running_mean, running_var, momentum, eps, relu, pending, nbt):
    """BatchNorm(+residual)(+ReLU) of a convolution's output: the finalize (``pending``: of the sums the
    convolution's epilogue left in the workspace; else after a statistics pass) and the apply pass.
    Returns y and (mask, w32, b32, mean, inv)."""
    w32, b32 = weight.float(), bias.float()
    mean, inv = launch_finalize(x, w32, b32, running_mean, running_var, momentum, eps, nbt, pending)
    y, mask = launch_apply(x, w32, b32, mean, inv, relu, residual)
    return y, (mask, w32, b32, mean, inv)


class _BNFromStats(torch.autograd.Function):
    """BatchNorm(+residual)(+ReLU) whose batch statistics are already in the workspace
    (``stats_ready``) or are computed by the stats pass here."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, momentum, eps, relu, stats_ready,
                link=None, nbt=None, bnlink=None):
        y, saved = _bn_fwd_from_stats(x, weight, bias, residual, running_mean, running_var, momentum, eps, relu,
                                      stats_ready, nbt)
        ctx.relu, ctx.has_res, ctx.wdtype = relu, residual is not None, weight.dtype
        ctx.params = (weight, bias)
        ctx.link = link if residual is not None else None
        ctx.bnlink = bnlink
        if bnlink is not None:
            bnlink.bind(x, *saved, relu)
        ctx.save_for_backward(x, *saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mask, w32, b32, mean, inv = ctx.saved_tensors
        dy = nhwc(dy)
        ready = ctx.bnlink is not None and ctx.bnlink.ready
        hand_masked = hands_masked(ctx.link, mask, ctx.relu)
        dx, dres, dw, db = launch_bwd(dy, x, mask, w32, b32, mean, inv, ctx.relu, ctx.has_res and not hand_masked,
                                      ready, ctx.params)
        if ctx.bnlink is not None:
            ctx.bnlink.release()
        dw, db, dres = finish_bwd(dw, db, ctx.wdtype, True, True, ctx.link, dy, mask, dres, hand_masked)
        return dx, dw, db, dres, None, None, None, None, None, None, None, None, None


class _BN2Conv3(torch.autograd.Function):
    """(a2, c3) = (relu(bn2(c2)), conv3(a2)) of a bottleneck from one read of c2: bn2's finalize, then one
    streaming kernel (csrc/kernels/bn_relu_conv1x1_fwd.hip) instead of the apply pass and the expansion GEMM;
    bn3's sums are left pending in the workspace as the GEMM's epilogue leaves them. a2 is bit for bit the apply
    pass's. c3 is not differentiable here: the node that consumes it (``conv1x1_hybrid``, ``_Conv3BN3``,
    ``_Conv3DsBN`` with ``c3`` given) skips its forward GEMM and owns conv3's backward through a2. The
    backward is ``_BNFromStats``'s for a ReLU without residual (the mask recomputed from c2)."""

    @staticmethod
    def forward(ctx, c2, weight, bias, running_mean, running_var, momentum, eps, stats_ready, nbt, conv_weight):
        c2 = nhwc(c2)
        w32, b32 = weight.float(), bias.float()
        mean, inv, scale, shift = launch_finalize(c2, w32, b32, running_mean, running_var, momentum, eps, nbt,
                                                  stats_ready, affine=True)
        a2, c3 = launch_apply_conv1x1(c2, scale, shift, conv_weight)
        ctx.wdtype, ctx.params = weight.dtype, (weight, bias)
        ctx.save_for_backward(c2, w32, b32, mean, inv)
        ctx.mark_non_differentiable(c3)
        # (materialised, the gradient of c3 that nobody computes is a zero fill of c3's size per backward)
        ctx.set_materialize_grads(False)
        return a2, c3

    @staticmethod
    def backward(ctx, dy, _):
        if dy is None:  # a2 took no part in what is differentiated
            return (None,) * 10
        c2, w32, b32, mean, inv = ctx.saved_tensors
        dx, _, dw, db = launch_bwd(nhwc(dy), c2, None, w32, b32, mean, inv, True, params=ctx.params)
        dw, db, _ = finish_bwd(dw, db, ctx.wdtype, True, True, None, None, None, None, False)
        return dx, dw, db, None, None, None, None, None, None, None


# bn2's apply pass and conv3's forward GEMM as one kernel in stages 1 and 2 (FLUXMPI_BN2CONV3=0: the two
# launches; profiles/bn2c3_bn2conv3.md)
BN2CONV3 = os.environ.get("FLUXMPI_BN2CONV3", "1") != "0"


def bn2conv3_ok(c2, bn, conv) -> bool:
    """:func:`bn_relu_conv3` applies: gradients recorded, bf16 NHWC, a training-mode affine fused BatchNorm, the
    1x1 expansion 64 -> 256 or 128 -> 512 where :func:`conv1x1_forward_is_ours` holds for the shape, and at
    least one 32-pixel tile per workgroup of the fullest grid measured (two per compute unit): below that
    the persistent kernel cannot fill the device and nobody has timed it against the two launches."""
    wt = conv.weight
    if not (BN2CONV3 and G.ENGINE != 1 and torch.is_grad_enabled() and c2.is_cuda and c2.dim() == 4
            and c2.dtype == torch.bfloat16 and c2.is_contiguous(memory_format=torch.channels_last)
            and wt.dtype == torch.bfloat16 and wt.is_contiguous()
            and (c2.shape[1], tuple(wt.shape)) in ((64, (256, 64, 1, 1)), (128, (512, 128, 1, 1)))
            and _fused_bn_training(bn)):
        return False
    cus = torch.cuda.get_device_properties(c2.device).multi_processor_count
    return c2.numel() // c2.shape[1] >= 32 * 2 * cus and conv1x1_forward_is_ours(c2, wt)


def bn_relu_conv3(c2, bn, conv, stats_ready=True):
    """(relu(bn(c2)), conv(relu(bn(c2)))) from one read of c2 (check :func:`bn2conv3_ok`); ``stats_ready`` as for
    :func:`bn_from_stats`. The second result goes to its consumer as ``c3=`` / ``c=``."""
    mom, nbt = bn_counter(bn)
    return _BN2Conv3.apply(c2, bn.weight, bn.bias, bn.running_mean, bn.running_var, mom, bn.eps, stats_ready, nbt,
                           conv.weight)


class _Conv3BN3(torch.autograd.Function):
    """out = relu(bn3(conv3(a2)) + residual) of a stage-1 or stage-2 identity block (1x1, 64 -> 256 or
    128 -> 512: the shape is the filter's), whose backward never materialises bn3's input gradient dx3.
    Forward: exactly the launches of ``conv1x1_hybrid(ours_stats=True)`` + ``bn_from_stats``. Backward: bn3's
    reduce + finalize (``bn_bwd`` without a dx), then one kernel (``gemm_bf16`` mode 4,
    csrc/kernels/conv3bn3_bwd.hip or conv3bn3_s2_bwd.hip) that streams (dy, c3, mask, a2) once, forms dx3
    in registers and produces d_a2 = dx3 . W and the per-workgroup partials of dW = dx3^T . a2, then the
    split-K reduce into the filter's gradient. Unfused, dx3 (the network's largest activation size) is
    written once and read twice.

    The filter gradient always comes from the one-pass kernel: there is no per-shape choice as
    ``wgrad_best`` makes for the unfused path. That is measured at ResNet-50's 56 x 56 and 28 x 28, batch 256
    only (``profiles/c3b3_conv3bn3.md``, ``profiles/c3b3s2_conv3bn3_s2.md``); for 64 -> 256
    :func:`conv3bn3_ok` admits any N, H, W, and at few pixels the kernel runs few workgroups, each loading
    the 32 KiB filter first, which nobody has timed against the unfused kernels (128 -> 512 is gated)."""

    @staticmethod
    def forward(ctx, a2, weight, bn_weight, bn_bias, residual, running_mean, running_var, momentum, eps, nbt, link,
                ours_fwd, c3=None):
        a2 = nhwc(a2)
        note_filter(weight)
        # the per-shape forward choice of conv1x1_hybrid: our GEMM with bn3's sums in its epilogue, or
        # MIOpen and the statistics pass; or c3 already computed, the sums pending (bn_relu_conv3)
        ours_fwd = ours_fwd or c3 is not None
        if c3 is None:
            c3 = _fwd1x1_stats(a2, weight, _workspace(a2)) if ours_fwd else torch.nn.functional.conv2d(a2, weight)
        y, saved = _bn_fwd_from_stats(c3, bn_weight, bn_bias, residual, running_mean, running_var, momentum, eps, True,
                                      ours_fwd, nbt)
        ctx.link, ctx.wdtype, ctx.params = link, bn_weight.dtype, (bn_weight, bn_bias)
        ctx.save_for_backward(a2, weight, c3, *saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        a2, weight, c3, mask, w32, b32, mean, inv = ctx.saved_tensors
        dy = nhwc(dy)
        n, ci, h, w = a2.shape
        # reduce + finalize only (no dx, no dres): the two finished sums land in dbw / dbb
        _, _, dbw, dbb = launch_bwd(dy, c3, mask, w32, b32, mean, inv, True, params=ctx.params, want_dx=False)
        part = torch.empty(conv3bn3_slabs(n * h * w, dy.device, weight.shape[0]), weight.shape[0], ci,
                           device=dy.device, dtype=torch.float32)
        d_a2 = _one_pass_branch(dy, mask, c3, w32, mean, inv, (dbb, dbw), a2, weight, part, _empty_nhwc(n, ci, h, w, a2))
        dw = _slabs_to_wgrad(part, weight) if ctx.needs_input_grad[1] else None
        # the residual's gradient travels as (dy, mask): conv1's dgrad epilogue applies the mask
        dbw, dbb, _ = finish_bwd(dbw, dbb, ctx.wdtype, True, True, ctx.link, dy, mask, None, True)
        return (d_a2, dw, dbw, dbb, None, None, None, None, None, None, None, None, None)


def _one_pass_branch(dy, mask, c, w32, mean, inv, sums, act, weight, part, out):
    """One branch of the one-pass backward around a BatchNorm after a 1x1 convolution (``gemm_bf16`` mode 4,
    csrc/kernels/conv3bn3_bwd.hip for 64 -> 256, conv3bn3_s2_bwd.hip for 128 -> 512): streams (dy, c, mask, act)
    once, forms the BatchNorm's input gradient in registers from its finished ``sums`` = (sum dy, sum dy xhat), writes ``out`` = d_act = dx . W and one fp32
    partial of dW = dx^T . act per workgroup into the slab set ``part`` [slabs, Cout, Cin]."""
    co, ci = weight.shape[0], weight.shape[1]
    return gemm(dy, weight, out, M=act.numel() // ci, N=ci, K=co, lda=co, ldb=ci, ldc=ci, a_kmajor=True, b_kmajor=False,
                mode=4, splits=part.shape[0], a_affine=sums, stats=part, residual=_nhwc2d(act),
                bn_bwd=(c, w32, None, mean, inv, mask, 3))


def _slabs_to_wgrad(part, weight):
    """The split-K reduce of the slab set ``part`` [slabs, Cout, Cin] into the 1x1 filter's gradient, in its DDP
    bucket slice when one is attached."""
    co, ci = weight.shape[0], weight.shape[1]
    with graddst.into(weight):
        dw = graddst.empty((co, ci), weight.dtype, part.device)
    _ext.get(required=True).gemm_splitk_reduce(part.data_ptr(), part.shape[0], co * ci, dw.data_ptr(),
                                               DTYPE_CODE[dw.dtype], _stream(part))
    return dw.view(co, ci, 1, 1)


# the one-pass conv3 -> bn3 backward of the identity blocks (FLUXMPI_CONV3BN3=0: the separate dx pass +
# input-gradient GEMM + weight-gradient kernel everywhere; 1: one pass in stage 1 (64 -> 256) only; 2, the
# default: in stage 2 (128 -> 512) as well, profiles/c3b3s2_conv3bn3_s2.md)
CONV3BN3 = int(os.environ.get("FLUXMPI_CONV3BN3", "2"))


def conv3bn3_slabs(rows: int, device, cout: int = 256) -> int:
    """Workgroups (= fp32 partial slabs) of the mode-4 kernel: one resident round, never more than the
    32-pixel tiles there are. 64 -> 256: two workgroups per compute unit; 128 -> 512 (``cout`` 512): one, its
    filter-gradient accumulator being half of a compute unit's registers."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max(1, min(-(-rows // 32), cus if cout == 512 else 2 * cus))


def _fused_bn_training(*bns) -> bool:
    """Every module is a training-mode affine fused BatchNorm with running statistics (what the nodes
    that launch its kernels themselves read from it)."""
    from .batchnorm import FusedBatchNorm2d
    return all(isinstance(m, FusedBatchNorm2d) and m.training and m.affine and m.track_running_stats for m in bns)


def conv3bn3_admits(filter_shape, pixels: int, cus: int) -> bool:
    """The shape part of :func:`conv3bn3_ok` under the ``CONV3BN3`` switch: the (256, 64, 1, 1) filter at any
    pixel count from switch value 1; the (512, 128, 1, 1) filter from value 2, and only with at least 64
    pixels per compute unit (``cus``)."""
    if tuple(filter_shape) == (256, 64, 1, 1):
        return CONV3BN3 >= 1
    if tuple(filter_shape) == (512, 128, 1, 1):
        return CONV3BN3 >= 2 and pixels >= 32 * 2 * cus
    return False


def conv3bn3_ok(a2, conv, bn, residual, link) -> bool:
    """:func:`conv3_bn3_relu` applies: bf16 NHWC, the 64 -> 256 1x1 convolution (``CONV3BN3`` >= 1) or the
    128 -> 512 one (``CONV3BN3`` >= 2), a training-mode affine fused BatchNorm, and a residual whose gradient
    travels as (dy, mask) through a masked :class:`GradLink` (or is not needed). 128 -> 512 also needs at least
    64 pixels per compute unit (the gate of :func:`bn2conv3_ok`): its kernel is one workgroup per compute unit,
    each forming the 128 KiB filter's fragments first, and nobody has timed that against the unfused kernels
    at fewer pixels."""
    wt = conv.weight
    co, ci = wt.shape[0], wt.shape[1]
    if not (G.ENGINE != 1 and a2.is_cuda and a2.dim() == 4 and a2.dtype == torch.bfloat16
            and wt.dtype == torch.bfloat16 and wt.is_contiguous()
            and a2.shape[1] == ci and a2.numel() // ci < 2 ** 31 and residual is not None
            and residual.shape == (a2.shape[0], co, a2.shape[2], a2.shape[3]) and residual.dtype == a2.dtype
            and (link.masked if link is not None else not (residual.requires_grad and torch.is_grad_enabled()))
            and _fused_bn_training(bn)):
        return False
    return conv3bn3_admits(tuple(wt.shape), a2.numel() // ci,
                           torch.cuda.get_device_properties(a2.device).multi_processor_count)


def conv3_bn3_relu(a2, conv, bn, residual, link=None, ours_fwd=True, c3=None):
    """relu(bn(conv(a2)) + residual) with the one-pass backward (check :func:`conv3bn3_ok`);
    ``ours_fwd``: :func:`conv1x1_forward_is_ours` for this shape; ``c3``: conv(a2) already computed, bn's sums
    pending in the workspace (:func:`bn_relu_conv3`)."""
    mom, nbt = bn_counter(bn)
    return _Conv3BN3.apply(a2, conv.weight, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var, mom,
                           bn.eps, nbt, link, bool(ours_fwd), c3)


def _dual_bn_fwd(c3, bn, stats_ready, cds, bn2, ds_ready):
    """The forward launches of relu(bn(c3) + bn2(cds)): two finalizes (a statistics pass first where the
    sums are not pending) and one dual apply. ``bn`` / ``bn2``: (weight, bias, running_mean, running_var,
    momentum, eps, num_batches_tracked). Returns y and (c3, cds, mask, w32, mean, inv, w232, mean2, inv2)."""
    w, b, rm, rv, mom, eps, nbt = bn
    w2, b2, rm2, rv2, mom2, eps2, nbt2 = bn2
    c3, cds = nhwc(c3), nhwc(cds)
    w32, b32, w232, b232 = w.float(), b.float(), w2.float(), b2.float()
    # bn3 first: its sums may be pending in the workspace (conv3's GEMM epilogue)
    mean, inv = launch_finalize(c3, w32, b32, rm, rv, mom, eps, nbt, stats_ready)
    # bn_ds: its sums pending in the dual workspace (the downsample GEMM's epilogue), or a stats pass
    mean2, inv2 = launch_finalize(cds, w232, b232, rm2, rv2, mom2, eps2, nbt2, ds_ready,
                                  ws=_dual_workspace(c3) if ds_ready else None)
    ch = c3.shape[1]
    y = torch.empty_like(c3)
    mask = torch.empty(c3.numel() // 8, device=c3.device, dtype=torch.uint8)
    _ext.get(required=True).bn_apply_dual(
        c3.data_ptr(), cds.data_ptr(), y.data_ptr(), w32.data_ptr(), b32.data_ptr(), mean.data_ptr(), inv.data_ptr(),
        w232.data_ptr(), b232.data_ptr(), mean2.data_ptr(), inv2.data_ptr(), c3.numel() // ch, ch, mask.data_ptr(),
        DTYPE_CODE[c3.dtype], _stream(c3))
    return y, (c3, cds, mask, w32, mean, inv, w232, mean2, inv2)


class _DualBN(torch.autograd.Function):
    """out = relu(bn3(c3) + bn_ds(c_ds)) for a ResNet downsample block, without materialising the
    downsample branch's output bn_ds(c_ds). Forward: bn3's statistics (pending from the conv3
    GEMM epilogue when ``stats_ready``, else a stats pass), bn_ds's stats pass, one apply pass
    reading (c3, c_ds). Backward: dy_eff = dy * relu_mask is the output gradient of BOTH
    BatchNorms, so one reduce pass over (dy, mask, c3, c_ds) produces both BatchNorms' sums
    and one pass writes both input gradients: versus two separate BatchNorms, the identity is
    neither written nor read forward, and dres is neither written nor read twice backward
    (~10 B/element saved on a block's largest activations)."""

    @staticmethod
    def forward(ctx, c3, w, b, rm, rv, mom, eps, nbt, stats_ready, cds, w2, b2, rm2, rv2, mom2, eps2, nbt2,
                ds_ready=False):
        y, saved = _dual_bn_fwd(c3, (w, b, rm, rv, mom, eps, nbt), stats_ready, cds,
                                (w2, b2, rm2, rv2, mom2, eps2, nbt2), ds_ready)
        ctx.wdtypes = (w.dtype, w2.dtype)
        ctx.params = (w, b, w2, b2)
        ctx.save_for_backward(*saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        c3, cds, mask, w32, mean, inv, w232, mean2, inv2 = ctx.saved_tensors
        dx, dx2, dw, db, dw2, db2 = launch_bwd_dual(nhwc(dy), mask, c3, cds, w32, mean, inv, w232, mean2, inv2,
                                                    ctx.params)
        t1, t2 = ctx.wdtypes
        return (dx, dw.to(t1), db.to(t1), None, None, None, None, None, None,
                dx2, dw2.to(t2), db2.to(t2), None, None, None, None, None, None)


def dual_bn_supported(c, bn, bn_ds) -> bool:
    """``dual_bn_relu`` applies: fused training-mode affine BatchNorms with running statistics,
    channels a power of two <= 2048 (C/8 divides the 256-lane workgroup)."""
    from .batchnorm import kernel_supported
    ch = c.shape[1]
    return (DUAL_BN and kernel_supported(c) and c.dim() == 4 and (ch & (ch - 1)) == 0
            and _fused_bn_training(bn, bn_ds))


def dual_bn_relu(c3, bn, cds, bn_ds, stats_ready=False, ds_stats_ready=False):
    """relu(bn(c3) + bn_ds(cds)) (training); ``stats_ready``: bn's sums are pending in the
    workspace from the GEMM that produced c3; ``ds_stats_ready``: bn_ds's sums are pending in the
    dual workspace (``conv1x1_downsample(..., ours_stats=True)``)."""
    mom, nbt = bn_counter(bn)
    mom2, nbt2 = bn_counter(bn_ds)
    return _DualBN.apply(c3, bn.weight, bn.bias, bn.running_mean, bn.running_var, mom, bn.eps, nbt, stats_ready,
                         cds, bn_ds.weight, bn_ds.bias, bn_ds.running_mean, bn_ds.running_var, mom2, bn_ds.eps, nbt2,
                         ds_stats_ready)


def dual_bn_ok(x, ch, bn, bn_ds) -> bool:
    """:func:`dual_bn_supported` for the output (``ch`` channels, x's dtype/device) of a
    convolution of ``x``, decided before running it."""
    return (DUAL_BN and x.is_cuda and x.dtype in (torch.bfloat16, torch.float16, torch.float32) and x.dim() == 4
            and ch % 8 == 0 and 8 <= ch <= 2048 and (ch & (ch - 1)) == 0 and _fused_bn_training(bn, bn_ds))


class _Conv3DsBN(torch.autograd.Function):
    """out = relu(bn3(conv3(a2)) + bn_ds(conv_ds(x))) of a stage-1 downsample block (both convolutions
    1x1, 64 -> 256, stride 1), whose backward materialises neither BatchNorm's input gradient. Forward:
    exactly the launches of ``conv1x1_hybrid`` + ``conv1x1_downsample`` + ``dual_bn_relu`` (each
    convolution on its per-shape choice). Backward: the dual reduce + finalize (``bn_bwd_dual`` without a
    dx), then either one kernel over both branches (``form`` 2: csrc/kernels/conv3ds_bwd.hip) or the
    identity blocks' kernel once per branch (``form`` 1: ``gemm_bf16`` mode 4 on (dy, c3, mask, a2, W3),
    then on (dy, c_ds, mask, x, W_ds)), and the two split-K reduces into the filters' gradients. The
    downsample convolution's input gradient goes to conv1's dgrad epilogue through the block's
    :class:`SideGradLink`, as ``_Conv1x1Downsample`` hands it over.

    As for ``_Conv3BN3`` the filter gradients always come from the one-pass kernel (no ``wgrad_best``
    choice), measured at ResNet-50's 56 x 56, batch 256 only (``profiles/c3ds_conv3ds.md``)."""

    @staticmethod
    def forward(ctx, a2, w3, x, wds, w, b, w2, b2, rm, rv, mom, eps, nbt, rm2, rv2, mom2, eps2, nbt2, link, ours3,
                ours_ds, form, c3=None):
        a2, x = nhwc(a2), nhwc(x)
        note_filter(w3)
        note_filter(wds)
        ours3 = ours3 or c3 is not None  # already computed, bn3's sums pending (bn_relu_conv3)
        if c3 is None:
            c3 = _fwd1x1_stats(a2, w3, _workspace(a2)) if ours3 else torch.nn.functional.conv2d(a2, w3)
        cds = _ds_fwd_ours(x, wds, 1, _dual_workspace(x)) if ours_ds else torch.nn.functional.conv2d(x, wds)
        y, saved = _dual_bn_fwd(c3, (w, b, rm, rv, mom, eps, nbt), ours3, cds, (w2, b2, rm2, rv2, mom2, eps2, nbt2),
                                ours_ds)
        ctx.link, ctx.form = link, form
        ctx.wdtypes = (w.dtype, w2.dtype)
        ctx.params = (w, b, w2, b2)
        ctx.save_for_backward(a2, w3, x, wds, *saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        a2, w3, x, wds, c3, cds, mask, w32, mean, inv, w232, mean2, inv2 = ctx.saved_tensors
        dy = nhwc(dy)
        n, ci, h, w = a2.shape
        co, rows = w3.shape[0], n * h * w
        dev = dy.device
        # reduce + finalize only (no dx, dx2): the four finished sums land in dw / db / dw2 / db2
        _, _, dw, db, dw2, db2 = launch_bwd_dual(dy, mask, c3, cds, w32, mean, inv, w232, mean2, inv2, ctx.params,
                                                 want_dx=False)
        d_a2, d_x = _empty_nhwc(n, ci, h, w, a2), _empty_nhwc(n, ci, h, w, x)
        if ctx.form == 2:
            slabs = conv3ds_slabs(rows, dev)
            part = torch.empty(2, slabs, co, ci, device=dev, dtype=torch.float32)
            _ext.get(required=True).conv3ds_bwd(
                dy.data_ptr(), mask.data_ptr(), c3.data_ptr(), cds.data_ptr(), w32.data_ptr(), mean.data_ptr(),
                inv.data_ptr(), db.data_ptr(), dw.data_ptr(), w232.data_ptr(), mean2.data_ptr(), inv2.data_ptr(),
                db2.data_ptr(), dw2.data_ptr(), a2.data_ptr(), x.data_ptr(), w3.data_ptr(), wds.data_ptr(),
                d_a2.data_ptr(), d_x.data_ptr(), part[0].data_ptr(), part[1].data_ptr(), rows, slabs, _stream(dy))
        else:
            part = torch.empty(2, conv3bn3_slabs(rows, dev), co, ci, device=dev, dtype=torch.float32)
            _one_pass_branch(dy, mask, c3, w32, mean, inv, (db, dw), a2, w3, part[0], d_a2)
            _one_pass_branch(dy, mask, cds, w232, mean2, inv2, (db2, dw2), x, wds, part[1], d_x)
        grads = [_slabs_to_wgrad(part[i], wt) if ctx.needs_input_grad[1 + 2 * i] else None
                 for i, wt in enumerate((w3, wds))]
        if ctx.link is not None and ctx.link.offer(d_x):
            d_x = None  # delivered to conv1's dgrad epilogue
        t1, t2 = ctx.wdtypes
        return (d_a2, grads[0], d_x, grads[1], dw.to(t1), db.to(t1), dw2.to(t2), db2.to(t2)) + (None,) * 15


# the one-pass backward around the dual BatchNorm of the stage-1 downsample block (FLUXMPI_CONV3DS=0:
# the dual dx pass + two input-gradient GEMMs + two weight-gradient kernels; 1, the default: the
# identity blocks' one-pass kernel once per branch; 2: one kernel over both branches,
# csrc/kernels/conv3ds_bwd.hip, 366 us against 2 x 191 us per step and no faster end to end than
# the run-to-run spread: profiles/c3ds_conv3ds.md)
CONV3DS = int(os.environ.get("FLUXMPI_CONV3DS", "1"))


def conv3ds_slabs(rows: int, device) -> int:
    """Workgroups (= fp32 partial slabs per branch) of the dual kernel: one resident round, one
    workgroup per compute unit, never more than the 32-pixel tiles there are."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max(1, min(-(-rows // 32), cus))


def conv3ds_ok(x, conv2, conv3, bn, ds_conv, bn_ds) -> bool:
    """:func:`conv3ds_bn_relu` applies to the block whose input is ``x``: bf16 NHWC, a stride-1
    conv2 (so a2 has x's pixels), both 1x1 filters 64 -> 256 and contiguous, downsample stride 1,
    training-mode affine fused BatchNorms (:func:`dual_bn_ok`), and pixels x 64 below 2^31."""
    w3, wds = conv3.weight, ds_conv.weight
    return (CONV3DS in (1, 2) and G.ENGINE != 1 and x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16
            and x.shape[1] == 64 and x.is_contiguous(memory_format=torch.channels_last)
            and x.numel() < 2 ** 31 and tuple(conv2.stride) == (1, 1) and tuple(ds_conv.stride) == (1, 1)
            and all(wt.dtype == torch.bfloat16 and tuple(wt.shape) == (256, 64, 1, 1) and wt.is_contiguous()
                    for wt in (w3, wds))
            and dual_bn_ok(x, 256, bn, bn_ds))


def conv3ds_bn_relu(a2, conv3, bn, x, ds_conv, bn_ds, link=None, ours3=True, ours_ds=True, c3=None):
    """relu(bn(conv3(a2)) + bn_ds(ds_conv(x))) with the one-pass backward (check :func:`conv3ds_ok`);
    ``ours3`` / ``ours_ds``: :func:`conv1x1_forward_is_ours` / :func:`ds_forward_is_ours` for the shapes;
    ``c3``: conv3(a2) already computed, bn's sums pending in the workspace (:func:`bn_relu_conv3`)."""
    mom, nbt = bn_counter(bn)
    mom2, nbt2 = bn_counter(bn_ds)
    return _Conv3DsBN.apply(a2, conv3.weight, x, ds_conv.weight, bn.weight, bn.bias, bn_ds.weight, bn_ds.bias,
                            bn.running_mean, bn.running_var, mom, bn.eps, nbt, bn_ds.running_mean, bn_ds.running_var,
                            mom2, bn_ds.eps, nbt2, link, bool(ours3), bool(ours_ds), CONV3DS, c3)


class _BNReluConv1x1(torch.autograd.Function):
    """c3 = conv1x1(relu(BN(c2)), W) without materialising relu(BN(c2)); c3's statistics
    go to the workspace (consumed by the next ``bn_from_stats``)."""

    @staticmethod
    def forward(ctx, c2, bn_weight, bn_bias, running_mean, running_var, weight, momentum, eps, nbt=None,
                stats_ready=False):
        c2 = nhwc(c2)
        n, ch, h, w = c2.shape
        w32, b32 = bn_weight.float(), bn_bias.float()
        mean, inv, scale, shift = launch_finalize(c2, w32, b32, running_mean, running_var, momentum, eps, nbt,
                                                  stats_ready, affine=True)
        co = weight.shape[0]
        c3 = _empty_nhwc(n, co, h, w, c2)
        gemm(_nhwc2d(c2), weight.reshape(co, ch), c3, M=n * h * w, N=co, K=ch, lda=ch, ldb=ch, ldc=co, a_kmajor=True,
             b_kmajor=True, mode=1, stats=_workspace(c2), a_affine=(scale, shift))
        ctx.bn_wdtype = bn_weight.dtype
        ctx.params = (bn_weight, bn_bias)  # the leaves: their gradients' bucket slices (graddst)
        ctx.save_for_backward(c2, w32, b32, mean, inv, scale, shift, weight)
        return c3

    @staticmethod
    def backward(ctx, dc3):
        c2, w32, b32, mean, inv, scale, shift, weight = ctx.saved_tensors
        n, ch, h, w = c2.shape
        co = weight.shape[0]
        dc3_2d = _nhwc2d(dc3)
        c2_2d = _nhwc2d(c2)
        # dW = dc3^T @ relu(bn(c2))  — the activation is rebuilt on the fly in the B-operand load
        # (side stream: overlaps the input-gradient chain below)
        with graddst.into(weight):
            dw = conv1x1_wgrad(dc3_2d, c2_2d, in_affine=(scale, shift), out_dtype=weight.dtype).view_as(weight)
        # d(relu(bn(c2))) = dc3 @ W with the BN-backward reductions (ReLU mask recomputed from c2)
        # accumulated in the same GEMM's epilogue, then the BN backward without its reduce pass
        # (w4d: the LDS-DMA kernel on the cached W^T, whose epilogue has the BN-backward reductions)
        da = conv1x1_dgrad(dc3_2d, weight.reshape(co, ch), bn_bwd=(c2_2d, w32, b32, mean, inv, None, 2),
                           stats=_link_workspace(c2), w4d=weight).view(n, h, w, ch).permute(0, 3, 1, 2)
        dc2, _, dbw, dbb = launch_bwd(da, c2, None, w32, b32, mean, inv, True, stats_ready=True, params=ctx.params)
        return dc2, dbw.to(ctx.bn_wdtype), dbb.to(ctx.bn_wdtype), None, None, dw, None, None, None, None


class _Conv3x3(torch.autograd.Function):
    """3x3 / stride 1 / pad 1 convolution: implicit-GEMM forward (optionally with the next
    BatchNorm's statistics accumulated in its epilogue) and input gradient on the LDS-DMA
    MFMA kernel; weight gradient on MIOpen."""

    @staticmethod
    def forward(ctx, x, weight, fwd_ours, with_stats, bnlink=None, gradlink=None):
        x = nhwc(x)
        ctx.bnlink = bnlink
        ctx.gradlink = gradlink
        note_filter(weight)
        if fwd_ours:
            y = conv3x3_fwd(x, weight, stats=_workspace(x) if with_stats else None,
                            engine=_FWD_ENGINE.get((tuple(x.shape), weight.shape[0])))
        else:
            y = torch.nn.functional.conv2d(x, weight, None, 1, 1)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = nhwc(dy)
        dw = None
        # (inside groupnorm.skip_param_grads — the DEQ adjoint's VJPs w.r.t. activations only — the
        # filter gradient is not wanted although needs_input_grad, fixed at forward time, says so)
        if ctx.needs_input_grad[1] and not _GN._SKIP_PARAM_GRADS:
            impls = {"miopen": lambda: conv_backward(dy, x, weight, 1, 1, False, True)[1],
                     "ours": lambda: G.conv3x3_wgrad(dy, x)}
            if x.dtype == torch.bfloat16 and G.wgrad3x3n_ok(tuple(x.shape), weight.shape[0]):
                impls["w3n"] = lambda cfg: G.conv3x3_wgrad_n(dy, x, *cfg)  # narrow channels: rows staged once
                impls["w3n_cfgs"] = w3n_configs(x.shape[1])
            dw = wgrad_best(("3x3", tuple(x.shape), weight.shape[0]), impls, param=weight)
        dx = None
        if ctx.needs_input_grad[0]:
            bl = ctx.bnlink
            bn = stats = None
            if bl is not None and bl.bound and bl.x.shape == x.shape and \
                    bl.x.is_contiguous(memory_format=torch.channels_last) and G.ENGINE != 1:
                # the epilogue reduces the backward statistics of the BatchNorm that produced x
                bn = (_nhwc2d(bl.x), bl.w32, bl.b32, bl.mean, bl.inv, bl.mask, bl.relu_mode)
                stats = _link_workspace(x)
            # gradlink: x's other consumer deposited its gradient of x (GroupNorm / BatchNorm backward
            # ran first: autograd orders it by data dependency); added in the dgrad epilogue
            res = ctx.gradlink.take() if ctx.gradlink is not None else None
            if bn is None and not _dgrad_is_ours(dy, weight, x.shape):
                dx = conv_backward(dy, x, weight, 1, 1, True, False)[0]
                if res is not None:
                    dx = dx + res
            elif res is not None and bn is not None:
                dx = conv3x3_dgrad(dy, weight, bn_bwd=bn, stats=stats) + res
            else:
                dx = conv3x3_dgrad(dy, weight, bn_bwd=bn, stats=stats, residual=res)
            if bn is not None:
                bl.ready = True
        elif ctx.gradlink is not None:
            ctx.gradlink.grad = None
        return dx, dw, None, None, None, None


def _dgrad_is_ours(dy, weight, x_shape) -> bool:
    """Input gradient on our implicit GEMM, or MIOpen. Channel counts that are multiples of 32
    (ResNet-50) always take ours; narrower ones (e.g. the 48-channel DEQ cell, whose K tiles
    straddle filter taps) are measured once per shape, like the forward."""
    if weight.shape[0] % 32 == 0:
        return True
    key = (tuple(x_shape), weight.shape[0])
    hit = _DGRAD_CHOICE.get(key)
    if hit is not None:
        return hit
    if _no_measure():
        return True
    with torch.no_grad():
        d = dy.detach()
        w = weight.detach()
        xe = torch.empty(x_shape, device=dy.device, dtype=dy.dtype).contiguous(memory_format=torch.channels_last)
        ours = _time_us(lambda: conv3x3_dgrad(d, w))
        theirs = _time_us(lambda: conv_backward(d, xe, w, 1, 1, True, False))
    _DGRAD_CHOICE[key] = ours <= theirs
    return _DGRAD_CHOICE[key]


class _Conv3x3S2(torch.autograd.Function):
    """3x3 / stride 2 / pad 1 convolution (the first conv2 of ResNet stages 2-4). Forward: MIOpen,
    or (``with_stats``) our implicit GEMM over the output pixels with the next BatchNorm's sums in
    its epilogue; input gradient on the four parity-class implicit GEMMs (``gemm.conv3x3_s2_dgrad``,
    even input sizes; MIOpen otherwise); weight gradient measured per shape between MIOpen and
    our split-K kernel over the stride-2 implicit im2col (``gemm.conv3x3_wgrad_s2``)."""

    @staticmethod
    def forward(ctx, x, weight, with_stats=False):
        x = nhwc(x)
        ctx.save_for_backward(x, weight)
        if G.S2_DGRAD:
            note_filter(weight)  # the input gradient reads the batched transposed-filter cache
        if with_stats:
            return G.conv3x3_s2_fwd(x, weight, stats=_workspace(x))
        return torch.nn.functional.conv2d(x, weight, None, 2, 1)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = nhwc(dy)
        dx = dw = None
        if ctx.needs_input_grad[1]:
            dw = wgrad_best(("3x3s2", tuple(x.shape), weight.shape[0]), {
                "miopen": lambda: conv_backward(dy, x, weight, 2, 1, False, True)[1],
                "ours": lambda: G.conv3x3_wgrad_s2(dy, x)}, param=weight)
        if ctx.needs_input_grad[0]:
            if G.s2_dgrad_ok(dy, weight, x.shape):
                dx = G.conv3x3_s2_dgrad(dy, weight, x.shape)  # four parity-class implicit GEMMs
            else:
                dx = conv_backward(dy, x, weight, 2, 1, True, False)[0]
        return dx, dw, None


def _conv3x3_geometry_ok(x: torch.Tensor, conv: torch.nn.Conv2d, stride: int) -> bool:
    """What our 3x3 kernels of either stride take: a bf16 GPU batch, a plain 3x3 / pad 1 convolution of that
    stride without bias, channel counts that are multiples of 8, pixels below 2^31."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4
            and conv.kernel_size == (3, 3) and conv.stride == (stride, stride) and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None
            and conv.in_channels % 8 == 0 and conv.out_channels % 8 == 0 and conv.weight.dtype == torch.bfloat16
            and x.numel() // x.shape[1] < 2 ** 31)


def conv3x3_s2_supported(x: torch.Tensor, conv: torch.nn.Conv2d) -> bool:
    return DS_WGRAD and G.ENGINE != 1 and _conv3x3_geometry_ok(x, conv, 2)


def conv3x3_s2_forward_is_ours(x, weight) -> bool:
    """Per-shape choice of the stride-2 3x3 forward, measured once: our implicit GEMM with the
    statistics epilogue vs MIOpen plus the statistics pass (one read of the output at 5 TB/s)."""
    if CONV3X3 != "ours" or not S2_FWD or x.shape[1] % 32 != 0:
        return False
    def make():
        xs, w = x.detach().contiguous(memory_format=torch.channels_last), weight.detach()
        n, _, h, wd = x.shape
        ws = torch.zeros_like(_workspace(xs))
        return (lambda: G.conv3x3_s2_fwd(xs, w, stats=ws), lambda: torch.nn.functional.conv2d(xs, w, None, 2, 1),
                n * ((h + 1) // 2) * ((wd + 1) // 2) * w.shape[0] * x.element_size())
    return stats_choice(_S2_CHOICE, (tuple(x.shape), weight.shape[0]), make)


def conv3x3_s2(x, weight, with_stats=False):
    """``with_stats``: our forward, the output's BatchNorm sums pending in the workspace (consume
    with ``bn_from_stats(..., stats_ready=True)``); decide with :func:`conv3x3_s2_forward_is_ours`."""
    return _Conv3x3S2.apply(x, weight, with_stats)


def conv3x3_supported(x: torch.Tensor, conv: torch.nn.Conv2d) -> bool:
    return CONV3X3 in ("ours", "dgrad") and _conv3x3_geometry_ok(x, conv, 1)


def conv3x3_forward_is_ours(x, weight) -> bool:
    """Per-shape choice of the 3x3 forward, measured once (like cudnn.benchmark): our implicit
    GEMM with the statistics epilogue vs MIOpen plus the separate statistics pass it then needs
    (priced at one read of the output at 5 TB/s). Wave quantization makes some shapes (e.g.
    ResNet-50's 14x14x256 at batch 256: 1.5 rounds of 128x128 tiles) slower on our kernel."""
    if CONV3X3 != "ours":
        return False
    key = (tuple(x.shape), weight.shape[0])
    hit = _FWD_CHOICE.get(key)
    if hit is not None:
        return hit
    if _no_measure():
        return True
    with torch.no_grad():
        xs = x.detach().contiguous(memory_format=torch.channels_last)
        w = weight.detach()
        ws = torch.zeros_like(_workspace(xs))
        # our tile configurations: the default 128x128 and the 256x128 ones (fewer, larger tiles:
        # less wave quantization on e.g. 14x14x256, 1.5 rounds of 128x128 tiles)
        best = None
        for eng in (FWD_ENGINES if G.ENGINE == 0 else (0,)):
            t = _time_us(lambda: conv3x3_fwd(xs, w, stats=ws, engine=eng))
            if best is None or t < best[0]:
                best = (t, eng)
        theirs = _time_us(lambda: torch.nn.functional.conv2d(xs, w, None, 1, 1))
    n, _, h, wd = x.shape
    stats_pass_us = n * h * wd * weight.shape[0] * x.element_size() / 5e12 * 1e6
    choice = best[0] <= theirs + stats_pass_us
    _FWD_CHOICE[key] = choice
    _FWD_ENGINE[key] = best[1]
    return choice


def conv3x3(x, weight, with_stats=False, bnlink=None, gradlink=None):
    """Returns the conv output. If the forward runs on our kernel (:func:`conv3x3_forward_is_ours`)
    and ``with_stats``, its per-channel sum / sumsq are pending in the BatchNorm workspace
    (consume them with ``bn_from_stats(..., stats_ready=True)``); check with
    ``conv3x3_forward_is_ours`` first. ``gradlink`` (:class:`GradLink`): x's other consumer
    deposits its gradient of x there; the input gradient adds it in the dgrad epilogue."""
    ours = conv3x3_forward_is_ours(x, weight)
    return _Conv3x3.apply(x, weight, ours, with_stats and ours, bnlink, gradlink)


def conv3x3_fwd_raw(x, weight):
    """The 3x3 / s1 forward the autograd path would run (per-shape choice), without autograd."""
    x = nhwc(x)
    # a forward marks the cached transposed filter stale whichever kernel runs (as _Conv3x3 does):
    # the next input gradient re-derives it from the current weights
    note_filter(weight)
    if conv3x3_forward_is_ours(x, weight):
        return conv3x3_fwd(x, weight, engine=_FWD_ENGINE.get((tuple(x.shape), weight.shape[0])))
    return torch.nn.functional.conv2d(x, weight, None, 1, 1)


def conv3x3_dgrad_raw(dy, weight, x_shape, residual=None):
    """The 3x3 / s1 input gradient (+ ``residual`` in the epilogue) per the per-shape choice,
    without autograd."""
    dy = nhwc(dy)
    if _dgrad_is_ours(dy, weight, x_shape):
        return conv3x3_dgrad(dy, weight, residual=residual)
    xe = torch.empty(x_shape, device=dy.device, dtype=dy.dtype).contiguous(memory_format=torch.channels_last)
    dx = conv_backward(dy, xe, weight, 1, 1, True, False)[0]
    return dx + residual if residual is not None else dx


def masked_links_ok() -> bool:
    """GradLinks may carry (dy, mask) instead of dres: the LDS-DMA dgrad kernel masks in its epilogue."""
    return G.ENGINE != 1


def conv1x1_stats(x, weight, link=None, bnlink=None):
    return _Conv1x1Stats.apply(x, weight, link, bnlink)


def conv1x1_forward_is_ours(x, weight) -> bool:
    """Per-shape choice of a 1x1 forward, measured once: our GEMM with the statistics epilogue
    vs MIOpen plus the statistics pass the next BatchNorm then needs (one read of the output
    at 5 TB/s)."""
    if CONV1X1 != "ours":
        return False
    def make():
        xs, w = x.detach().contiguous(memory_format=torch.channels_last), weight.detach()
        n, _, h, wd = xs.shape
        ws = torch.zeros_like(_workspace(xs))
        return (lambda: _fwd1x1_stats(xs, w, ws), lambda: torch.nn.functional.conv2d(xs, w),
                n * h * wd * w.shape[0] * xs.element_size())
    return stats_choice(_FWD1_CHOICE, (tuple(x.shape), weight.shape[0]), make)


def conv1x1_hybrid(x, weight, link=None, bnlink=None, ours_stats=False, c=None):
    """``ours_stats``: forward on our GEMM with the next BatchNorm's statistics left pending in
    the workspace (``bn_from_stats(..., stats_ready=True)``); else MIOpen's forward. ``c``: the output already
    computed, the statistics pending (:func:`bn_relu_conv3`): no forward launch, the backward as ever."""
    return _Conv1x1Hybrid.apply(x, weight, link, bnlink, ours_stats, c)


def bn_from_stats(x, bn, relu=False, residual=None, stats_ready=True, link=None, bnlink=None):
    mom, nbt = bn_counter(bn)
    return _BNFromStats.apply(x, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var, mom, bn.eps, relu,
                              stats_ready, link, nbt, bnlink)


def bn_relu_conv1x1(c2, bn, weight, stats_ready=False):
    """conv1x1(relu(bn(c2)), W) with the BatchNorm + ReLU applied in the GEMM's A load (``stats_ready``:
    c2's sums are pending in the workspace from the GEMM that produced it)."""
    mom, nbt = bn_counter(bn)
    return _BNReluConv1x1.apply(c2, bn.weight, bn.bias, bn.running_mean, bn.running_var, weight, mom, bn.eps, nbt,
                                stats_ready)


def supported(x: torch.Tensor, *channels: int) -> bool:
    """Shapes the fused path handles (bf16 NHWC on GPU, channels % 32 == 0, <= 2048)."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4
            and all(c % 32 == 0 and 32 <= c <= 2048 for c in channels))
