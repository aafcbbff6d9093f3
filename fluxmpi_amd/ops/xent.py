"""Fused softmax cross-entropy: loss, gradient and top-k counts on the device (``csrc/kernels/xent.hip``).

``softmax_cross_entropy(logits, target)`` replaces ``F.cross_entropy(logits.float(), target)`` on a
classifier head: the bf16 / fp16 / fp32 logits are read as they are (fp32 arithmetic), the gradient
is written once in the logits' dtype with the incoming gradient (the loss scale) applied, and a
:class:`ClassificationMeter` accumulates the loss and the top-k counts on the device without a host
read. Per row, with ``m = max x``, ``s = sum exp(x - m)`` and ``lse = m + log s``::

    loss_row = W * lse - d                      dx = (softmax(x) * W - t) * gs
    rank     = #{j : x_j > x_y} + #{j < y : x_j == x_y}      (top-k hit: rank < k)

and the target forms

* hard: integer labels ``y``, smoothing ``eps``: ``d = (1 - eps) x_y + eps mean(x)``, ``W = 1``;
* mixed: labels, the partner of row ``b`` is row ``B - 1 - b`` (:class:`DeviceAugment`'s rule),
  ``lam`` a float or a 0-dim fp32 device tensor, ``rest = fl32(1 - lam)`` as
  :func:`..augment.mix_targets` forms it: ``d = (1 - eps)(lam x_y + rest x_yp) + (lam + rest) eps
  mean(x)``, ``W = lam + rest``; no dense target exists on this path;
* dense: ``t [B, C]`` (fp32 / bf16 / fp16), ``t' = t (1 - eps) + eps / C`` (torch's rule): ``d = sum
  t' x``, ``W = sum t'``; rows need not sum to 1; no gradient flows to the target.

GPU tensors run the kernels (mandatory there), CPU tensors :func:`xent_reference` in fp32.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch
import torch.nn as nn

from . import _ext
from ._launch import ptr as _p, stream as _stream
from .multi_tensor import DTYPE_CODE

OP = "softmax_cross_entropy"
MODE_HARD, MODE_MIXED, MODE_DENSE = 0, 1, 2
REDUCTIONS = {"mean": 0, "sum": 1, "none": 2}
_FLOATS = (torch.bfloat16, torch.float16, torch.float32)
_LABEL_CODE = {torch.int32: 2, torch.int64: 4}
METER_WORDS = 8  # 32-bit words: {fp64 sum of the row losses, int64 rows, int64 correct@k0, int64 correct@k1}


class MixedLabels(NamedTuple):
    """The targets of a mixed batch without the dense matrix: row ``b`` is ``lam`` of ``labels[b]`` and
    ``1 - lam`` of ``labels[B - 1 - b]``, smoothed by ``label_smoothing``. ``lam``: a float, or a 0-dim
    fp32 tensor on the labels' device (then nothing is read on the host)."""
    labels: torch.Tensor
    lam: object = 1.0
    label_smoothing: float = 0.0


class _Spec(NamedTuple):
    mode: int
    labels: torch.Tensor | None
    dense: torch.Tensor | None
    lam: object
    eps: float


def _is_labels(t) -> bool:
    return isinstance(t, torch.Tensor) and t.dtype in _LABEL_CODE


def _parse(op: str, logits, target, label_smoothing, lam, labels, wide_ok: bool = False) -> _Spec:
    if not isinstance(logits, torch.Tensor):
        raise TypeError(f"{op}: the logits are a torch tensor, got {type(logits).__name__}")
    if logits.dim() != 2:
        raise ValueError(f"{op}: the logits are [B, C], got {tuple(logits.shape)}")
    if logits.dtype not in _FLOATS and not (wide_ok and logits.dtype == torch.float64):
        raise TypeError(f"{op}: the logits are bf16, fp16 or fp32, got {logits.dtype}")
    B, C = logits.shape
    if C < 1:
        raise ValueError(f"{op}: need at least one class, got {tuple(logits.shape)}")
    if isinstance(target, MixedLabels):
        if lam is not None or labels is not None:
            raise ValueError(f"{op}: a MixedLabels target carries its own lam and labels")
        if float(label_smoothing) != 0.0 and float(label_smoothing) != float(target.label_smoothing):
            raise ValueError(f"{op}: label_smoothing={label_smoothing} contradicts the MixedLabels target's "
                             f"{target.label_smoothing}")
        target, lam, label_smoothing = target.labels, target.lam, target.label_smoothing
        if lam is None:
            raise ValueError(f"{op}: a MixedLabels target needs lam")
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"{op}: label_smoothing must lie in [0, 1), got {label_smoothing}")
    if not isinstance(target, torch.Tensor):
        raise TypeError(f"{op}: the target is integer labels [B], a dense [B, C] tensor or MixedLabels, got "
                        f"{type(target).__name__}")
    if target.device != logits.device:
        raise ValueError(f"{op}: the target lives on {target.device}, the logits on {logits.device}")

    def check_labels(y, what):
        if not _is_labels(y):
            raise TypeError(f"{op}: {what} are int32 or int64, got {getattr(y, 'dtype', type(y).__name__)}")
        if y.shape != (B,):
            raise ValueError(f"{op}: {what} have shape [{B}], got {tuple(y.shape)}")
        if y.device != logits.device:
            raise ValueError(f"{op}: {what} live on {y.device}, the logits on {logits.device}")
        return y.contiguous()

    if _is_labels(target):
        if labels is not None:
            raise ValueError(f"{op}: labels= goes with a dense target only")
        y = check_labels(target, "the labels")
        if lam is None:
            return _Spec(MODE_HARD, y, None, None, eps)
        if isinstance(lam, torch.Tensor):
            if lam.dim() != 0 or lam.dtype != torch.float32 or lam.device != logits.device:
                raise ValueError(f"{op}: a tensor lam is a 0-dim fp32 tensor on the logits' device")
        else:
            lam = float(lam)
            if not math.isfinite(lam):
                raise ValueError(f"{op}: lam must be finite, got {lam}")
        return _Spec(MODE_MIXED, y, None, lam, eps)
    if not target.is_floating_point():
        raise TypeError(f"{op}: the target is integer labels [B] or a float [B, C] tensor, got {target.dtype}")
    if target.shape != (B, C):
        raise ValueError(f"{op}: a dense target has the logits' shape {(B, C)}, got {tuple(target.shape)}")
    if target.dtype not in _FLOATS and not (wide_ok and target.dtype == torch.float64):
        raise TypeError(f"{op}: a dense target is fp32, bf16 or fp16, got {target.dtype}")
    if lam is not None:
        raise ValueError(f"{op}: lam goes with integer labels, not with a dense target")
    y = check_labels(labels, "labels=") if labels is not None else None
    return _Spec(MODE_DENSE, y, target.detach().contiguous(), None, eps)


def _lam_pair(lam, device, dtype):
    """``(lam, rest)`` as 0-dim tensors of ``dtype``: the fp32 values ``lam32`` and ``fl32(1 - lam32)``."""
    if isinstance(lam, torch.Tensor):
        l32 = lam.detach().to(torch.float32)
        return l32.to(dtype), (1.0 - l32).to(dtype)
    l32 = np.float32(lam)
    return (torch.tensor(float(l32), dtype=dtype, device=device),
            torch.tensor(float(np.float32(1.0) - l32), dtype=dtype, device=device))


def _formulas(x, spec: _Spec, dtype):
    """``(loss_row, t, W, p)`` of the module docstring's formulas evaluated in ``dtype``; ``t`` the dense
    form of the target, ``W`` its row weight ``[B, 1]``, ``p`` the softmax."""
    B, C = x.shape
    xs = x.detach().to(dtype)
    eps = spec.eps
    m = xs.max(dim=1, keepdim=True).values if B else xs.new_zeros(0, 1)
    e = torch.exp(xs - m)
    s = e.sum(dim=1, keepdim=True)
    lse = (m + torch.log(s)).squeeze(1)
    mean = xs.sum(dim=1) / C
    if spec.mode == MODE_DENSE:
        t = spec.dense.to(dtype) * (1.0 - eps) + eps / C
        d = (t * xs).sum(dim=1)
        W = t.sum(dim=1)
    else:
        y = spec.labels.long()
        onehot = torch.zeros(B, C, dtype=dtype, device=x.device).scatter_(1, y.unsqueeze(1), 1.0)
        xy = xs.gather(1, y.unsqueeze(1)).squeeze(1)
        if spec.mode == MODE_MIXED:
            lam, rest = _lam_pair(spec.lam, x.device, dtype)
            W = (lam + rest).expand(B)
            xp = xs.gather(1, y.flip(0).unsqueeze(1)).squeeze(1)  # the partner's label in the row's own logits
            d = (1.0 - eps) * (lam * xy + rest * xp) + W * (eps * mean)
            t = (1.0 - eps) * (lam * onehot + rest * onehot.flip(0)) + W.unsqueeze(1) * (eps / C)
        else:
            W = torch.ones(B, dtype=dtype, device=x.device)
            d = (1.0 - eps) * xy + eps * mean
            t = (1.0 - eps) * onehot + eps / C
    return W * lse - d, t, W.unsqueeze(1), e / s


def _rank(x, labels):
    """The number of classes that beat the label, on the stored values: greater, or equal at a lower index."""
    y = labels.long().unsqueeze(1)
    xy = x.gather(1, y)
    idx = torch.arange(x.shape[1], device=x.device).unsqueeze(0)
    return ((x > xy) | ((x == xy) & (idx < y))).sum(dim=1).to(torch.int32)


def _check_range(op, spec: _Spec, C: int) -> None:
    if spec.labels is not None and spec.labels.numel():
        lo, hi = int(spec.labels.min()), int(spec.labels.max())
        if lo < 0 or hi >= C:
            raise ValueError(f"{op}: labels must lie in [0, {C}), got [{lo}, {hi}]")


def xent_reference(logits, target, *, label_smoothing=0.0, reduction="mean", lam=None, labels=None,
                   dtype=torch.float64):
    """The formulas of the module docstring in plain torch, evaluated in ``dtype`` (the kernels' oracle):
    ``(loss, loss_row, dlogits for an incoming gradient of 1, rank)``; ``rank`` is ``None`` when a dense
    target comes without ``labels=``. Labels are range-checked here."""
    op = "xent_reference"
    if reduction not in REDUCTIONS:
        raise ValueError(f"{op}: reduction is 'mean', 'sum' or 'none', got {reduction!r}")
    spec = _parse(op, logits, target, label_smoothing, lam, labels, wide_ok=True)
    B, C = logits.shape
    _check_range(op, spec, C)
    loss_row, t, W, p = _formulas(logits, spec, dtype)
    gs = 1.0 / B if (reduction == "mean" and B) else 1.0
    dx = (p * W - t) * gs
    if reduction == "mean":
        loss = loss_row.sum() / B if B else loss_row.new_full((), float("nan"))
    elif reduction == "sum":
        loss = loss_row.sum()
    else:
        loss = loss_row
    rank = _rank(logits.detach(), spec.labels) if spec.labels is not None else None
    return loss, loss_row, dx, rank


# ---- the device launches --------------------------------------------------------------------------

def _lam_args(spec: _Spec):
    if isinstance(spec.lam, torch.Tensor):
        return 1.0, spec.lam.data_ptr()
    return (1.0 if spec.lam is None else float(spec.lam)), 0


def _target_args(spec: _Spec):
    return (_p(spec.labels), _p(spec.dense), _LABEL_CODE[spec.labels.dtype] if spec.labels is not None else 0,
            DTYPE_CODE[spec.dense.dtype] if spec.dense is not None else 0)


def _fwd_gpu(x, spec: _Spec, want_rank: bool):
    X = _ext.xent()
    B, C = x.shape
    stats = torch.empty(3, B, device=x.device, dtype=torch.float32)  # loss_row, m, s
    rank = torch.empty(B, device=x.device, dtype=torch.int32) if want_rank else None
    lp, dp, lcode, tcode = _target_args(spec)
    lam, dev_lam = _lam_args(spec)
    X.xent_fwd(x.data_ptr(), lp, dp, stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(), _p(rank), B, C,
               DTYPE_CODE[x.dtype], lcode, tcode, spec.mode, spec.eps, lam, dev_lam, _stream(x))
    return stats[0], stats[1], stats[2], rank


def _bwd_gpu(x, spec: _Spec, m, s, g, reduction: int):
    X = _ext.xent()
    B, C = x.shape
    dx = torch.empty_like(x)
    lp, dp, lcode, tcode = _target_args(spec)
    lam, dev_lam = _lam_args(spec)
    X.xent_bwd(x.data_ptr(), lp, dp, m.data_ptr(), s.data_ptr(), g.data_ptr(), dx.data_ptr(), B, C,
               DTYPE_CODE[x.dtype], lcode, tcode, spec.mode, reduction, spec.eps, lam, dev_lam, _stream(x))
    return dx


class _XentFn(torch.autograd.Function):
    """``(loss, rank)``; ``rank`` is an empty tensor when not asked for."""

    @staticmethod
    def forward(ctx, logits, spec: _Spec, reduction: str, meter, want_rank: bool):
        x = logits.detach().contiguous()
        B, C = x.shape
        red = REDUCTIONS[reduction]
        ctx.spec, ctx.red, ctx.shape, ctx.xdtype = spec, red, (B, C), x.dtype
        want_rank = want_rank or meter is not None
        if B == 0:  # nothing to launch: torch's values
            loss = (x.new_full((), float("nan"), dtype=torch.float32) if red == 0 else
                    x.new_zeros((), dtype=torch.float32) if red == 1 else x.new_zeros(0, dtype=torch.float32))
            rank = torch.empty(0, dtype=torch.int32, device=x.device)
            ctx.mark_non_differentiable(rank)
            return loss, rank
        if x.is_cuda:
            loss_row, m, s, rank = _fwd_gpu(x, spec, want_rank)
            if red == 2:
                loss = loss_row
            else:
                loss = torch.empty((), device=x.device, dtype=torch.float32)
            if red != 2 or meter is not None:
                k0, k1 = meter.topk if meter is not None else (1, 1)
                _ext.xent().xent_finish(loss_row.data_ptr(), _p(rank), loss.data_ptr() if red != 2 else 0,
                                        meter._block_on(x.device).data_ptr() if meter is not None else 0, B,
                                        min(red, 1), k0, k1, _stream(x))
            ctx.save_for_backward(x, m, s)
        else:
            _check_range(OP, spec, C)
            loss_row, t, W, p = _formulas(x, spec, torch.float32)
            rank = _rank(x, spec.labels) if want_rank else None
            loss = loss_row if red == 2 else (loss_row.sum() / B if red == 0 else loss_row.sum())
            if meter is not None:
                meter._add_host(loss_row, rank)
            ctx.save_for_backward(x, p * W - t)
        if rank is None:
            rank = torch.empty(0, dtype=torch.int32, device=x.device)
        ctx.mark_non_differentiable(rank)
        return loss, rank

    @staticmethod
    def backward(ctx, g, _g_rank):
        B, C = ctx.shape
        if B == 0:
            return g.new_zeros((0, C), dtype=ctx.xdtype), None, None, None, None
        if ctx.red == 2:
            g = g.expand(B)
        g = g.to(torch.float32).contiguous()  # read on the device: never on the host
        x = ctx.saved_tensors[0]
        if x.is_cuda:
            _, m, s = ctx.saved_tensors
            return _bwd_gpu(x, ctx.spec, m, s, g, ctx.red), None, None, None, None
        _, pt = ctx.saved_tensors
        gs = g.unsqueeze(1) if ctx.red == 2 else (g / B if ctx.red == 0 else g)
        return (pt * gs).to(x.dtype), None, None, None, None


def softmax_cross_entropy(logits, target, *, label_smoothing=0.0, reduction="mean", lam=None, labels=None, meter=None,
                          return_rank=False):
    """Softmax cross-entropy of ``logits [B, C]`` (bf16 / fp16 / fp32) against ``target``: integer labels
    ``[B]`` (int32 / int64), a dense float ``[B, C]`` tensor, or :class:`MixedLabels`. ``lam`` (a float or
    a 0-dim fp32 device tensor) together with integer labels selects the mixed form. Returns the fp32
    loss, 0-dim for ``"mean"`` / ``"sum"`` and ``[B]`` for ``"none"``; with ``return_rank=True``
    ``(loss, rank)``, ``rank`` int32 ``[B]`` (module docstring). ``meter``: a
    :class:`ClassificationMeter` that takes the batch in (no host read). ``labels=``: the labels of a
    dense target, for ``return_rank`` and ``meter``.

    The gradient reaches the logits only, in their dtype, rounded once, with the incoming gradient
    (read on the device) applied. Non-contiguous logits are made contiguous. ``B = 0`` launches no
    kernel and gives ``nan`` / ``0`` as torch does.

    Labels are NOT range-checked on the device (that would be a host read): a label outside ``[0, C)``
    is compared, never used as an address, and gives a wrong loss for its row instead of a fault. The
    CPU path does check them."""
    if reduction not in REDUCTIONS:
        raise ValueError(f"{OP}: reduction is 'mean', 'sum' or 'none', got {reduction!r}")
    spec = _parse(OP, logits, target, label_smoothing, lam, labels)
    if meter is not None and not isinstance(meter, ClassificationMeter):
        raise TypeError(f"{OP}: meter is a ClassificationMeter, got {type(meter).__name__}")
    if (return_rank or meter is not None) and spec.labels is None:
        raise ValueError(f"{OP}: return_rank and meter need labels: pass labels= with a dense target")
    loss, rank = _XentFn.apply(logits, spec, reduction, meter, bool(return_rank))
    return (loss, rank) if return_rank else loss


class SoftmaxCrossEntropy(nn.Module):
    """:func:`softmax_cross_entropy` as a module: ``loss = crit(logits, target, **kw)``."""

    def __init__(self, label_smoothing: float = 0.0, reduction: str = "mean"):
        super().__init__()
        if not 0.0 <= float(label_smoothing) < 1.0:
            raise ValueError(f"SoftmaxCrossEntropy: label_smoothing must lie in [0, 1), got {label_smoothing}")
        if reduction not in REDUCTIONS:
            raise ValueError(f"SoftmaxCrossEntropy: reduction is 'mean', 'sum' or 'none', got {reduction!r}")
        self.label_smoothing, self.reduction = float(label_smoothing), reduction

    def forward(self, logits, target, **kw):
        kw.setdefault("reduction", self.reduction)
        if not isinstance(target, MixedLabels):
            kw.setdefault("label_smoothing", self.label_smoothing)
        return softmax_cross_entropy(logits, target, **kw)

    def extra_repr(self) -> str:
        return f"label_smoothing={self.label_smoothing}, reduction={self.reduction!r}"


class ClassificationMeter:
    """A running loss and top-k count that never synchronises until :meth:`read`.

    ``block``: 8 words on the logits' device (created on first use), ``{fp64 sum of the row losses, int64
    rows, int64 correct@k0, int64 correct@k1}`` as an int64 tensor of 4. Passed as ``meter=`` to
    :func:`softmax_cross_entropy`, the loss's finish kernel adds the batch to it: the fixed-order fp32 sum
    of the row losses widened to fp64, ``B``, and the counts of ``rank < k``; one thread, no atomics. It
    works under ``torch.no_grad()`` and inside a captured graph (create the block first: one eager call,
    or :meth:`to`)."""

    def __init__(self, topk=(1, 5)):
        topk = tuple(int(k) for k in topk)
        if len(topk) != 2 or min(topk) < 1:
            raise ValueError(f"ClassificationMeter: topk is two positive ints, got {topk!r}")
        self.topk = topk
        self.block: torch.Tensor | None = None

    def _block_on(self, device) -> torch.Tensor:
        device = torch.empty(0, device=device).device  # with its index
        if self.block is None:
            self.block = torch.zeros(METER_WORDS // 2, dtype=torch.int64, device=device)
        elif self.block.device != device:
            raise ValueError(f"ClassificationMeter: the block lives on {self.block.device}, the batch on {device}")
        return self.block

    def to(self, device):
        """Create the (zeroed) block on ``device`` ahead of the first batch."""
        self._block_on(device)
        return self

    def _add_host(self, loss_row, rank) -> None:
        b = self._block_on(loss_row.device)
        b[:1].view(torch.float64).add_(loss_row.detach().sum().double())
        b[1] += loss_row.shape[0]
        b[2] += (rank < self.topk[0]).sum()
        b[3] += (rank < self.topk[1]).sum()

    def reset(self) -> None:
        """Zero the block: one fill."""
        if self.block is not None:
            self.block.zero_()

    def read(self, reduce: bool = False) -> dict:
        """``{"loss": sum / rows, "rows", "top{k0}", "top{k1}"}``, the accuracies as fractions: the only
        call that synchronises. ``reduce=True`` (after ``Init()``): the four numbers are summed over the
        ranks first, with one fp64 allreduce."""
        if reduce:
            from ..parallel import Initialized, allreduce, device as rank_device
            if not Initialized():
                raise RuntimeError("ClassificationMeter.read(reduce=True) needs Init()")
            if self.block is None:
                self._block_on(rank_device())
        if self.block is None:
            vals = [0.0, 0.0, 0.0, 0.0]
        else:
            v = torch.cat([self.block[:1].view(torch.float64), self.block[1:].to(torch.float64)])
            if reduce:
                v = allreduce(v)
            vals = v.tolist()
        total, rows, c0, c1 = vals
        rows = int(rows)
        nan = float("nan")
        return {"loss": total / rows if rows else nan, "rows": rows,
                f"top{self.topk[0]}": c0 / rows if rows else nan, f"top{self.topk[1]}": c1 / rows if rows else nan}


__all__ = ["softmax_cross_entropy", "xent_reference", "SoftmaxCrossEntropy", "ClassificationMeter", "MixedLabels"]
