"""Fused multi-tensor optimiser steps (wrappers of ``csrc/kernels/optim.hip`` — Adam, the SGD
family, sums of squares — ``csrc/kernels/optim_rules.hip`` — the rest of the rule set — and
``csrc/kernels/optim_layerwise.hip`` — LARS and LAMB).

Each function updates many (param, grad, state...) tuples in one launch per
dtype group. CPU tensors use the PyTorch reference math, which mirrors the
Optimisers.jl formulas term by term (and is the GPU kernels' test oracle).
"""
from __future__ import annotations

import torch

from . import _ext, philox
from .multi_tensor import DTYPE_CODE

_SUPPORTED = {
    (torch.float32, torch.float32, torch.float32, False),
    (torch.float32, torch.bfloat16, torch.float32, False),  # fp32 parameters, bf16 gradients (mixed precision)
    (torch.bfloat16, torch.bfloat16, torch.bfloat16, False),
    (torch.bfloat16, torch.bfloat16, torch.float32, False),
    (torch.bfloat16, torch.bfloat16, torch.float32, True),
    (torch.bfloat16, torch.float32, torch.float32, True),
    (torch.float16, torch.float16, torch.float16, False),
    (torch.float16, torch.float16, torch.float32, False),
    (torch.float16, torch.float16, torch.float32, True),
    (torch.float16, torch.float32, torch.float32, True),
    (torch.float64, torch.float64, torch.float64, False),
}


def supported(p_dtype, g_dtype, s_dtype, master: bool) -> bool:
    return (p_dtype, g_dtype, s_dtype, master) in _SUPPORTED


def _acc_dtype(dt: torch.dtype) -> torch.dtype:
    """Accumulation / scale precision of a gradient dtype: fp32, or fp64 for fp64."""
    return torch.float64 if dt == torch.float64 else torch.float32


def _tscale_ptr(tscale, idx, ct, n) -> int:
    """Device address of the per-leaf scales of the leaves ``idx`` of the call, in list order.

    The kernels index the scales by the leaf's position in the list they are handed: the whole
    call's (one dtype group: the common case), a contiguous run of it, or a gathered copy."""
    if tscale is None:
        return 0
    if tscale.dtype != ct or not tscale.is_contiguous():
        raise TypeError(f"fused optimiser: tscale must be a contiguous {ct} tensor, got {tscale.dtype}")
    if tscale.numel() < n:
        raise ValueError(f"fused optimiser: tscale has {tscale.numel()} entries for {n} leaves")
    if idx == list(range(idx[0], idx[0] + len(idx))):
        return tscale.data_ptr() + idx[0] * tscale.element_size()
    # allocated and consumed on the current stream: the allocator reuses it in stream order
    return tscale[torch.tensor(idx, device=tscale.device)].data_ptr()


def _f32(v: float) -> float:
    """``v`` as the kernels' ``float`` arguments (``grad_scale``, ``clip_delta``) hold it."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _scalars(ct: torch.dtype, *vals):
    """The step's scalars as the kernels hold them: each rounded once to the compute type ``ct``, so that
    ``1 - beta`` is formed in ``ct`` from the rounded ``beta`` (fp32: off by up to 3e-5 of ``1 - 0.999``
    from the double's) and a CPU step is the kernel's to rounding."""
    return [torch.tensor(float(v), dtype=ct) for v in vals]


def _ptr(t: torch.Tensor | None) -> int:
    """Device address of an optional tensor; 0 when it is not given."""
    return t.data_ptr() if t is not None else 0


def _call(C, name: str, *args, _scaling: dict, _sr: tuple | None = None, **kw):
    """Call ``_C``'s entry ``name`` with, as trailing keywords, those of the loss-scaling arguments
    ``_scaling`` (device addresses; 0: not given) that are given and, with ``_sr`` (the generator's
    arguments, :meth:`SR._native`), ``sr``. Without either the call is the entry's plain one."""
    given = {k: v for k, v in _scaling.items() if v}
    if _sr is not None:
        given["sr"] = _sr
    return getattr(C, name)(*args, **kw, **given)


def _skip_ptr(dev_skip) -> int:
    """Device address of the optional skip predicate: one int32, non-zero calls the launch off."""
    if dev_skip is None:
        return 0
    if dev_skip.dtype != torch.int32 or dev_skip.numel() < 1:
        raise TypeError(f"fused optimiser: dev_skip is an int32 tensor of one entry, got {dev_skip.dtype}")
    return dev_skip.data_ptr()


def _skipped(dev_skip) -> bool:
    """The reference path's reading of the skip predicate (a host read: CPU tensors)."""
    return bool(_skip_ptr(dev_skip)) and int(dev_skip.reshape(-1)[0]) != 0


# ---- stochastic rounding of the bf16 stores (csrc/kernels/optim_sr.h, ops/philox.py) --------------
SR_WORDS = 8  # the step block: {uint32 step, 7 unused}


def sr_block(device, step: int = 0) -> torch.Tensor:
    """A fresh step block on ``device`` (8 int32 words, the first the uint32 step counter's bits)."""
    philox.check_ids(0, 0, 0, step)
    blk = torch.zeros(SR_WORDS, dtype=torch.int32)
    blk[0] = int(step) - (1 << 32) if int(step) >= 1 << 31 else int(step)
    return blk.to(device)


def _sr_block_ok(block, what: str) -> None:
    if block.dtype != torch.int32 or block.numel() < SR_WORDS or not block.is_contiguous():
        raise TypeError(f"{what}: the step block is a contiguous int32 tensor of {SR_WORDS} entries (sr_block)")


class SR:
    """The stochastic-rounding argument ``sr=`` of :func:`adam_`, :func:`sgd_`, :func:`rule_` and
    :func:`stochastic_round_`: every bf16 store of the call (the parameter, slot 0, and bf16 state
    tensors, slots 1..3) becomes ``sr(x, r)`` of ``ops.philox`` with Philox4x32-10 bits.

    ``seed``: the key, below 2^64. ``stream``: a caller-chosen id below 2^30 (the engine: the bucket
    index). ``step``: a uint32 from the host, or ``dev_block`` (:func:`sr_block`, advanced by
    :func:`sr_advance_`), whose device value wins: HIP-graph replay. ``offsets``: per leaf of the call
    the index of its first element in the random stream (default 0 for each); leaves of one flat
    buffer given their offsets in it round like one launch over the buffer."""

    def __init__(self, seed: int, stream: int = 0, step: int = 0, dev_block: torch.Tensor | None = None,
                 offsets=None):
        philox.check_ids(seed, stream, 0, step)
        if dev_block is not None:
            _sr_block_ok(dev_block, "SR")
        self.seed, self.stream, self.step, self.dev_block = int(seed), int(stream), int(step), dev_block
        self.offsets = None if offsets is None else [int(o) for o in offsets]
        if self.offsets is not None and any(o < 0 for o in self.offsets):
            raise ValueError("SR: offsets are not negative")

    def _offsets(self, n: int) -> list:
        if self.offsets is None:
            return [0] * n
        if len(self.offsets) != n:
            raise ValueError(f"SR: {len(self.offsets)} offsets for {n} leaves")
        return self.offsets

    def _offset(self, i: int) -> int:
        return 0 if self.offsets is None else self.offsets[i]

    def _native(self, idx, n: int) -> tuple:
        """``(seed, sr_stream, step, dev_step, offsets)``: the update entries' ``sr`` keyword, and under
        those names the keywords of ``mt_stochastic_round``."""
        off = self._offsets(n)
        return self.seed, self.stream, self.step, _ptr(self.dev_block), [off[i] for i in idx]

    def _host_step(self) -> int:
        """The step as the reference path reads it (a host read of the block: CPU tensors)."""
        if self.dev_block is not None:
            return int(self.dev_block.reshape(-1)[0]) & 0xFFFFFFFF
        return self.step


def _sr_check(name: str, sr, params, grads, states, masters) -> None:
    """``sr=`` is for bf16 parameters and gradients without masters, states bf16 or fp32."""
    if sr is None:
        return
    if not isinstance(sr, SR):
        raise TypeError(f"fused {name}: sr is an ops.optim.SR, got {type(sr).__name__}")
    if masters is not None:
        raise ValueError(f"fused {name}: stochastic rounding replaces the fp32 masters: pass masters=None")
    for i, p in enumerate(params):
        dts = [p.dtype, grads[i].dtype]
        if any(d != torch.bfloat16 for d in dts) or any(s[i].dtype not in (torch.bfloat16, torch.float32)
                                                        for s in states):
            raise TypeError(f"fused {name}: leaf {i}: stochastic rounding takes bf16 parameters and gradients with "
                            f"bf16 or fp32 states, got param={p.dtype} grad={grads[i].dtype}")
    sr._offsets(len(params))


def _flat(t: torch.Tensor) -> torch.Tensor:
    """A dense tensor's elements in memory order."""
    return t.reshape(-1) if t.is_contiguous() else t.as_strided((t.numel(),), (1,))


def _store(dst: torch.Tensor, val: torch.Tensor, sr, slot: int, i: int) -> None:
    """The reference path's store ``dst <- val``: a cast, or with ``sr`` and a bf16 ``dst`` the
    stochastic rounding of slot ``slot`` of leaf ``i`` of the call."""
    if sr is None or dst.dtype != torch.bfloat16 or val.dtype != torch.float32:
        dst.copy_(val)
        return
    tmp = torch.empty_like(dst, dtype=torch.float32)  # dst's strides: memory order is the kernels' element order
    tmp.copy_(val)
    _flat(dst).copy_(philox.sr_reference(_flat(tmp), sr.seed, sr.stream, slot, sr._host_step(), sr._offset(i)))


def sr_advance_(block: torch.Tensor, *, dev_skip: torch.Tensor | None = None) -> None:
    """``step += 1`` on the step block (:func:`sr_block`), one thread on the device, after a step's
    launches; not when ``dev_skip`` is non-zero: a skipped step does not count. Graph-capturable."""
    _sr_block_ok(block, "sr_advance_")
    if block.is_cuda:
        _ext.get(required=True).sr_advance(block.data_ptr(), _skip_ptr(dev_skip),
                                           torch.cuda.current_stream(block.device).cuda_stream)
    elif not _skipped(dev_skip):
        nxt = ((int(block[0]) & 0xFFFFFFFF) + 1) & 0xFFFFFFFF
        block[0] = nxt - (1 << 32) if nxt >= 1 << 31 else nxt


def _sr_cast_check(dsts, srcs, sr) -> None:
    if not isinstance(sr, SR):
        raise TypeError(f"stochastic_round_: sr is an ops.optim.SR, got {type(sr).__name__}")
    if len(dsts) != len(srcs):
        raise ValueError(f"stochastic_round_: {len(dsts)} destinations for {len(srcs)} sources")
    for i, (d, x) in enumerate(zip(dsts, srcs)):
        if d.dtype != torch.bfloat16 or x.dtype != torch.float32:
            raise TypeError(f"stochastic_round_: leaf {i}: rounds fp32 to bf16, got {x.dtype} -> {d.dtype}")
        if d.numel() != x.numel() or d.device != x.device or (d.numel() and not _one_memory_order(d, x)):
            raise TypeError(f"stochastic_round_: leaf {i}: destination and source must be dense with one size, "
                            "device and memory order")
    sr._offsets(len(dsts))


def stochastic_round_(dsts, srcs, sr: "SR", *, dev_skip: torch.Tensor | None = None) -> None:
    """``dsts[i] (bf16) <- sr(srcs[i] (fp32))`` over lists of tensors with the bits of slot 0 of
    ``sr``: the update kernels' rounding as a stand-alone multi-tensor cast (``optim_sr.hip``), one
    launch per 24 leaves. ``dev_skip``: as in :func:`adam_`. Graph-capturable."""
    dsts, srcs = list(dsts), list(srcs)
    _sr_cast_check(dsts, srcs, sr)
    if not dsts:
        return
    if not dsts[0].is_cuda:
        stochastic_round_reference_(dsts, srcs, sr, dev_skip=dev_skip)
        return
    _ext.get(required=True).mt_stochastic_round([d.data_ptr() for d in dsts], [x.data_ptr() for x in srcs],
                                                [d.numel() for d in dsts], _skip_ptr(dev_skip),
                                                torch.cuda.current_stream(dsts[0].device).cuda_stream,
                                                **dict(zip(("seed", "sr_stream", "step", "dev_step", "offsets"),
                                                           sr._native(range(len(dsts)), len(dsts)))))


def stochastic_round_reference_(dsts, srcs, sr: "SR", *, dev_skip: torch.Tensor | None = None) -> None:
    """Reference of :func:`stochastic_round_` through ``ops.philox.sr_reference``: the CPU path and
    the kernel's oracle."""
    dsts, srcs = list(dsts), list(srcs)
    _sr_cast_check(dsts, srcs, sr)
    if _skipped(dev_skip):
        return
    with torch.no_grad():
        for i, (d, x) in enumerate(zip(dsts, srcs)):
            if d.numel():
                _store(d, x, sr, 0, i)


def _dtype_groups(name: str, params, grads, states, masters, slots: int) -> list:
    """The call's leaves by (param, grad, state, master) dtype, one ``(idx, pd, head)`` per group, checked
    before anything is launched. ``idx``: the group's positions in the call's lists; ``pd``: its
    parameter dtype; ``head``: the leading arguments of the kernel entry — the address lists of the
    parameters, the gradients, ``slots`` state lists (those beyond ``states`` empty) and the masters
    (empty without), the element counts and the three dtype codes.

    ``TypeError`` unless every leaf's gradient, states (of one dtype; a call without states counts as
    the parameter's, or as fp32 beside a master: the mixed-precision layout) and fp32 master have
    the parameter's element count — the kernels index all of them by it — and the kernels are built
    for the group's dtypes."""
    groups: dict = {}
    for i, p in enumerate(params):
        sd = states[0][i].dtype if states else (torch.float32 if masters is not None else p.dtype)
        if any(s[i].dtype != sd or s[i].numel() != p.numel() for s in states) or grads[i].numel() != p.numel() \
                or (masters is not None and (masters[i].dtype != torch.float32 or masters[i].numel() != p.numel())):
            raise TypeError(f"fused {name}: leaf {i}: gradient, states and master must match the parameter's "
                            "size (states of one dtype, fp32 master)")
        groups.setdefault((p.dtype, grads[i].dtype, sd, masters is not None), []).append(i)
    out = []
    for (pd, gd, sd, hm), idx in groups.items():
        if not supported(pd, gd, sd, hm):
            raise TypeError(f"fused {name}: unsupported dtypes param={pd} grad={gd} state={sd} master={hm}")
        lists = [params, grads, *states, *[None] * (slots - len(states)), masters]
        out.append((idx, pd, [*([t[i].data_ptr() for i in idx] if t is not None else [] for t in lists),
                              [params[i].numel() for i in idx], DTYPE_CODE[pd], DTYPE_CODE[gd], DTYPE_CODE[sd]]))
    return out


def adam_(params, grads, exp_avgs, exp_avg_sqs, *, lr: float, beta1: float, beta2: float, eps: float,
          bc1: float, bc2: float, weight_decay: float = 0.0, grad_scale: float = 1.0, masters=None,
          dev_hyper: torch.Tensor | None = None, dev_gscale: torch.Tensor | None = None,
          tscale: torch.Tensor | None = None, clip_delta: float = 0.0,
          dev_skip: torch.Tensor | None = None, sr: "SR | None" = None) -> None:
    """In-place fused Adam over lists of tensors.

    ``bc1``/``bc2`` are ``1 - beta^t`` (Optimisers.jl keeps ``beta^t`` in the
    state and starts it at ``beta``). ``dev_hyper`` (fp32 ``[lr, beta1^t,
    beta2^t]`` on device) overrides ``lr``/``bc1``/``bc2`` for HIP-graph replay.

    Clipping, applied to the gradient before anything else:
    ``g = clamp(g * grad_scale * dev_gscale * tscale[i], -clip_delta, clip_delta)`` with
    ``tscale`` one device scalar per leaf of ``params`` (fp32; fp64 for fp64 parameters; see
    :func:`sumsq_`) and ``clip_delta == 0`` meaning no clamp.

    ``dev_skip``: one int32 on the device (loss scaling's non-finite flag, :func:`check_finite_`).
    When it is non-zero the launch reads and writes no tensor: the step is called off.

    ``sr`` (:class:`SR`): the bf16 stores — the parameter and bf16 moments — round stochastically
    (bf16 parameters and gradients without masters; else ``TypeError`` / ``ValueError``).
    """
    _sr_check("Adam", sr, params, grads, [exp_avgs, exp_avg_sqs], masters)
    if not params:
        return
    if params[0].is_cuda:
        C = _ext.get(required=True)
        stream = torch.cuda.current_stream(params[0].device).cuda_stream
        for idx, pd, head in _dtype_groups("Adam", params, grads, [exp_avgs, exp_avg_sqs], masters, 2):
            _call(C, "mt_adam", *head, float(lr), float(beta1), float(beta2), float(eps), float(bc1), float(bc2),
                  float(weight_decay), float(grad_scale), _ptr(dev_hyper), _ptr(dev_gscale), stream,
                  tscale=_tscale_ptr(tscale, idx, _acc_dtype(pd), len(params)), clip_delta=float(clip_delta),
                  _scaling={"dev_skip": _skip_ptr(dev_skip)}, _sr=sr and sr._native(idx, len(params)))
        return
    if dev_hyper is not None:
        h = dev_hyper.tolist()
        lr, bc1, bc2 = h[0], 1.0 - float(torch.tensor(h[1])), 1.0 - float(torch.tensor(h[2]))
    grad_scale, clip_delta = _f32(grad_scale), _f32(clip_delta)
    if dev_gscale is not None:
        grad_scale = grad_scale * float(dev_gscale)
    adam_reference_(params, grads, exp_avgs, exp_avg_sqs, lr=lr, beta1=beta1, beta2=beta2, eps=eps, bc1=bc1,
                    bc2=bc2, weight_decay=weight_decay, grad_scale=grad_scale, masters=masters, tscale=tscale,
                    clip_delta=clip_delta, dev_skip=dev_skip, sr=sr)


def _clip_reference(g, i, tscale, clip_delta):
    if tscale is not None:
        g = g * tscale[i].to(g.dtype)
    if clip_delta:
        g = torch.clamp(g, -clip_delta, clip_delta)
    return g


def adam_reference_(params, grads, exp_avgs, exp_avg_sqs, *, lr, beta1, beta2, eps, bc1, bc2,
                    weight_decay=0.0, grad_scale=1.0, masters=None, tscale=None, clip_delta=0.0, dev_skip=None,
                    sr=None):
    """PyTorch reference of the fused kernel (compute in fp32, or fp64 for fp64 params); with ``sr``
    the bf16 stores go through ``ops.philox.sr_reference``."""
    _sr_check("Adam", sr, params, grads, [exp_avgs, exp_avg_sqs], masters)
    if _skipped(dev_skip):
        return
    for i, p in enumerate(params):
        ct = torch.float64 if p.dtype == torch.float64 else torch.float32
        lr_, b1, b2, eps_, c1, c2, wd = _scalars(ct, lr, beta1, beta2, eps, bc1, bc2, weight_decay)
        g = grads[i].to(ct) * grad_scale if grad_scale != 1.0 else grads[i].to(ct)
        g = _clip_reference(g, i, tscale, clip_delta)
        m = exp_avgs[i].to(ct) * b1 + (1 - b1) * g
        v = exp_avg_sqs[i].to(ct) * b2 + (1 - b2) * (g * g)
        x = masters[i].to(ct) if masters is not None else p.to(ct)
        dx = m / c1 / (torch.sqrt(v / c2) + eps_) * lr_
        if weight_decay != 0.0:
            dx = dx + wd * x
        x = x - dx
        _store(exp_avgs[i], m, sr, 1, i)
        _store(exp_avg_sqs[i], v, sr, 2, i)
        if masters is not None:
            masters[i].copy_(x)
        _store(p, x, sr, 0, i)


def adam_advance_(dev_hyper: torch.Tensor, beta1: float, beta2: float, *,
                  dev_skip: torch.Tensor | None = None) -> None:
    """``beta^t *= beta`` on the device hyper block (after the step's Adam launches); not when
    ``dev_skip`` is non-zero: a skipped step does not count."""
    if dev_hyper.is_cuda:
        C = _ext.get(required=True)
        _call(C, "adam_advance", dev_hyper.data_ptr(), float(beta1), float(beta2),
              torch.cuda.current_stream(dev_hyper.device).cuda_stream, _scaling={"dev_skip": _skip_ptr(dev_skip)})
    elif not _skipped(dev_skip):
        dev_hyper[1] *= beta1
        dev_hyper[2] *= beta2


def sgd_(params, grads, bufs, *, lr: float, momentum: float = 0.0, nesterov: bool = False,
         weight_decay: float = 0.0, grad_scale: float = 1.0, masters=None,
         dev_lr: torch.Tensor | None = None, dev_gscale: torch.Tensor | None = None,
         tscale: torch.Tensor | None = None, clip_delta: float = 0.0,
         dev_skip: torch.Tensor | None = None, sr: "SR | None" = None) -> None:
    """Fused Descent / Momentum / Nesterov (Optimisers.jl semantics); ``dev_gscale``, ``tscale``,
    ``clip_delta``, ``dev_skip`` and ``sr`` as in :func:`adam_` (the clipped gradient is formed before
    weight decay)."""
    _sr_check("SGD", sr, params, grads, [bufs] if momentum != 0.0 else [], masters)
    if not params:
        return
    if params[0].is_cuda:
        C = _ext.get(required=True)
        stream = torch.cuda.current_stream(params[0].device).cuda_stream
        # without momentum the buffers are not read: Optimisers.Descent has none
        for idx, pd, head in _dtype_groups("SGD", params, grads, [bufs] if momentum != 0.0 else [], masters, 1):
            _call(C, "mt_sgd", *head, float(lr), float(momentum), float(weight_decay), float(grad_scale),
                  int(bool(nesterov)),
                  _ptr(dev_lr), stream, dev_gscale=_ptr(dev_gscale),
                  tscale=_tscale_ptr(tscale, idx, _acc_dtype(pd), len(params)), clip_delta=float(clip_delta),
                  _scaling={"dev_skip": _skip_ptr(dev_skip)}, _sr=sr and sr._native(idx, len(params)))
        return
    if dev_lr is not None:
        lr = float(dev_lr.reshape(-1)[0])
    grad_scale, clip_delta = _f32(grad_scale), _f32(clip_delta)
    if dev_gscale is not None:
        grad_scale = grad_scale * float(dev_gscale)
    sgd_reference_(params, grads, bufs, lr=lr, momentum=momentum, nesterov=nesterov, weight_decay=weight_decay,
                   grad_scale=grad_scale, masters=masters, tscale=tscale, clip_delta=clip_delta, dev_skip=dev_skip,
                   sr=sr)


def sgd_reference_(params, grads, bufs, *, lr, momentum=0.0, nesterov=False, weight_decay=0.0, grad_scale=1.0,
                   masters=None, tscale=None, clip_delta=0.0, dev_skip=None, sr=None):
    _sr_check("SGD", sr, params, grads, [bufs] if momentum != 0.0 else [], masters)
    if _skipped(dev_skip):
        return
    for i, p in enumerate(params):
        ct = torch.float64 if p.dtype == torch.float64 else torch.float32
        lr_, rho, wd = _scalars(ct, lr, momentum, weight_decay)
        x = masters[i].to(ct) if masters is not None else p.to(ct)
        g = _clip_reference(grads[i].to(ct) * grad_scale, i, tscale, clip_delta)
        if weight_decay:
            g = g + wd * x
        if momentum == 0.0:
            dx = g * lr_
        elif not nesterov:
            vel = rho * bufs[i].to(ct) + lr_ * g
            _store(bufs[i], vel, sr, 1, i)
            dx = vel
        else:
            vel0 = bufs[i].to(ct)
            dx = -(rho * rho) * vel0 + (1 + rho) * lr_ * g
            _store(bufs[i], rho * vel0 - lr_ * g, sr, 1, i)
        x = x - dx
        if masters is not None:
            masters[i].copy_(x)
        _store(p, x, sr, 0, i)


# kind -> (code of the kernel's rule switch, state tensors per leaf, reads beta^t)
RULES = {
    "rmsprop": (0, 1, False),
    "adagrad": (1, 1, False),
    "lion": (2, 1, False),
    "adamax": (3, 2, True),
    "amsgrad": (4, 3, False),
    "nadam": (5, 2, True),
    "adabelief": (6, 2, True),
    "adadelta": (7, 2, False),
}


def _rule_info(kind: str) -> tuple:
    try:
        return RULES[kind]
    except KeyError:
        raise ValueError(f"fused optimiser: unknown rule {kind!r} (one of {sorted(RULES)})") from None


def rule_(kind: str, params, grads, states, *, lr: float = 0.0, beta1: float = 0.0, beta2: float = 0.0,
          rho: float | None = None, eps: float = 0.0, bt1: float = 0.0, bt2: float = 0.0, masters=None,
          dev_hyper: torch.Tensor | None = None, dev_gscale: torch.Tensor | None = None,
          tscale: torch.Tensor | None = None, clip_delta: float = 0.0, weight_decay: float = 0.0,
          grad_scale: float = 1.0, dev_skip: torch.Tensor | None = None, sr: "SR | None" = None) -> None:
    """In-place fused step of one of :data:`RULES` over lists of tensors (``optim_rules.hip``).

    ``states``: one list of tensors per state slot of the rule, in the order of its Optimisers.jl
    state (RMSProp / AdaGrad ``[acc]``, Lion ``[m]``, AdaMax ``[m, u]``, AMSGrad ``[m, v, v̂]``,
    NAdam ``[m, v]``, AdaBelief ``[m, s]``, AdaDelta ``[acc, Δ]``). ``rho`` (RMSProp, AdaDelta)
    is another name of ``beta1``. ``bt1`` / ``bt2`` are ``beta^t`` (AdaMax, NAdam, AdaBelief:
    Optimisers.jl keeps them in the state and starts them at ``beta``); ``dev_hyper`` (fp32
    ``[lr, beta1^t, beta2^t]``, or ``[lr]`` for the rules without ``beta^t``) overrides them for
    HIP-graph replay, advanced by :func:`adam_advance_`. ``weight_decay`` adds ``wd * x`` to the
    rule's ``dx'`` (an ``OptimiserChain(rule, WeightDecay)``); the clip arguments, ``dev_skip`` and
    ``sr`` are :func:`adam_`'s."""
    code, ns, has_bt = _rule_info(kind)
    if rho is not None:
        beta1 = rho
    states = [list(s) for s in states]
    if len(states) != ns or any(len(s) != len(params) for s in states) or len(grads) != len(params):
        raise ValueError(f"fused {kind}: needs {ns} state list(s) and a gradient per parameter")
    if masters is not None and len(masters) != len(params):
        raise ValueError(f"fused {kind}: needs a master per parameter")
    _sr_check(kind, sr, params, grads, states, masters)
    if dev_hyper is not None and (dev_hyper.dtype != torch.float32 or dev_hyper.numel() < (3 if has_bt else 1)
                                  or not dev_hyper.is_contiguous()):
        raise TypeError(f"fused {kind}: dev_hyper is a contiguous fp32 tensor of {3 if has_bt else 1} entries")
    if not params:
        return
    if params[0].is_cuda:
        C = _ext.get(required=True)
        stream = torch.cuda.current_stream(params[0].device).cuda_stream
        for idx, pd, head in _dtype_groups(kind, params, grads, states, masters, 3):
            _call(C, "mt_rule", code, *head, float(lr), float(beta1), float(beta2), float(eps), float(bt1), float(bt2),
                  float(weight_decay), float(grad_scale), _ptr(dev_hyper), _ptr(dev_gscale),
                  _tscale_ptr(tscale, idx, _acc_dtype(pd), len(params)), float(clip_delta), stream,
                  _scaling={"dev_skip": _skip_ptr(dev_skip)}, _sr=sr and sr._native(idx, len(params)))
        return
    if dev_hyper is not None:
        h = dev_hyper.tolist()
        lr = h[0]
        if has_bt:
            bt1, bt2 = h[1], h[2]
    grad_scale, clip_delta = _f32(grad_scale), _f32(clip_delta)
    if dev_gscale is not None:
        grad_scale = grad_scale * float(dev_gscale)
    rule_reference_(kind, params, grads, states, lr=lr, beta1=beta1, beta2=beta2, eps=eps, bt1=bt1, bt2=bt2,
                    masters=masters, tscale=tscale, clip_delta=clip_delta, weight_decay=weight_decay,
                    grad_scale=grad_scale, dev_skip=dev_skip, sr=sr)


def rule_reference_(kind: str, params, grads, states, *, lr=0.0, beta1=0.0, beta2=0.0, rho=None, eps=0.0, bt1=0.0,
                    bt2=0.0, masters=None, tscale=None, clip_delta=0.0, weight_decay=0.0, grad_scale=1.0,
                    dev_skip=None, sr=None):
    """PyTorch reference of :func:`rule_`, term by term as the rules of ``optimisers`` write them
    (compute in fp32, or fp64 for fp64 params): the CPU path and the kernels' oracle."""
    _, ns, _ = _rule_info(kind)
    _sr_check(kind, sr, params, grads, [list(st) for st in states], masters)
    if _skipped(dev_skip):
        return
    if rho is not None:
        beta1 = rho
    hyper = (lr, beta1, beta2, eps, bt1, bt2, weight_decay)
    for i, p in enumerate(params):
        ct = torch.float64 if p.dtype == torch.float64 else torch.float32
        lr, b1, b2, eps, bt1, bt2, wd = _scalars(ct, *hyper)
        g = grads[i].to(ct) * grad_scale if grad_scale != 1.0 else grads[i].to(ct)
        g = _clip_reference(g, i, tscale, clip_delta)
        s = [st[i].to(ct) for st in states]
        x = masters[i].to(ct) if masters is not None else p.to(ct)
        if kind == "rmsprop":
            s[0] = s[0] * b1 + (1 - b1) * (g * g)
            dx = g * lr / (torch.sqrt(s[0]) + eps)
        elif kind == "adagrad":
            s[0] = s[0] + g * g
            dx = g * lr / (torch.sqrt(s[0]) + eps)
        elif kind == "lion":
            a = s[0] * b1 + (1 - b1) * g
            dx = lr * torch.where(torch.isnan(a), a, torch.sign(a))  # torch.sign(NaN) is 0; the kernel keeps the NaN
            s[0] = s[0] * b2 + (1 - b2) * g
        elif kind == "adamax":
            s[0] = s[0] * b1 + (1 - b1) * g
            s[1] = torch.maximum(s[1] * b2, g.abs())
            dx = lr / (1 - bt1) * s[0] / (s[1] + eps)
        elif kind == "amsgrad":
            s[0] = s[0] * b1 + (1 - b1) * g
            s[1] = s[1] * b2 + (1 - b2) * (g * g)
            s[2] = torch.maximum(s[2], s[1])
            dx = lr * s[0] / (torch.sqrt(s[2]) + eps)
        elif kind == "nadam":
            s[0] = s[0] * b1 + (1 - b1) * g
            s[1] = s[1] * b2 + (1 - b2) * (g * g)
            dx = (b1 * s[0] / (1 - b1 * bt1) + (1 - b1) * g / (1 - bt1)) / (torch.sqrt(s[1] * b2 / (1 - bt2)) + eps) * lr
        elif kind == "adabelief":
            s[0] = s[0] * b1 + (1 - b1) * g
            s[1] = s[1] * b2 + (1 - b2) * (g - s[0]) ** 2 + eps
            dx = lr * s[0] / (1 - bt1) / (torch.sqrt(s[1] / (1 - bt2)) + eps)
        else:  # adadelta
            s[0] = s[0] * b1 + (1 - b1) * (g * g)
            dx = g * torch.sqrt(s[1] + eps) / torch.sqrt(s[0] + eps)
            s[1] = s[1] * b1 + (1 - b1) * (dx * dx)
        if weight_decay != 0.0:
            dx = dx + wd * x
        x = x - dx
        for k in range(ns):
            _store(states[k][i], s[k], sr, k + 1, i)
        if masters is not None:
            masters[i].copy_(x)
        _store(p, x, sr, 0, i)


# ---- layer-wise adaptive rules (csrc/kernels/optim_layerwise.hip) ---------------------------------
LAYERWISE = {"lars": 8, "lamb": 9}  # codes of the kernel's rule switch, behind rule_'s entry


def layerwise_workspace(params) -> int:
    """Entries of the ``workspace`` :func:`lars_` / :func:`lamb_` need for ``params``: two per
    4096-element chunk (the chunk's sums of squares of the parameter and of the gradient / update)."""
    return 2 * sumsq_partials(params)


def _layerwise_(kind, params, grads, states, hyper, *, weight_decay, grad_scale, masters, dev_hyper, dev_gscale,
                ratios, workspace, dev_skip=None):
    """The GPU side of :func:`lars_` / :func:`lamb_`: one ``mt_rule`` call per dtype group, each leaf's
    slice of the workspace in the ``s3`` slot and the ratio table in ``tscale``."""
    C = _ext.get(required=True)
    dev = params[0].device
    stream = torch.cuda.current_stream(dev).cuda_stream
    nh = 3 if kind == "lamb" else 1
    if dev_hyper is not None and (dev_hyper.dtype != torch.float32 or dev_hyper.numel() < nh
                                  or not dev_hyper.is_contiguous()):
        raise TypeError(f"fused {kind}: dev_hyper is a contiguous fp32 tensor of {nh} entries")
    groups = _dtype_groups(kind, params, grads, states, masters, 3)
    for idx, pd, head in groups:
        at = _acc_dtype(pd)
        need = layerwise_workspace([params[i] for i in idx])
        ws = workspace
        if ws is None or len(groups) > 1:
            # allocated and consumed on the current stream: the allocator reuses it in stream order
            ws = torch.empty(max(need, 1), dtype=at, device=dev)
        elif ws.dtype != at or ws.numel() < need or not ws.is_contiguous() or ws.device != dev:
            raise TypeError(f"fused {kind}: workspace must be a contiguous {at} tensor with at least {need} entries "
                            f"on {dev} (layerwise_workspace)")
        table = ratios
        if table is None or idx != list(range(len(params))):
            table = torch.empty(len(idx), dtype=at, device=dev)
        elif table.dtype != at or table.numel() < len(idx) or not table.is_contiguous() or table.device != dev:
            raise TypeError(f"fused {kind}: ratios must be a contiguous {at} tensor with {len(idx)} entries on {dev}")
        part, off, esz = [], 0, ws.element_size()
        for k, i in enumerate(idx):
            part.append(ws.data_ptr() + off * esz)
            off += 2 * ((params[i].numel() + 4095) // 4096)
            if params[i].numel() == 0:
                table[k:k + 1].fill_(1)  # a leaf without elements reaches no kernel: ratio 1
        head[4] = part  # the s3 slot
        _call(C, "mt_rule", LAYERWISE[kind], *head, float(hyper["lr"]), float(hyper["beta1"]), float(hyper["beta2"]),
              float(hyper["eps"]), float(hyper.get("bt1", 0.0)), float(hyper.get("bt2", 0.0)), float(weight_decay),
              float(grad_scale), _ptr(dev_hyper), _ptr(dev_gscale), table.data_ptr(), 0.0, stream,
              _scaling={"dev_skip": _skip_ptr(dev_skip)})
        if ratios is not None and table is not ratios:
            if dev_skip is not None:
                raise ValueError(f"fused {kind}: with dev_skip the ratios of a call of several dtype groups cannot "
                                 "be kept through a skipped step; call once per dtype group")
            ratios[torch.tensor(idx, device=dev)] = table.to(ratios.dtype)


def _check_layerwise(kind, params, grads, states, masters, ratios):
    if any(len(s) != len(params) for s in states) or len(grads) != len(params):
        raise ValueError(f"fused {kind}: needs a gradient and {len(states)} state tensor(s) per parameter")
    if masters is not None and len(masters) != len(params):
        raise ValueError(f"fused {kind}: needs a master per parameter")
    if ratios is not None and ratios.numel() < len(params):
        raise ValueError(f"fused {kind}: ratios has {ratios.numel()} entries for {len(params)} leaves")


def lars_(params, grads, bufs, *, lr: float, momentum: float, trust: float, weight_decay: float = 0.0,
          eps: float = 0.0, grad_scale: float = 1.0, masters=None, dev_hyper: torch.Tensor | None = None,
          dev_gscale: torch.Tensor | None = None, ratios: torch.Tensor | None = None,
          workspace: torch.Tensor | None = None, dev_skip: torch.Tensor | None = None) -> None:
    """In-place fused LARS over lists of tensors, every leaf adapted (``optim_layerwise.hip``):
    ``q = trust·‖x‖ / (‖g‖ + wd·‖x‖ + eps)`` (1 when either norm is 0), ``vel = momentum·vel +
    lr·q·(g + wd·x)``, ``x -= vel`` with ``g = grads[i] * grad_scale * dev_gscale`` and ``x`` the
    fp32 master where there is one. Two launches per 24 leaves (three with a leaf above 16.8M
    elements), deterministic norms, no host read.

    ``dev_hyper``: fp32 ``[lr]`` on the device. ``ratios``: optional table (fp32; fp64 for fp64
    parameters) that receives ``q`` of each leaf of ``params``. ``workspace``: scratch of
    :func:`layerwise_workspace` entries of the same dtype, allocated here when not given.
    ``dev_skip``: as in :func:`adam_`; a skipped step also leaves ``ratios`` as they were."""
    states = [list(bufs)]
    _check_layerwise("lars", params, grads, states, masters, ratios)
    if not params:
        return
    if params[0].is_cuda:
        _layerwise_("lars", params, grads, states, {"lr": lr, "beta1": momentum, "beta2": trust, "eps": eps},
                    weight_decay=weight_decay, grad_scale=grad_scale, masters=masters, dev_hyper=dev_hyper,
                    dev_gscale=dev_gscale, ratios=ratios, workspace=workspace, dev_skip=dev_skip)
        return
    if dev_hyper is not None:
        lr = float(dev_hyper.reshape(-1)[0])
    grad_scale = _f32(grad_scale)
    if dev_gscale is not None:
        grad_scale = grad_scale * float(dev_gscale)
    lars_reference_(params, grads, bufs, lr=lr, momentum=momentum, trust=trust, weight_decay=weight_decay, eps=eps,
                    grad_scale=grad_scale, masters=masters, ratios=ratios, dev_skip=dev_skip)


def lamb_(params, grads, exp_avgs, exp_avg_sqs, *, lr: float, beta1: float, beta2: float, eps: float,
          bt1: float, bt2: float, weight_decay: float = 0.0, grad_scale: float = 1.0, masters=None,
          dev_hyper: torch.Tensor | None = None, dev_gscale: torch.Tensor | None = None,
          ratios: torch.Tensor | None = None, workspace: torch.Tensor | None = None,
          dev_skip: torch.Tensor | None = None) -> None:
    """In-place fused LAMB over lists of tensors, every leaf adapted (``optim_layerwise.hip``):
    Adam's ``m`` and ``v``, ``u = m/(1-bt1) / (sqrt(v/(1-bt2)) + eps) + wd·x``, ``q = ‖x‖/‖u‖`` (1
    when either norm is 0), ``x -= lr·q·u``. ``bt1`` / ``bt2`` are ``beta^t``; ``dev_hyper`` (fp32
    ``[lr, beta1^t, beta2^t]``) overrides them and ``lr``, advanced by :func:`adam_advance_`. The
    other arguments are :func:`lars_`'s. ``u`` is never written to memory: the second phase forms it
    again from the stored ``m`` and ``v``."""
    states = [list(exp_avgs), list(exp_avg_sqs)]
    _check_layerwise("lamb", params, grads, states, masters, ratios)
    if not params:
        return
    if params[0].is_cuda:
        _layerwise_("lamb", params, grads, states,
                    {"lr": lr, "beta1": beta1, "beta2": beta2, "eps": eps, "bt1": bt1, "bt2": bt2},
                    weight_decay=weight_decay, grad_scale=grad_scale, masters=masters, dev_hyper=dev_hyper,
                    dev_gscale=dev_gscale, ratios=ratios, workspace=workspace, dev_skip=dev_skip)
        return
    if dev_hyper is not None:
        h = dev_hyper.tolist()
        lr, bt1, bt2 = h[0], h[1], h[2]
    grad_scale = _f32(grad_scale)
    if dev_gscale is not None:
        grad_scale = grad_scale * float(dev_gscale)
    lamb_reference_(params, grads, exp_avgs, exp_avg_sqs, lr=lr, beta1=beta1, beta2=beta2, eps=eps, bt1=bt1, bt2=bt2,
                    weight_decay=weight_decay, grad_scale=grad_scale, masters=masters, ratios=ratios,
                    dev_skip=dev_skip)


def _norm(t: torch.Tensor) -> torch.Tensor:
    return torch.sqrt((t * t).sum())


def lars_reference_(params, grads, bufs, *, lr, momentum, trust, weight_decay=0.0, eps=0.0, grad_scale=1.0,
                    masters=None, ratios=None, dev_skip=None):
    """PyTorch reference of :func:`lars_` (compute in fp32, or fp64 for fp64 params)."""
    if _skipped(dev_skip):
        return
    for i, p in enumerate(params):
        ct = torch.float64 if p.dtype == torch.float64 else torch.float32
        lr_, rho, tr, wd, eps_ = _scalars(ct, lr, momentum, trust, weight_decay, eps)
        x = masters[i].to(ct) if masters is not None else p.to(ct)
        g = grads[i].to(ct) * grad_scale
        xn, gn = _norm(x), _norm(g)
        q = torch.where((xn > 0) & (gn > 0), tr * xn / (gn + wd * xn + eps_), torch.ones_like(xn))
        d = g + wd * x if weight_decay else g
        vel = rho * bufs[i].to(ct) + lr_ * (q * d)
        bufs[i].copy_(vel)
        x = x - vel
        if ratios is not None:
            ratios[i] = q
        if masters is not None:
            masters[i].copy_(x)
        p.copy_(x)


def lamb_reference_(params, grads, exp_avgs, exp_avg_sqs, *, lr, beta1, beta2, eps, bt1, bt2, weight_decay=0.0,
                    grad_scale=1.0, masters=None, ratios=None, dev_skip=None):
    """PyTorch reference of :func:`lamb_` (compute in fp32, or fp64 for fp64 params): ``u`` is formed
    from the moments as stored, in the state's dtype."""
    if _skipped(dev_skip):
        return
    for i, p in enumerate(params):
        ct = torch.float64 if p.dtype == torch.float64 else torch.float32
        lr_, b1, b2, eps_, t1, t2, wd = _scalars(ct, lr, beta1, beta2, eps, bt1, bt2, weight_decay)
        x = masters[i].to(ct) if masters is not None else p.to(ct)
        g = grads[i].to(ct) * grad_scale
        exp_avgs[i].copy_(exp_avgs[i].to(ct) * b1 + (1 - b1) * g)
        exp_avg_sqs[i].copy_(exp_avg_sqs[i].to(ct) * b2 + (1 - b2) * (g * g))
        u = exp_avgs[i].to(ct) / (1 - t1) / (torch.sqrt(exp_avg_sqs[i].to(ct) / (1 - t2)) + eps_)
        if weight_decay:
            u = u + wd * x
        xn, un = _norm(x), _norm(u)
        q = torch.where((xn > 0) & (un > 0), xn / un, torch.ones_like(xn))
        x = x - (lr_ * q) * u
        if ratios is not None:
            ratios[i] = q
        if masters is not None:
            masters[i].copy_(x)
        p.copy_(x)


def sumsq_partials(grads) -> int:
    """Entries of the ``partials`` workspace :func:`sumsq_` needs for ``grads`` (one per 4096-element chunk)."""
    return sum((g.numel() + 4095) // 4096 for g in grads)


def sumsq_(grads, out: torch.Tensor, *, scales: torch.Tensor | None = None, omega: float = 0.0,
           grad_scale: float = 1.0, partials: torch.Tensor | None = None, flag: torch.Tensor | None = None,
           dev_pre: torch.Tensor | None = None) -> None:
    """``out[i] = sum(grads[i] ** 2)`` for a list of dense gradients of one dtype, deterministically
    (two launches per 24 leaves, no float atomics: bit-identical from run to run), and, with
    ``scales``, the ClipNorm factors ``scales[i] = min(1, omega / (grad_scale * sqrt(out[i])))``
    — ``torch.clamp(omega / nrm, max=1)``: norm 0 gives 1, NaN gives NaN, inf gives 0.

    ``out`` / ``scales`` / ``partials`` are fp32 (fp64 for fp64 gradients) tensors on the
    gradients' device with ``len(grads)`` (``partials``: :func:`sumsq_partials`) entries;
    ``partials`` is scratch, allocated here when not given. No host read: graph-capturable.

    ``flag`` (one int32): the same pass runs :func:`check_finite_`'s test on every element it reads,
    so an engine that takes norms reads its gradients once; ``out`` and ``scales`` are the bits of
    the call without it. ``dev_pre`` (one fp32 on the device, the inverse loss scale) is multiplied
    into the norm — ``scales[i] = min(1, omega / (grad_scale * dev_pre * sqrt(out[i])))``, the
    factors of the unscaled gradient; ``out`` stays the raw sum.
    """
    if not grads:
        return
    gd, n = grads[0].dtype, len(grads)
    at = _acc_dtype(gd)
    if any(g.dtype != gd or g.device != grads[0].device for g in grads):
        raise TypeError("sumsq_: the gradients of one call share one dtype and device")
    for name, t in (("out", out), ("scales", scales)):
        if t is not None and (t.dtype != at or t.numel() < n or not t.is_contiguous() or t.device != grads[0].device):
            raise TypeError(f"sumsq_: {name} must be a contiguous {at} tensor with {n} entries on {grads[0].device}")
    if grads[0].is_cuda:
        if gd not in DTYPE_CODE or not gd.is_floating_point:
            raise TypeError(f"sumsq_: unsupported gradient dtype {gd}")
        C = _ext.get(required=True)
        need = sumsq_partials(grads)
        if partials is None:
            partials = torch.empty(max(need, 1), dtype=at, device=grads[0].device)
        elif partials.dtype != at or partials.numel() < need or not partials.is_contiguous():
            raise TypeError(f"sumsq_: partials must be a contiguous {at} tensor with at least {need} entries")
        _call(C, "mt_leaf_sumsq", [g.data_ptr() for g in grads], [g.numel() for g in grads], DTYPE_CODE[gd],
              partials.data_ptr(), out.data_ptr(), _ptr(scales),
              float(omega), float(grad_scale), torch.cuda.current_stream(grads[0].device).cuda_stream,
              _scaling={"nonfinite_flag": _flag_ptr(flag), "dev_pre": _pre_ptr(dev_pre)})
        return
    ss = torch.stack([(g.to(at) * g.to(at)).sum() for g in grads])
    out[:n].copy_(ss)
    if scales is not None:
        nrm = grad_scale * torch.sqrt(ss)
        if dev_pre is not None:
            nrm = nrm * dev_pre.reshape(-1)[0].to(at)
        scales[:n].copy_(torch.clamp(omega / nrm, max=1.0).to(at))
    if flag is not None:
        check_finite_reference_(grads, flag)


def _flag_ptr(flag) -> int:
    if flag is None:
        return 0
    if flag.dtype != torch.int32 or flag.numel() < 1:
        raise TypeError(f"non-finite check: flag is an int32 tensor of one entry, got {flag.dtype}")
    return flag.data_ptr()


def _pre_ptr(dev_pre) -> int:
    if dev_pre is None:
        return 0
    if dev_pre.dtype != torch.float32 or dev_pre.numel() < 1:
        raise TypeError(f"dev_pre is an fp32 tensor of one entry, got {dev_pre.dtype}")
    return dev_pre.data_ptr()


def check_finite_(grads, flag: torch.Tensor) -> None:
    """``flag[0] = 1`` if any element of any of ``grads`` is inf or NaN; untouched otherwise.

    The test is exact and per element (exponent field all ones), not "the sum of squares came out
    non-finite": a bf16 or fp32 gradient of 1e20 is finite while its square is not. ``flag`` (one
    int32 on the gradients' device) is sticky: the checks of all buckets and dtypes of a step
    accumulate into it and only :func:`loss_scale_update_` clears it. One launch per 24 leaves of a
    dtype in the update kernels' job layout, no atomics, no host read: graph-capturable."""
    if not grads:
        return
    if flag.dtype != torch.int32 or flag.numel() < 1 or flag.device != grads[0].device:
        raise TypeError(f"check_finite_: flag is an int32 tensor of one entry on {grads[0].device}")
    if not grads[0].is_cuda:
        check_finite_reference_(grads, flag)
        return
    S = _ext.get(required=True)
    stream = torch.cuda.current_stream(grads[0].device).cuda_stream
    by_dtype: dict = {}
    for g in grads:
        if g.dtype not in DTYPE_CODE or not g.dtype.is_floating_point or g.device != grads[0].device:
            raise TypeError(f"check_finite_: unsupported gradient {g.dtype} on {g.device}")
        by_dtype.setdefault(g.dtype, []).append(g)
    for gd, gs in by_dtype.items():
        S.mt_check_finite([g.data_ptr() for g in gs], [g.numel() for g in gs], DTYPE_CODE[gd], flag.data_ptr(), stream)


def check_finite_reference_(grads, flag: torch.Tensor) -> None:
    """PyTorch reference of :func:`check_finite_` (``torch.isfinite`` per element)."""
    if any(g.numel() and not bool(torch.isfinite(g).all()) for g in grads):
        flag.reshape(-1)[0] = 1


# the scaler's device block (csrc/api.h: loss_scale_update): 8 int32 words, the first two fp32 bits
LS_WORDS = 8
LS_SCALE, LS_INV, LS_TRACKER, LS_SKIPPED, LS_LAST, LS_FLAG = range(6)


def loss_scale_block(scale: float, device, *, tracker: int = 0, skipped: int = 0) -> torch.Tensor:
    """A fresh scaler block on ``device``: ``scale``, its inverse, the counters; last-skipped and flag clear."""
    blk = torch.zeros(LS_WORDS, dtype=torch.int32)
    f = blk.view(torch.float32)
    f[LS_SCALE] = scale
    f[LS_INV] = 1.0 / f[LS_SCALE]
    blk[LS_TRACKER], blk[LS_SKIPPED] = int(tracker), int(skipped)
    return blk.to(device)


def loss_scale_update_(block: torch.Tensor, *, growth: float, backoff: float, interval: int, min_scale: float,
                       max_scale: float) -> None:
    """``GradScaler``'s rule on the scaler block (:func:`loss_scale_block`), one thread on the device:
    flag set → ``scale *= backoff``, tracker = 0, skipped += 1; flag clear → tracker += 1 and at
    ``tracker == interval`` ``scale *= growth``, tracker = 0. Then the scale is clamped to
    ``[min_scale, max_scale]``, its inverse stored, the flag copied to "last step skipped" and
    cleared. A static scale is ``growth = backoff = 1``. No host read: graph-capturable."""
    if block.dtype != torch.int32 or block.numel() < LS_WORDS or not block.is_contiguous():
        raise TypeError(f"loss_scale_update_: block is a contiguous int32 tensor of {LS_WORDS} entries")
    if block.is_cuda:
        _ext.get(required=True).loss_scale_update(block.data_ptr(), float(growth), float(backoff), int(interval),
                                                  float(min_scale), float(max_scale),
                                                  torch.cuda.current_stream(block.device).cuda_stream)
        return
    loss_scale_update_reference_(block, growth=growth, backoff=backoff, interval=interval, min_scale=min_scale,
                                 max_scale=max_scale)


def loss_scale_update_reference_(block: torch.Tensor, *, growth, backoff, interval, min_scale, max_scale) -> None:
    """PyTorch reference of :func:`loss_scale_update_` on a CPU block, in fp32 as the kernel computes."""
    f = block.view(torch.float32)
    scale, flag = f[LS_SCALE].clone(), int(block[LS_FLAG])
    if flag != 0:
        scale = scale * torch.tensor(backoff, dtype=torch.float32)
        block[LS_TRACKER] = 0
        block[LS_SKIPPED] += 1
    else:
        block[LS_TRACKER] += 1
        if int(block[LS_TRACKER]) == int(interval):
            scale = scale * torch.tensor(growth, dtype=torch.float32)
            block[LS_TRACKER] = 0
    scale = torch.clamp(scale, torch.tensor(min_scale, dtype=torch.float32), torch.tensor(max_scale, dtype=torch.float32))
    f[LS_SCALE] = scale
    f[LS_INV] = 1.0 / scale
    block[LS_LAST] = 1 if flag != 0 else 0
    block[LS_FLAG] = 0


# ---- exponential moving average of the weights (csrc/kernels/optim_ema.hip) -----------------------
# the EMA device block (csrc/api.h: ema_advance): 8 int32 words, the first two fp32 bits
EMA_WORDS = 8
EMA_OMD, EMA_DECAY, EMA_UPDATES, EMA_SINCE, EMA_HOLD = range(5)


def _ema_decay_at(decay: float, warmup: bool, n: int) -> torch.Tensor:
    """``d_t`` after ``n`` EMA updates, in fp32 as the kernel computes it."""
    d = torch.tensor(decay, dtype=torch.float32)
    if warmup:
        d = torch.minimum(d, torch.tensor(1.0 + n, dtype=torch.float32) / torch.tensor(10.0 + n, dtype=torch.float32))
    return d


def ema_block(decay: float, warmup: bool, every: int, device, *, updates: int = 0, since: int = 0) -> torch.Tensor:
    """A fresh EMA block on ``device`` with the values of the coming step: ``d_t`` (``warmup``:
    ``min(decay, (1 + n) / (10 + n))`` with ``n = updates``), ``omd = 1 - d_t``, the counters, and
    ``hold = since + 1 < every`` (the coming optimiser step is not an EMA step)."""
    if not 0.0 <= decay < 1.0 or int(every) < 1:
        raise ValueError(f"ema_block: need 0 <= decay < 1 and every >= 1, got decay={decay} every={every}")
    blk = torch.zeros(EMA_WORDS, dtype=torch.int32)
    f = blk.view(torch.float32)
    f[EMA_DECAY] = _ema_decay_at(decay, warmup, int(updates))
    f[EMA_OMD] = 1.0 - f[EMA_DECAY]
    blk[EMA_UPDATES], blk[EMA_SINCE] = int(updates), int(since)
    blk[EMA_HOLD] = 1 if int(since) + 1 < int(every) else 0
    return blk.to(device)


def _ema_block_ok(block, what: str) -> None:
    if block.dtype != torch.int32 or block.numel() < EMA_WORDS or not block.is_contiguous():
        raise TypeError(f"{what}: the EMA block is a contiguous int32 tensor of {EMA_WORDS} entries (ema_block)")


def _ema_check(emas, srcs) -> None:
    if len(emas) != len(srcs):
        raise ValueError(f"ema_: {len(emas)} EMA leaves for {len(srcs)} sources")
    for i, (e, x) in enumerate(zip(emas, srcs)):
        if x.dtype not in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
            raise TypeError(f"ema_: leaf {i}: unsupported source dtype {x.dtype}")
        if e.dtype != _acc_dtype(x.dtype):
            raise TypeError(f"ema_: leaf {i}: the EMA of a {x.dtype} source is kept in {_acc_dtype(x.dtype)}, "
                            f"got {e.dtype}")
        if e.numel() != x.numel() or e.device != x.device:
            raise TypeError(f"ema_: leaf {i}: EMA and source differ in size or device")
        if e.numel() and not _one_memory_order(e, x):
            raise TypeError(f"ema_: leaf {i}: EMA and source must be dense with one memory order")


def _one_memory_order(e: torch.Tensor, x: torch.Tensor) -> bool:
    """Both contiguous, or the same shape and (dense) strides: element ``i`` in memory is the same leaf entry."""
    if e.is_contiguous() and x.is_contiguous():
        return True
    if e.shape != x.shape or e.stride() != x.stride():
        return False
    expect = 1
    for st, n in sorted(zip(x.stride(), x.shape)):
        if n != 1 and st != expect:
            return False
        expect *= n
    return True


def ema_(emas, srcs, *, decay: float | None = None, dev_block: torch.Tensor | None = None,
         dev_skip: torch.Tensor | None = None) -> None:
    """In-place fused exponential moving average over lists of tensors (``optim_ema.hip``):
    ``e <- e + omd * (x - e)`` per element, in this form (``x == e`` keeps ``e``'s bits), computed in
    fp32 (fp64 for fp64 sources). ``srcs``: the fp32 masters where a leaf has one, else the parameters
    (fp32, bf16, fp16, fp64); ``emas``: fp32 (fp64 sources: fp64) tensors of the same sizes, else
    ``TypeError``. One launch per 24 leaves of a source dtype; leaves without elements are skipped.

    ``omd = 1 - decay`` from the host, or, with ``dev_block`` (:func:`ema_block`, advanced by
    :func:`ema_advance_`), the block's: the device value wins, and a block whose ``hold`` word is set
    calls the launch off. ``dev_skip``: as in :func:`adam_`. A launch that is called off reads and
    writes no tensor. No host read: graph-capturable."""
    emas, srcs = list(emas), list(srcs)
    _ema_check(emas, srcs)
    if dev_block is None and decay is None:
        raise ValueError("ema_: needs decay or dev_block")
    if dev_block is not None:
        _ema_block_ok(dev_block, "ema_")
    if not emas:
        return
    if not emas[0].is_cuda:
        ema_reference_(emas, srcs, decay=decay, dev_block=dev_block, dev_skip=dev_skip)
        return
    E = _ext.get(required=True)
    stream = torch.cuda.current_stream(emas[0].device).cuda_stream
    omd = 1.0 - float(decay) if decay is not None else 0.0
    groups: dict = {}
    for e, x in zip(emas, srcs):
        if e.numel():
            groups.setdefault(x.dtype, []).append((e, x))
    for xd, leaves in groups.items():
        E.mt_ema([e.data_ptr() for e, _ in leaves], [x.data_ptr() for _, x in leaves], [e.numel() for e, _ in leaves],
                 DTYPE_CODE[xd], omd, _ptr(dev_block), _skip_ptr(dev_skip), stream)


def ema_reference_(emas, srcs, *, decay=None, dev_block=None, dev_skip=None) -> None:
    """PyTorch reference of :func:`ema_`: the same expression, three roundings in the compute type.
    The CPU path of the engine and the kernel's oracle."""
    emas, srcs = list(emas), list(srcs)
    _ema_check(emas, srcs)
    if _skipped(dev_skip):
        return
    if dev_block is not None:
        _ema_block_ok(dev_block, "ema_reference_")
        if int(dev_block[EMA_HOLD]) != 0:
            return
        omd = dev_block.view(torch.float32)[EMA_OMD].detach().cpu()
    else:
        omd = torch.tensor(1.0 - float(decay), dtype=torch.float64)
    with torch.no_grad():
        for e, x in zip(emas, srcs):
            if e.numel():
                d = x.to(e.dtype) - e
                e.add_(omd.to(device=e.device, dtype=e.dtype) * d)


def ema_advance_(block: torch.Tensor, *, decay: float, warmup: bool, every: int,
                 dev_skip: torch.Tensor | None = None) -> None:
    """The EMA block's bookkeeping after an optimiser step's :func:`ema_` launches, one thread on the
    device. Nothing changes when ``dev_skip`` is non-zero (a skipped step does not count). The step
    was an EMA step (``hold == 0``): ``n += 1``, ``k = 0``; else ``k += 1``. Then, for the coming
    step, ``hold = k + 1 < every``, ``d_t = min(decay, (1 + n) / (10 + n))`` (``warmup``; else
    ``decay``) and ``omd = 1 - d_t``. No host read: graph-capturable."""
    _ema_block_ok(block, "ema_advance_")
    if int(every) < 1:
        raise ValueError(f"ema_advance_: every must be >= 1, got {every}")
    if block.is_cuda:
        _ext.get(required=True).ema_advance(block.data_ptr(), float(decay), int(bool(warmup)), int(every),
                                            _skip_ptr(dev_skip), torch.cuda.current_stream(block.device).cuda_stream)
        return
    ema_advance_reference_(block, decay=decay, warmup=warmup, every=every, dev_skip=dev_skip)


def ema_advance_reference_(block: torch.Tensor, *, decay, warmup, every, dev_skip=None) -> None:
    """PyTorch reference of :func:`ema_advance_` on a CPU block, in fp32 as the kernel computes."""
    _ema_block_ok(block, "ema_advance_reference_")
    if int(every) < 1:
        raise ValueError(f"ema_advance_reference_: every must be >= 1, got {every}")
    if _skipped(dev_skip):
        return
    n, k = int(block[EMA_UPDATES]), int(block[EMA_SINCE])
    if int(block[EMA_HOLD]) == 0:
        n, k = n + 1, 0
    else:
        k += 1
    f = block.view(torch.float32)
    f[EMA_DECAY] = _ema_decay_at(decay, warmup, n)
    f[EMA_OMD] = 1.0 - f[EMA_DECAY]
    block[EMA_UPDATES], block[EMA_SINCE] = n, k
    block[EMA_HOLD] = 1 if k + 1 < int(every) else 0


def sumsq_reference(grads) -> torch.Tensor:
    """fp64 CPU sums of squares of ``grads`` (the oracle of :func:`sumsq_`)."""
    return torch.stack([g.detach().cpu().double().pow(2).sum() for g in grads]) if grads else torch.zeros(0, dtype=torch.float64)


def clip_scales_reference(sumsq: torch.Tensor, omega: float, grad_scale: float = 1.0) -> torch.Tensor:
    """``min(1, omega / (grad_scale * sqrt(sumsq)))`` as the rule writes it (``optimisers.ClipNorm``)."""
    return torch.clamp(omega / (grad_scale * torch.sqrt(sumsq)), max=1.0)


def clip_total_(sumsq: torch.Tensor, slot: torch.Tensor, *, accumulate: bool = False, omega: float = 0.0,
                grad_scale: float = 1.0, dev_pre: torch.Tensor | None = None) -> None:
    """Fold per-leaf sums of squares into the fp32 device slot ``[sum, norm, scale]``:
    ``slot[0] = (slot[0] if accumulate else 0) + sum(sumsq)`` (fixed order), ``slot[1] = grad_scale *
    sqrt(slot[0])`` (the global gradient norm) and ``slot[2] = min(1, omega / slot[1])`` (1 when
    ``omega <= 0``). ``slot[2:3]`` is the ``dev_gscale`` of a global-norm clipped update. With
    ``dev_pre`` (one fp32 on the device, the inverse loss scale) ``slot[1]`` and ``slot[2]`` are
    multiplied by it: the norm of the unscaled gradient, and one scalar that unscales and clips."""
    if slot.dtype != torch.float32 or slot.numel() < 3 or not slot.is_contiguous():
        raise TypeError("clip_total_: slot is a contiguous fp32 tensor of 3 entries")
    if sumsq.dtype not in (torch.float32, torch.float64) or not sumsq.is_contiguous():
        raise TypeError("clip_total_: sumsq is a contiguous fp32 or fp64 tensor")
    if sumsq.is_cuda:
        C = _ext.get(required=True)
        _call(C, "clip_total", sumsq.data_ptr(), sumsq.numel(), DTYPE_CODE[sumsq.dtype], slot.data_ptr(),
              int(bool(accumulate)),
              float(omega), float(grad_scale), torch.cuda.current_stream(sumsq.device).cuda_stream,
              _scaling={"dev_pre": _pre_ptr(dev_pre)})
        return
    total = (slot[0] if accumulate else 0.0) + sumsq.sum().float()
    nrm = grad_scale * torch.sqrt(total)
    pre = dev_pre.reshape(-1)[0] if dev_pre is not None else None
    if pre is not None:
        nrm = nrm * pre
    cs = torch.clamp(omega / nrm, max=1.0) if omega > 0 else torch.ones((), dtype=torch.float32)
    slot[0] = total
    slot[1] = nrm
    slot[2] = cs * pre if pre is not None else cs


def bias_corrections(beta1_t: float, beta2_t: float) -> tuple[float, float]:
    return 1.0 - beta1_t, 1.0 - beta2_t


__all__ = ["adam_", "adam_reference_", "adam_advance_", "sgd_", "sgd_reference_", "supported", "bias_corrections",
           "rule_", "rule_reference_", "RULES",
           "lars_", "lamb_", "lars_reference_", "lamb_reference_", "layerwise_workspace", "LAYERWISE",
           "sumsq_", "sumsq_partials", "sumsq_reference", "clip_scales_reference", "clip_total_",
           "check_finite_", "check_finite_reference_", "loss_scale_block", "loss_scale_update_",
           "loss_scale_update_reference_", "LS_WORDS", "LS_SCALE", "LS_INV", "LS_TRACKER", "LS_SKIPPED", "LS_LAST",
           "LS_FLAG",
           "ema_", "ema_reference_", "ema_block", "ema_advance_", "ema_advance_reference_", "EMA_WORDS", "EMA_OMD",
           "EMA_DECAY", "EMA_UPDATES", "EMA_SINCE", "EMA_HOLD",
           "SR", "SR_WORDS", "sr_block", "sr_advance_", "stochastic_round_", "stochastic_round_reference_"]
