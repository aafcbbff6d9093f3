"""Optimisers.jl-shaped optimiser API on PyTorch tensors.

The reference wraps Optimisers.jl rules (``src/optimizer.jl:16-25``) and its
tests compare state trees leaf by leaf (``test/test_optimizer.jl:13-14``), so
the *state layout* must match Optimisers.jl:

=============  ==============================================  =======================
rule           per-leaf state                                   update ``dx'``
=============  ==============================================  =======================
Descent(η)     ``None``                                         ``η·dx``
Momentum(η,ρ)  ``vel`` (zeros like x)                           ``vel = ρ·vel + η·dx``
Nesterov(η,ρ)  ``vel``                                          ``-ρ²·vel + (1+ρ)·η·dx``
RMSProp(η,ρ,ϵ) ``acc``                                          ``dx·η / (sqrt(acc)+ϵ)``
AdaGrad(η,ϵ)   ``acc`` (filled with ϵ), ``acc += dx²``          ``dx·η / (sqrt(acc)+ϵ)``
Adam(η,β,ϵ)    ``(mt, vt, (β1ᵗ, β2ᵗ))``, βᵗ starts at β         ``mt/(1-β1ᵗ)/(sqrt(vt/(1-β2ᵗ))+ϵ)·η``
AdamW(η,β,γ,ϵ) ``OptimiserChain(Adam, WeightDecay(γ))``         Adam's dx' + γ·x
Lion(η,β)      ``m``, then ``m = β2·m + (1-β2)·dx``             ``η·sign(β1·m + (1-β1)·dx)``
AdaMax(η,β,ϵ)  ``(m, u, βᵗ)``, ``u = max(β2·u, |dx|)``          ``η/(1-β1ᵗ)·m/(u+ϵ)``
AMSGrad(η,β,ϵ) ``(m, v, v̂)`` each filled with ϵ, v̂ = max(v̂,v)  ``η·m/(sqrt(v̂)+ϵ)``
NAdam(η,β,ϵ)   ``(m, v, βᵗ)``                                   ``(β1·m/(1-β1·β1ᵗ) + (1-β1)·dx/(1-β1ᵗ))``
                                                                ``/(sqrt(v·β2/(1-β2ᵗ))+ϵ)·η``
AdaBelief(η,β,ϵ) ``(m, s, βᵗ)``, ``s = β2·s+(1-β2)·(dx-m)²+ϵ``  ``η·m/(1-β1ᵗ)/(sqrt(s/(1-β2ᵗ))+ϵ)``
AdaDelta(ρ,ϵ)  ``(acc, Δ)``, ``Δ = ρ·Δ + (1-ρ)·dx'²``           ``dx·sqrt(Δ+ϵ)/sqrt(acc+ϵ)``
LARS(η,ρ,trust,decay,ϵ) ``vel``; q = trust·‖x‖/(‖dx‖+decay·‖x‖+ϵ)   ``vel = ρ·vel + η·q·(dx + decay·x)``
LAMB(η,β,ϵ,decay) Adam's; u = Adam's dx'/η + decay·x            ``η·‖x‖/‖u‖·u`` (1-D leaves: Momentum / Adam)
WeightDecay(γ) ``None``                                         ``dx + γ·x``
ClipGrad(δ)    ``None``                                         ``clamp(dx, -δ, δ)``
ClipNorm(ω,p)  ``None``                                         ``dx · min(1, ω/‖dx‖ₚ)``
=============  ==============================================  =======================

``setup(rule, model)`` builds a tree of :class:`Leaf` mirroring the model
tree (tied arrays share one Leaf); ``update(state, model, grads)`` is
out-of-place (copies state and model first, like Optimisers.jl) and
``update_`` (Julia's ``update!``) mutates in place. Leaves are *batched*:
``update_`` collects every (leaf, x, dx) first and hands whole batches to
rules that implement ``apply_batch`` — that is where the fused multi-tensor
HIP kernels run on GPU and where :class:`DistributedOptimizer` performs one
bucketed allreduce for all gradients instead of one collective per leaf.
"""
from __future__ import annotations

import copy
import dataclasses
from typing import Any

import numpy as np
import torch

from ..ops import optim as _fused
from ..utils.tree import fmap, is_numeric_array, node_def, register_node


class AbstractRule:
    """Base class of optimisation rules (``Optimisers.AbstractRule``)."""

    def init(self, x: torch.Tensor) -> Any:
        return None

    def apply(self, state, x: torch.Tensor, dx: torch.Tensor):
        """Return ``(new_state, dx')``; ``x -= dx'`` is applied by the caller."""
        raise NotImplementedError

    #: True for rules that issue collectives (``DistributedOptimizer``): every rank must then
    #: hand them the same leaves, so a missing gradient is zero-filled instead of skipped.
    collective = False

    def apply_batch(self, items: list) -> list:
        """``items``: list of ``(leaf, x, dx)``. Returns the ``dx'`` list; updates ``leaf.state``.

        Default: per-leaf :meth:`apply`. Rules override this to fuse.
        Returning ``None`` in place of ``dx'`` means "x already updated in place".
        """
        out = []
        for leaf, x, dx in items:
            leaf.state, d = self.apply(leaf.state, x, dx)
            out.append(d)
        return out

    def __repr__(self):
        fields = ", ".join(f"{k}={v!r}" for k, v in vars(self).items())
        return f"{type(self).__name__}({fields})"


@dataclasses.dataclass(eq=False)
class Leaf:
    """Optimiser state of one array (``Optimisers.Leaf``)."""

    rule: AbstractRule
    state: Any
    frozen: bool = False

    def __repr__(self):
        return f"Leaf({self.rule!r}, {_short(self.state)})"


def _short(s):
    if isinstance(s, torch.Tensor):
        return f"tensor{tuple(s.shape)}"
    if isinstance(s, tuple):
        return "(" + ", ".join(_short(x) for x in s) + ")"
    return repr(s)


# Functors: Leaf's children is its state only (the rule holds hyperparameters).
register_node(Leaf, lambda l: ([l.state], (l.rule, l.frozen)), lambda aux, ch: Leaf(aux[0], ch[0], aux[1]))


def _as_tensor(x):
    if isinstance(x, np.ndarray):
        return torch.from_numpy(x)
    return x


_T_CACHE: dict = {}


def _T(x: torch.Tensor, v: float) -> float:
    """Julia's ``T(η)`` cast (Optimisers.jl rules convert η, β, ϵ to ``eltype(x)``): round a
    hyperparameter to the array's precision — fp32, and for bf16 / fp16 arrays bf16 / fp16
    (``BFloat16(0.9) == 0.8984375``; ``Float16(1e-8) == 0``), exactly as the Julia rule does.
    fp64 (and non-float) arrays keep the double."""
    dt = x.dtype
    if dt not in (torch.float32, torch.bfloat16, torch.float16):
        return float(v)
    key = (dt, v)
    r = _T_CACHE.get(key)
    if r is None:
        r = float(np.float32(v)) if dt == torch.float32 else float(torch.tensor(float(v), dtype=dt))
        if len(_T_CACHE) < 4096:
            _T_CACHE[key] = r
    return r


def _eps(x: torch.Tensor, e: float) -> float:
    """Optimisers.jl's ``_eps(T, ϵ)``: ``T(ϵ)``, except that a Float16 ϵ is floored at
    ``Float16(1e-7)`` (a nonzero ϵ must not round to 0: ``Float16(1e-8) == 0`` would give
    ``0 / (sqrt(0) + 0) = NaN`` on every element whose gradient has been zero so far)."""
    if x.dtype == torch.float16:
        return 0.0 if e == 0 else max(_T(x, 1e-7), _T(x, e))
    return _T(x, e)


# ------------------------------------------------------------------ rules
class Descent(AbstractRule):
    def __init__(self, eta: float = 0.1):
        self.eta = eta

    def apply(self, state, x, dx):
        return state, dx * _T(x, self.eta)

    def apply_batch(self, items):
        return _sgd_batch(self, items, 0.0, False)


class Momentum(AbstractRule):
    def __init__(self, eta: float = 0.01, rho: float = 0.9):
        self.eta, self.rho = eta, rho

    def init(self, x):
        return torch.zeros_like(x)

    def apply(self, vel, x, dx):
        eta, rho = _T(x, self.eta), _T(x, self.rho)
        vel.mul_(rho).add_(dx, alpha=eta)
        return vel, vel

    def apply_batch(self, items):
        return _sgd_batch(self, items, self.rho, False)


class Nesterov(AbstractRule):
    def __init__(self, eta: float = 0.001, rho: float = 0.9):
        self.eta, self.rho = eta, rho

    def init(self, x):
        return torch.zeros_like(x)

    def apply(self, vel, x, dx):
        eta, rho = _T(x, self.eta), _T(x, self.rho)
        newdx = -(rho ** 2) * vel + (1 + rho) * eta * dx
        vel.mul_(rho).sub_(dx, alpha=eta)
        return vel, newdx

    def apply_batch(self, items):
        return _sgd_batch(self, items, self.rho, True)


def _clip_kwargs(clip, x0, gs) -> dict:
    """The fused update's clip arguments for one dtype group (``clip``: a leading ClipNorm(p=2) or
    ClipGrad of a chain, or None). ClipNorm: the deterministic multi-tensor sum of squares and its
    finish write one scale per leaf on the device (two launches per 24 leaves, no host read)."""
    if clip is None:
        return {}
    if isinstance(clip, ClipGrad):
        return {"clip_delta": _T(x0, clip.delta)}
    at = torch.float64 if gs[0].dtype == torch.float64 else torch.float32
    buf = torch.empty(2, len(gs), dtype=at, device=gs[0].device)
    _fused.sumsq_(gs, buf[0], scales=buf[1], omega=clip.omega)
    return {"tscale": buf[1]}


def _sgd_batch(rule, items, rho, nesterov, clip=None):
    """Fused GPU path for Descent / Momentum / Nesterov; per-leaf math elsewhere. ``clip``: the
    chain's leading clip rule, fused into the update on the GPU leaves."""
    gpu = [i for i, (l, x, dx) in enumerate(items)
           if x.is_cuda and dx is not None
           and _same_dense(x, dx, *([l.state] if rho != 0.0 and isinstance(l.state, torch.Tensor) else []))
           and _fused.supported(x.dtype, dx.dtype, x.dtype, False)]
    out: list = [None] * len(items)
    gset = set(gpu)
    for i, (leaf, x, dx) in enumerate(items):
        if i not in gset:
            if clip is not None:
                dx = clip.apply(None, x, dx)[1]
            leaf.state, out[i] = rule.apply(leaf.state, x, dx)
    if gpu:
        by_dtype: dict = {}
        for i in gpu:
            key = items[i][1].dtype if clip is None else (items[i][1].dtype, items[i][2].dtype, items[i][1].device)
            by_dtype.setdefault(key, []).append(i)
        for idx in by_dtype.values():
            x0 = items[idx[0]][1]
            xs = [items[i][1] for i in idx]
            gs = [items[i][2] for i in idx]
            bufs = [items[i][0].state for i in idx] if rho != 0.0 else None
            # hyperparameters rounded to the leaves' precision, as in Julia (``_T``)
            _fused.sgd_(xs, gs, bufs, lr=_T(x0, rule.eta), momentum=_T(x0, rho) if rho else 0.0,
                        nesterov=nesterov, **_clip_kwargs(clip, x0, gs))
    return out


class _KernelRule(AbstractRule):
    """A rule with a fused multi-tensor form in ``ops.optim.rule_`` (``_kind``: its name there)."""

    _kind = ""

    def _tensors(self, state) -> list:
        """The state's tensors in the kernel's slot order."""
        return [state] if isinstance(state, torch.Tensor) else list(state[:_fused.RULES[self._kind][1]])

    def _hyper(self, x=None) -> dict:
        """The kernel's hyperparameters, rounded to ``x``'s precision as ``apply`` does (``_T``,
        ``_eps``); ``x=None``: as given (the DDP engine computes in fp32)."""
        raise NotImplementedError

    def _r(self, x, v):
        return float(v) if x is None else _T(x, v)

    def _e(self, x, v):
        return float(v) if x is None else _eps(x, v)


class _FusedRule(_KernelRule):
    """A kernel rule whose GPU leaves take the fused path in the functional API too."""

    def apply_batch(self, items):
        return _rule_batch(self, items, 0.0)


class RMSProp(_KernelRule):
    _kind = "rmsprop"

    def __init__(self, eta: float = 0.001, rho: float = 0.9, epsilon: float = 1e-8):
        self.eta, self.rho, self.epsilon = eta, rho, epsilon

    def init(self, x):
        return torch.zeros_like(x)

    def apply(self, acc, x, dx):
        eta, rho, eps = _T(x, self.eta), _T(x, self.rho), _eps(x, self.epsilon)
        acc.mul_(rho).addcmul_(dx, dx, value=1 - rho)
        return acc, dx * eta / (torch.sqrt(acc) + eps)

    def _hyper(self, x=None):
        return {"lr": self._r(x, self.eta), "rho": self._r(x, self.rho), "eps": self._e(x, self.epsilon)}


class AdaGrad(_KernelRule):
    _kind = "adagrad"

    def __init__(self, eta: float = 0.1, epsilon: float = 1e-8):
        self.eta, self.epsilon = eta, epsilon

    def init(self, x):
        return torch.full_like(x, self.epsilon)

    def apply(self, acc, x, dx):
        acc.addcmul_(dx, dx)
        return acc, dx * _T(x, self.eta) / (torch.sqrt(acc) + _eps(x, self.epsilon))

    def _hyper(self, x=None):
        return {"lr": self._r(x, self.eta), "eps": self._e(x, self.epsilon)}


class _BetaRule(_FusedRule):
    """Shared by the rules with Adam's hyperparameters ``(η, β, ϵ)``."""

    def __init__(self, eta: float = 0.001, beta: tuple = (0.9, 0.999), epsilon: float = 1e-8):
        self.eta, self.beta, self.epsilon = eta, tuple(beta), epsilon

    def _hyper(self, x=None):
        return {"lr": self._r(x, self.eta), "beta1": self._r(x, self.beta[0]), "beta2": self._r(x, self.beta[1]),
                "eps": self._e(x, self.epsilon)}

    def _cast(self, x):
        return _T(x, self.eta), _T(x, self.beta[0]), _T(x, self.beta[1]), _eps(x, self.epsilon)

    def _bt0(self, x):
        return (_T(x, self.beta[0]), _T(x, self.beta[1]))


class Lion(_FusedRule):
    """``Lion(η=0.001, β=(0.9, 0.999))``; state ``m``."""

    _kind = "lion"

    def __init__(self, eta: float = 0.001, beta: tuple = (0.9, 0.999)):
        self.eta, self.beta = eta, tuple(beta)

    def init(self, x):
        return torch.zeros_like(x)

    def apply(self, m, x, dx):
        eta, b1, b2 = _T(x, self.eta), _T(x, self.beta[0]), _T(x, self.beta[1])
        dxp = eta * torch.sign(b1 * m + (1 - b1) * dx)
        m.mul_(b2).add_(dx, alpha=1 - b2)
        return m, dxp

    def _hyper(self, x=None):
        return {"lr": self._r(x, self.eta), "beta1": self._r(x, self.beta[0]), "beta2": self._r(x, self.beta[1])}


class AdaMax(_BetaRule):
    """``AdaMax(η=0.001, β=(0.9, 0.999), ϵ=1e-8)``; state ``(m, u, βt)``."""

    _kind = "adamax"

    def init(self, x):
        return (torch.zeros_like(x), torch.zeros_like(x), self._bt0(x))

    def apply(self, state, x, dx):
        eta, b1, b2, eps = self._cast(x)
        m, u, bt = state
        m.mul_(b1).add_(dx, alpha=1 - b1)
        torch.maximum(u * b2, dx.abs(), out=u)
        dxp = eta / (1 - bt[0]) * m / (u + eps)
        return (m, u, (_T(x, bt[0] * b1), _T(x, bt[1] * b2))), dxp


class AMSGrad(_BetaRule):
    """``AMSGrad(η=0.001, β=(0.9, 0.999), ϵ=1e-8)``; state ``(m, v, v̂)``, each filled with ϵ."""

    _kind = "amsgrad"

    def init(self, x):
        return (torch.full_like(x, self.epsilon), torch.full_like(x, self.epsilon), torch.full_like(x, self.epsilon))

    def apply(self, state, x, dx):
        eta, b1, b2, eps = self._cast(x)
        m, v, vh = state
        m.mul_(b1).add_(dx, alpha=1 - b1)
        v.mul_(b2).addcmul_(dx, dx, value=1 - b2)
        torch.maximum(vh, v, out=vh)
        return (m, v, vh), eta * m / (torch.sqrt(vh) + eps)


class NAdam(_BetaRule):
    """``NAdam(η=0.001, β=(0.9, 0.999), ϵ=1e-8)``; state ``(m, v, βt)``."""

    _kind = "nadam"

    def init(self, x):
        return (torch.zeros_like(x), torch.zeros_like(x), self._bt0(x))

    def apply(self, state, x, dx):
        eta, b1, b2, eps = self._cast(x)
        m, v, bt = state
        m.mul_(b1).add_(dx, alpha=1 - b1)
        v.mul_(b2).addcmul_(dx, dx, value=1 - b2)
        dxp = (b1 * m / (1 - b1 * bt[0]) + (1 - b1) * dx / (1 - bt[0])) / (torch.sqrt(v * b2 / (1 - bt[1])) + eps) * eta
        return (m, v, (_T(x, bt[0] * b1), _T(x, bt[1] * b2))), dxp


class AdaBelief(_BetaRule):
    """``AdaBelief(η=0.001, β=(0.9, 0.999), ϵ=1e-16)``; state ``(m, s, βt)``."""

    _kind = "adabelief"

    def __init__(self, eta: float = 0.001, beta: tuple = (0.9, 0.999), epsilon: float = 1e-16):
        super().__init__(eta, beta, epsilon)

    def init(self, x):
        return (torch.zeros_like(x), torch.zeros_like(x), self._bt0(x))

    def apply(self, state, x, dx):
        eta, b1, b2, eps = self._cast(x)
        m, s, bt = state
        m.mul_(b1).add_(dx, alpha=1 - b1)
        d = dx - m
        s.mul_(b2).addcmul_(d, d, value=1 - b2).add_(eps)
        dxp = eta * m / (1 - bt[0]) / (torch.sqrt(s / (1 - bt[1])) + eps)
        return (m, s, (_T(x, bt[0] * b1), _T(x, bt[1] * b2))), dxp


class AdaDelta(_FusedRule):
    """``AdaDelta(ρ=0.9, ϵ=1e-7)``; state ``(acc, Δ)``. No learning rate."""

    _kind = "adadelta"

    def __init__(self, rho: float = 0.9, epsilon: float = 1e-7):
        self.rho, self.epsilon = rho, epsilon

    def init(self, x):
        return (torch.zeros_like(x), torch.zeros_like(x))

    def apply(self, state, x, dx):
        rho, eps = _T(x, self.rho), _eps(x, self.epsilon)
        acc, delta = state
        acc.mul_(rho).addcmul_(dx, dx, value=1 - rho)
        dxp = dx * torch.sqrt(delta + eps) / torch.sqrt(acc + eps)
        delta.mul_(rho).addcmul_(dxp, dxp, value=1 - rho)
        return (acc, delta), dxp

    def _hyper(self, x=None):
        return {"rho": self._r(x, self.rho), "eps": self._e(x, self.epsilon)}


class Adam(AbstractRule):
    """``Adam(η=0.001, β=(0.9, 0.999), ϵ=1e-8)``; state ``(mt, vt, βt)``."""

    def __init__(self, eta: float = 0.001, beta: tuple = (0.9, 0.999), epsilon: float = 1e-8):
        self.eta, self.beta, self.epsilon = eta, tuple(beta), epsilon
        self.weight_decay = 0.0  # set by AdamW's fused path only

    def init(self, x):
        return (torch.zeros_like(x), torch.zeros_like(x), (_T(x, self.beta[0]), _T(x, self.beta[1])))

    def apply(self, state, x, dx):
        eta, b1, b2, eps = _T(x, self.eta), _T(x, self.beta[0]), _T(x, self.beta[1]), _eps(x, self.epsilon)
        mt, vt, bt = state
        mt.mul_(b1).add_(dx, alpha=1 - b1)
        vt.mul_(b2).addcmul_(dx, dx, value=1 - b2)
        dxp = mt / (1 - bt[0]) / (torch.sqrt(vt / (1 - bt[1])) + eps) * eta
        return (mt, vt, (_T(x, bt[0] * b1), _T(x, bt[1] * b2))), dxp

    def apply_batch(self, items):
        return _adam_batch(self, items, 0.0)


def _same_dense(*ts) -> bool:
    """All tensors dense (no gaps or overlaps) with identical shape and strides: the flat
    multi-tensor kernels then see matching elements at matching offsets (contiguous, or e.g.
    a channels_last filter with its channels_last gradient and zeros_like moments)."""
    from ..ops.graddst import _dense
    t0 = ts[0]
    if not (t0.is_contiguous() or _dense(t0)):
        return False
    return all(t.shape == t0.shape and t.stride() == t0.stride() for t in ts[1:])


def _leaf_norm(t: torch.Tensor) -> torch.Tensor:
    """L2 norm over the leaf in compute precision (fp32 for bf16 / fp16 leaves)."""
    t = t.float() if t.dtype in (torch.bfloat16, torch.float16) else t
    return torch.sqrt((t * t).sum())


class _LayerwiseRule(AbstractRule):
    """Shared by LARS and LAMB: a leaf with ``x.ndim <= 1`` (biases, norm scales and shifts) is
    neither decayed nor adapted unless ``adapt_1d`` — it takes the base rule (Momentum / Adam) — and
    the adapted GPU leaves take the fused two-phase kernels of ``ops.optim``."""

    adapt_1d = False

    def _adapts(self, x) -> bool:
        return self.adapt_1d or x.ndim > 1

    def _fused_ok(self, leaf, x, dx) -> bool:
        raise NotImplementedError

    def _base_batch(self, items) -> list:
        raise NotImplementedError

    def _fused(self, x0, idx, items) -> None:
        raise NotImplementedError

    def apply_batch(self, items):
        out: list = [None] * len(items)
        base = [i for i, (_, x, _) in enumerate(items) if not self._adapts(x)]
        for i, d in zip(base, self._base_batch([items[i] for i in base]) if base else []):
            out[i] = d
        fused: dict = {}
        for i, (leaf, x, dx) in enumerate(items):
            if not self._adapts(x):
                continue
            if x.is_cuda and dx is not None and self._fused_ok(leaf, x, dx):
                fused.setdefault(self._key(leaf, x, dx), []).append(i)
            else:
                leaf.state, out[i] = self.apply(leaf.state, x, dx)
        for idx in fused.values():
            self._fused(items[idx[0]][1], idx, items)
        return out


class LARS(_LayerwiseRule):
    """``LARS(η=0.1, ρ=0.9, trust=0.001, decay=0, ϵ=0)`` (You et al. 2017); state ``vel``, Momentum's.
    ``q = trust·‖x‖ / (‖dx‖ + decay·‖x‖ + ϵ)`` (1 when either norm is 0), ``vel = ρ·vel +
    η·q·(dx + decay·x)``, ``dx' = vel``."""

    def __init__(self, eta: float = 0.1, rho: float = 0.9, trust: float = 0.001, decay: float = 0.0,
                 epsilon: float = 0.0, adapt_1d: bool = False):
        self.eta, self.rho, self.trust, self.decay, self.epsilon, self.adapt_1d = eta, rho, trust, decay, epsilon, adapt_1d

    def init(self, x):
        return torch.zeros_like(x)

    def apply(self, vel, x, dx):
        if not self._adapts(x):
            return Momentum.apply(self, vel, x, dx)
        eta, rho, trust = _T(x, self.eta), _T(x, self.rho), _T(x, self.trust)
        decay, eps = _T(x, self.decay), _eps(x, self.epsilon)
        xn, gn = _leaf_norm(x), _leaf_norm(dx)
        q = torch.where((xn > 0) & (gn > 0), trust * xn / (gn + decay * xn + eps), torch.ones_like(xn)).to(x.dtype)
        d = dx + decay * x if decay else dx
        vel.mul_(rho).add_(q * d, alpha=eta)
        return vel, vel

    def _fused_ok(self, leaf, x, dx):
        return (isinstance(leaf.state, torch.Tensor) and _same_dense(x, dx, leaf.state)
                and _fused.supported(x.dtype, dx.dtype, leaf.state.dtype, False))

    def _key(self, leaf, x, dx):
        return (x.device, x.dtype, dx.dtype)

    def _base_batch(self, items):
        return _sgd_batch(self, items, self.rho, False)

    def _fused(self, x0, idx, items):
        _fused.lars_([items[i][1] for i in idx], [items[i][2] for i in idx], [items[i][0].state for i in idx],
                     lr=_T(x0, self.eta), momentum=_T(x0, self.rho), trust=_T(x0, self.trust),
                     weight_decay=_T(x0, self.decay), eps=_eps(x0, self.epsilon))


class LAMB(_LayerwiseRule):
    """``LAMB(η=0.001, β=(0.9, 0.999), ϵ=1e-6, decay=0.01)`` (You et al. 2020); state ``(mt, vt, βt)``,
    Adam's. ``u = mt/(1-β1ᵗ)/(sqrt(vt/(1-β2ᵗ))+ϵ) + decay·x``, ``q = ‖x‖/‖u‖`` (1 when either norm is
    0), ``dx' = η·q·u``."""

    def __init__(self, eta: float = 0.001, beta: tuple = (0.9, 0.999), epsilon: float = 1e-6, decay: float = 0.01,
                 adapt_1d: bool = False):
        self.eta, self.beta, self.epsilon, self.decay, self.adapt_1d = eta, tuple(beta), epsilon, decay, adapt_1d

    def init(self, x):
        return (torch.zeros_like(x), torch.zeros_like(x), (_T(x, self.beta[0]), _T(x, self.beta[1])))

    def apply(self, state, x, dx):
        if not self._adapts(x):
            return Adam.apply(self, state, x, dx)
        eta, b1, b2, eps = _T(x, self.eta), _T(x, self.beta[0]), _T(x, self.beta[1]), _eps(x, self.epsilon)
        decay = _T(x, self.decay)
        mt, vt, bt = state
        mt.mul_(b1).add_(dx, alpha=1 - b1)
        vt.mul_(b2).addcmul_(dx, dx, value=1 - b2)
        u = mt / (1 - bt[0]) / (torch.sqrt(vt / (1 - bt[1])) + eps)
        if decay:
            u = u + decay * x
        xn, un = _leaf_norm(x), _leaf_norm(u)
        q = torch.where((xn > 0) & (un > 0), xn / un, torch.ones_like(xn)).to(x.dtype)
        return (mt, vt, (_T(x, bt[0] * b1), _T(x, bt[1] * b2))), (eta * q) * u

    def _fused_ok(self, leaf, x, dx):
        st = leaf.state
        return (isinstance(st, tuple) and len(st) == 3 and _same_dense(x, dx, st[0], st[1])
                and st[0].dtype == st[1].dtype and _fused.supported(x.dtype, dx.dtype, st[0].dtype, False))

    def _key(self, leaf, x, dx):
        return (x.device, x.dtype, dx.dtype, tuple(leaf.state[2]))  # same precision and beta^t -> one call

    def _base_batch(self, items):
        return _adam_batch(self, items, 0.0)

    def _fused(self, x0, idx, items):
        bt = items[idx[0]][0].state[2]
        b1, b2 = _T(x0, self.beta[0]), _T(x0, self.beta[1])
        _fused.lamb_([items[i][1] for i in idx], [items[i][2] for i in idx], [items[i][0].state[0] for i in idx],
                     [items[i][0].state[1] for i in idx], lr=_T(x0, self.eta), beta1=b1, beta2=b2,
                     eps=_eps(x0, self.epsilon), bt1=bt[0], bt2=bt[1], weight_decay=_T(x0, self.decay))
        for i in idx:
            leaf, x = items[i][0], items[i][1]
            m, v, t = leaf.state
            leaf.state = (m, v, (_T(x, t[0] * b1), _T(x, t[1] * b2)))


def _adam_batch(rule: Adam, items, weight_decay: float, clip=None):
    """Fused multi-tensor Adam on GPU leaves (x updated in place, dx' = None). ``clip``: the
    chain's leading clip rule, fused into the update on the GPU leaves (per-leaf elsewhere)."""
    out: list = [None] * len(items)
    fused: dict = {}
    host: dict = {}
    for i, (leaf, x, dx) in enumerate(items):
        ok = (x.is_cuda and dx is not None and isinstance(leaf.state, tuple) and len(leaf.state) == 3
              and _same_dense(x, dx, leaf.state[0], leaf.state[1])
              and _fused.supported(x.dtype, dx.dtype, leaf.state[0].dtype, False))
        if ok:
            key = (x.device, x.dtype, tuple(leaf.state[2]))  # same precision and beta^t -> one launch
            if clip is not None:
                key = (*key, dx.dtype)  # the sum of squares takes one gradient dtype per call
            fused.setdefault(key, []).append(i)
        elif (clip is None and not x.is_cuda and dx is not None and x.dtype in (torch.float32, torch.float64)
              and dx.dtype == x.dtype and isinstance(leaf.state, tuple) and len(leaf.state) == 3
              and leaf.state[0].dtype == x.dtype and x.shape == dx.shape):
            host.setdefault((x.dtype, tuple(leaf.state[2])), []).append(i)
        else:
            if clip is not None:
                dx = clip.apply(None, x, dx)[1]
            st, d = Adam.apply(rule, leaf.state, x, dx)
            if weight_decay:
                d = d + _T(x, weight_decay) * x
            leaf.state, out[i] = st, d
    for (dt, bt), idx in host.items():
        # CPU leaves: the same formulas as Adam.apply, term by term, as multi-tensor (foreach)
        # ops — one dispatch per term for the whole batch instead of ~10 per leaf
        x0 = items[idx[0]][1]
        eta, b1, b2, eps = _T(x0, rule.eta), _T(x0, rule.beta[0]), _T(x0, rule.beta[1]), _eps(x0, rule.epsilon)
        xs = [items[i][1] for i in idx]
        gs = [items[i][2] for i in idx]
        ms = [items[i][0].state[0] for i in idx]
        vs = [items[i][0].state[1] for i in idx]
        torch._foreach_mul_(ms, b1)
        torch._foreach_add_(ms, gs, alpha=1 - b1)
        torch._foreach_mul_(vs, b2)
        torch._foreach_addcmul_(vs, gs, gs, value=1 - b2)
        num = torch._foreach_div(ms, 1 - bt[0])
        den = torch._foreach_div(vs, 1 - bt[1])
        torch._foreach_sqrt_(den)
        torch._foreach_add_(den, eps)
        torch._foreach_div_(num, den)
        torch._foreach_mul_(num, eta)
        if weight_decay:
            torch._foreach_add_(num, xs, alpha=_T(x0, weight_decay))
        for k, i in enumerate(idx):
            leaf = items[i][0]
            m, v, b = leaf.state
            leaf.state = (m, v, (_T(x0, b[0] * b1), _T(x0, b[1] * b2)))
            out[i] = num[k]
    for (_, _, bt, *_), idx in fused.items():
        x0 = items[idx[0]][1]
        xs = [items[i][1] for i in idx]
        gs = [items[i][2] for i in idx]
        ms = [items[i][0].state[0] for i in idx]
        vs = [items[i][0].state[1] for i in idx]
        # hyperparameters rounded to the leaves' precision, as in Julia (``_T``)
        _fused.adam_(xs, gs, ms, vs, lr=_T(x0, rule.eta), beta1=_T(x0, rule.beta[0]), beta2=_T(x0, rule.beta[1]),
                     eps=_eps(x0, rule.epsilon), bc1=1.0 - bt[0], bc2=1.0 - bt[1],
                     weight_decay=_T(x0, weight_decay) if weight_decay else 0.0, **_clip_kwargs(clip, x0, gs))
        for i in idx:
            leaf, x = items[i][0], items[i][1]
            m, v, b = leaf.state
            leaf.state = (m, v, (_T(x, b[0] * _T(x, rule.beta[0])), _T(x, b[1] * _T(x, rule.beta[1]))))
            out[i] = None
    return out


def _rule_batch(rule: _KernelRule, items, weight_decay: float, clip=None):
    """Fused multi-tensor step of a kernel rule on GPU leaves (x updated in place, dx' = None), the
    per-leaf ``apply`` elsewhere; ``weight_decay``: a WeightDecay behind the rule; ``clip`` as in
    :func:`_adam_batch`."""
    _, ns, has_bt = _fused.RULES[rule._kind]
    out: list = [None] * len(items)
    fused: dict = {}
    for i, (leaf, x, dx) in enumerate(items):
        st = leaf.state
        ts = rule._tensors(st) if isinstance(st, (tuple, torch.Tensor)) else []
        ok = (x.is_cuda and dx is not None and len(ts) == ns and all(isinstance(t, torch.Tensor) for t in ts)
              and (not has_bt or len(st) == 3) and _same_dense(x, dx, *ts)
              and all(t.dtype == ts[0].dtype for t in ts) and _fused.supported(x.dtype, dx.dtype, ts[0].dtype, False))
        if ok:
            # same precision and beta^t -> one launch (the sum of squares takes one gradient dtype)
            fused.setdefault((x.device, x.dtype, dx.dtype, tuple(st[2]) if has_bt else None), []).append(i)
        else:
            if clip is not None:
                dx = clip.apply(None, x, dx)[1]
            st, d = rule.apply(st, x, dx)
            if weight_decay:
                d = d + _T(x, weight_decay) * x
            leaf.state, out[i] = st, d
    for (_, _, _, bt), idx in fused.items():
        x0 = items[idx[0]][1]
        xs = [items[i][1] for i in idx]
        gs = [items[i][2] for i in idx]
        per_leaf = [rule._tensors(items[i][0].state) for i in idx]
        kw = rule._hyper(x0)  # rounded to the leaves' precision, as in Julia (``_T``)
        if has_bt:
            kw.update(bt1=bt[0], bt2=bt[1])
        _fused.rule_(rule._kind, xs, gs, [[t[k] for t in per_leaf] for k in range(ns)],
                     weight_decay=_T(x0, weight_decay) if weight_decay else 0.0, **kw, **_clip_kwargs(clip, x0, gs))
        for i in idx:
            leaf, x = items[i][0], items[i][1]
            if has_bt:
                a, b, t = leaf.state
                leaf.state = (a, b, (_T(x, t[0] * _T(x, rule.beta[0])), _T(x, t[1] * _T(x, rule.beta[1]))))
            out[i] = None
    return out


class WeightDecay(AbstractRule):
    def __init__(self, gamma: float = 5e-4):
        self.gamma = gamma

    def apply(self, state, x, dx):
        return state, dx + _T(x, self.gamma) * x


class ClipGrad(AbstractRule):
    def __init__(self, delta: float = 10.0):
        self.delta = delta

    def apply(self, state, x, dx):
        d = _T(x, self.delta)
        return state, torch.clamp(dx, -d, d)


class ClipNorm(AbstractRule):
    def __init__(self, omega: float = 10.0, p: float = 2.0):
        self.omega, self.p = omega, p

    def apply(self, state, x, dx):
        nrm = torch.linalg.vector_norm(dx.float() if dx.dtype in (torch.bfloat16, torch.float16) else dx, self.p)
        scale = torch.clamp(self.omega / nrm, max=1.0).to(dx.dtype)
        return state, dx * scale


class OptimiserChain(AbstractRule):
    """Apply rules in sequence; state is the tuple of member states."""

    def __init__(self, *opts: AbstractRule):
        self.opts = tuple(opts)

    @property
    def collective(self) -> bool:
        return any(getattr(o, "collective", False) for o in self.opts)

    def init(self, x):
        return tuple(o.init(x) for o in self.opts)

    def apply(self, states, x, dx):
        new = []
        for o, s in zip(self.opts, states):
            s, dx = o.apply(s, x, dx)
            new.append(s)
        return tuple(new), dx

    @staticmethod
    def _decays(r, engine: bool = False) -> bool:
        """``r`` takes a fused ``WeightDecay`` behind it (the kernels' ``dx' += γ·x`` epilogue)."""
        return isinstance(r, (Adam, _KernelRule if engine else _FusedRule))

    def _is_adamw(self, engine: bool = False) -> bool:
        return len(self.opts) == 2 and self._decays(self.opts[0], engine) and isinstance(self.opts[1], WeightDecay)

    def fused_plan(self, engine: bool = False):
        """``(clip, inner, where)`` when the chain has a fused batch form, else ``None``.

        ``clip``: a leading ``ClipNorm(p=2)`` / ``ClipGrad`` (or None); ``inner``: the update rule
        — Adam, Lion, AdaMax, AMSGrad, NAdam, AdaBelief or AdaDelta, one of them in a chain with
        WeightDecay, or Descent, Momentum or Nesterov; ``where``: the position of ``inner``'s
        state in the chain's state tuple (None: the tuple itself, the flat ``(clip, rule,
        WeightDecay)`` spelling, whose rule state is ``states[1]``). ``engine``: the plan of the
        DDP engine, which also runs RMSProp and AdaGrad fused (in the functional API a chain
        around them keeps its per-leaf results)."""
        if self._is_adamw(engine):
            return None, self, None
        o = self.opts
        if len(o) < 2 or not (isinstance(o[0], ClipGrad) or (isinstance(o[0], ClipNorm) and o[0].p == 2)):
            return None
        if len(o) == 2 and (type(o[1]) in (Adam, Descent, Momentum, Nesterov)
                            or isinstance(o[1], _KernelRule if engine else _FusedRule)
                            or (isinstance(o[1], OptimiserChain) and o[1]._is_adamw(engine))):
            return o[0], o[1], 1
        if len(o) == 3 and self._decays(o[1], engine) and isinstance(o[2], WeightDecay):
            return o[0], OptimiserChain(o[1], o[2]), None
        return None

    def apply_batch(self, items):
        # Fuse the common shapes into one kernel per dtype group: a rule with a decaying kernel
        # (Adam, Lion, AdaMax, AMSGrad, NAdam, AdaBelief, AdaDelta) then WeightDecay, and a leading
        # ClipNorm(p=2) / ClipGrad in front of such a rule, such a pair, Descent, Momentum or
        # Nesterov (the clip rides in the update kernel; ClipNorm's per-leaf scales come from a
        # multi-tensor sum of squares). The state keeps the chain's tuple-of-member-states layout.
        plan = self.fused_plan()
        if plan is None:
            return AbstractRule.apply_batch(self, items)
        clip, inner, where = plan

        def get(st):
            if clip is None:
                return st
            return st[1] if where == 1 else (st[1], st[2])

        def put(st, new):
            if clip is None:
                return new
            return (st[0], new) if where == 1 else (st[0], new[0], new[1])

        adamw = isinstance(inner, OptimiserChain)
        rule = inner.opts[0] if adamw else inner
        sub = [(Leaf(rule, get(leaf.state)[0] if adamw else get(leaf.state)), x, dx) for leaf, x, dx in items]
        if isinstance(rule, Adam):
            out = _adam_batch(rule, sub, inner.opts[1].gamma if adamw else 0.0, clip)
        elif isinstance(rule, _KernelRule):
            out = _rule_batch(rule, sub, inner.opts[1].gamma if adamw else 0.0, clip)
        else:
            out = _sgd_batch(rule, sub, getattr(rule, "rho", 0.0), isinstance(rule, Nesterov), clip)
        for (leaf, _, _), (sl, _, _) in zip(items, sub):
            leaf.state = put(leaf.state, (sl.state, get(leaf.state)[1]) if adamw else sl.state)
        return out


OptimizerChain = OptimiserChain


def AdamW(eta: float = 0.001, beta: tuple = (0.9, 0.999), decay: float = 0.0, epsilon: float = 1e-8):
    """Optimisers.jl ``AdamW`` = ``OptimiserChain(Adam(η, β, ϵ), WeightDecay(γ))``."""
    return OptimiserChain(Adam(eta, beta, epsilon), WeightDecay(decay))


# ------------------------------------------------------------------ tree API
def setup(rule: AbstractRule, model: Any) -> Any:
    """Build the state tree (``Optimisers.setup``). Tied arrays share one :class:`Leaf`."""
    cache: dict = {}
    keep: list = []

    def walk(x):
        if is_numeric_array(x) and (not isinstance(x, torch.Tensor) or x.is_floating_point()):
            key = id(x)
            if key in cache:
                return cache[key]
            leaf = Leaf(rule, rule.init(_as_tensor(x)))
            cache[key] = leaf
            keep.append(x)
            return leaf
        if isinstance(x, torch.nn.Module):
            return {n: walk(p) for n, p in x.named_parameters()}
        nd = node_def(x)
        if nd is None:
            return None
        ch, aux = nd[0](x)
        return nd[1](aux, [walk(c) for c in ch])

    return walk(model)


def _collect(tree, model, grads):
    """Walk (state, model, grad) in parallel; accumulate grads of tied leaves."""
    items: dict = {}
    order: list = []

    def walk(s, x, g):
        if isinstance(s, Leaf):
            if s.frozen:
                return
            if g is None:
                if not getattr(s.rule, "collective", False):
                    return
                # a rank without a gradient for this leaf still takes part in the
                # collective (the plan comes from the state tree), contributing zeros
                g = torch.zeros_like(_as_tensor(x))
            x_t, g_t = _as_tensor(x), _as_tensor(g)
            if id(s) in items:
                leaf, xx, gg = items[id(s)]
                items[id(s)] = (leaf, xx, gg + g_t)  # tied parameter: sum contributions
            else:
                items[id(s)] = (s, x_t, g_t)
                order.append(id(s))
            return
        if s is None:
            return
        if isinstance(x, torch.nn.Module):
            named = dict(x.named_parameters())
            gd = g if isinstance(g, dict) else {n: p.grad for n, p in named.items()}
            for n, p in named.items():
                walk(s.get(n), p, gd.get(n))
            return
        nd = node_def(s)
        if nd is None:
            return
        sc, _ = nd[0](s)
        xc, _ = node_def(x)[0](x) if node_def(x) is not None else ([x] * len(sc), None)
        if g is None or node_def(g) is None:
            gc = [g] * len(sc)
        else:
            gc, _ = node_def(g)[0](g)
        for a, b, c in zip(sc, xc, gc):
            walk(a, b, c)

    walk(tree, model, grads)
    return [items[k] for k in order]


def update_(tree: Any, model: Any, grads: Any):
    """In-place update (``Optimisers.update!``). Returns ``(tree, model)``."""
    items = _collect(tree, model, grads)
    # group consecutive leaves by rule object so each rule sees one batch
    by_rule: dict = {}
    for it in items:
        by_rule.setdefault(id(it[0].rule), (it[0].rule, []))[1].append(it)
    for rule, batch in by_rule.values():
        dxs = rule.apply_batch(batch)
        for (leaf, x, _), d in zip(batch, dxs):
            if d is None:
                continue
            with torch.no_grad():
                x.sub_(d.to(x.dtype) if d.dtype != x.dtype else d)
    return tree, model


update_inplace = update_


def _copy_tree(t):
    def cp(x):
        if isinstance(x, torch.Tensor):
            return x.detach().clone()
        if isinstance(x, np.ndarray):
            return x.copy()
        return x
    return fmap(cp, t)


def update(tree: Any, model: Any, grads: Any):
    """Out-of-place update (``Optimisers.update``): state and model are copied first."""
    if isinstance(model, torch.nn.Module):
        model = copy.deepcopy(model)
        if not isinstance(grads, dict):
            grads = {n: p.grad for n, p in model.named_parameters()}
    else:
        model = _copy_tree(model)
    tree = _copy_leaves(tree)
    return update_(tree, model, grads)


def _copy_leaves(tree):
    cache: dict = {}

    def walk(s):
        if isinstance(s, Leaf):
            if id(s) not in cache:
                cache[id(s)] = Leaf(s.rule, _copy_tree(s.state), s.frozen)
            return cache[id(s)]
        nd = node_def(s)
        if nd is None:
            return s
        ch, aux = nd[0](s)
        return nd[1](aux, [walk(c) for c in ch])

    return walk(tree)


def freeze_(tree):
    for l in _leaves_of(tree):
        l.frozen = True
    return tree


def thaw_(tree):
    for l in _leaves_of(tree):
        l.frozen = False
    return tree


def adjust_(tree, eta: float | None = None, **kw):
    """Change hyperparameters of every rule in ``tree`` (``Optimisers.adjust!``)."""
    seen = set()
    for l in _leaves_of(tree):
        r = l.rule
        if id(r) in seen:
            continue
        seen.add(id(r))
        _adjust_rule(r, eta, kw)
    return tree


def _adjust_rule(r, eta, kw):
    if isinstance(r, OptimiserChain):
        for o in r.opts:
            _adjust_rule(o, eta, kw)
        return
    inner = getattr(r, "optimizer", None)
    if inner is not None:
        _adjust_rule(inner, eta, kw)
        return
    if eta is not None and hasattr(r, "eta"):
        r.eta = eta
    for k, v in kw.items():
        if hasattr(r, k):
            setattr(r, k, v)


def _leaves_of(tree):
    out: list = []
    seen: set = set()

    def walk(s):
        if isinstance(s, Leaf):
            if id(s) not in seen:
                seen.add(id(s))
                out.append(s)
            return
        nd = node_def(s)
        if nd is None:
            return
        for c in nd[0](s)[0]:
            walk(c)

    walk(tree)
    return out


# ------------------------------------------------------------------ weight EMA
def _ema_of(x):
    """The average's leaf for a model leaf: an fp32 (fp64 leaves: fp64) copy in the leaf's memory
    order, a ``FlatParams`` over such a copy, or ``None`` for what is not averaged."""
    from ..parallel.flat import FlatParams
    if isinstance(x, FlatParams):
        return x.like(_ema_of(x.data))
    if isinstance(x, torch.Tensor) and x.is_floating_point():
        return x.detach().to(torch.float64 if x.dtype == torch.float64 else torch.float32, copy=True)
    return None


def ema_setup(ps: Any) -> Any:
    """The start of an exponential moving average of ``ps`` (a pytree, a ``FlatParams`` or a module):
    the same tree with every floating-point tensor replaced by an fp32 (fp64 leaves: fp64) copy and
    every other leaf by ``None``. Tied leaves share one copy."""
    if isinstance(ps, torch.nn.Module):
        ps = dict(ps.named_parameters())
    return fmap(_ema_of, ps)


def ema_update(ema: Any, ps: Any, decay: float, *, num_updates: int | None = None) -> Any:
    """``e <- e + (1 - d) (x - e)`` for every leaf of ``ema`` (:func:`ema_setup`) and the matching leaf
    of ``ps``, in place; returns ``ema``. ``d = decay``, or with ``num_updates`` (the updates done
    before this one) the warmed-up ``min(decay, (1 + n) / (10 + n))``. GPU leaves run on the fused
    multi-tensor kernel (``ops.optim.ema_``: 24 leaves per launch, computed in fp32 / fp64 from the
    leaf as it is stored), CPU leaves on the same expression in torch ops."""
    from ..parallel.flat import FlatParams
    if isinstance(decay, bool) or not 0.0 <= decay < 1.0:
        raise ValueError(f"ema_update: need 0 <= decay < 1, got {decay!r}")
    d = float(decay)
    if num_updates is not None:
        if num_updates < 0:
            raise ValueError(f"ema_update: num_updates counts the updates done so far, got {num_updates}")
        d = min(d, (1.0 + num_updates) / (10.0 + num_updates))
    if isinstance(ps, torch.nn.Module):
        ps = dict(ps.named_parameters())
    by_dev: dict = {}

    def pair(e, x):
        if isinstance(e, FlatParams):
            e, x = e.data, x.data
        if isinstance(e, torch.Tensor):
            if not isinstance(x, torch.Tensor):
                raise TypeError(f"ema_update: an averaged leaf meets {type(x).__name__} in the model")
            es, xs = by_dev.setdefault(e.device, ([], []))
            es.append(e)
            xs.append(x.detach())
        return e

    fmap(pair, ema, ps)
    for es, xs in by_dev.values():
        _fused.ema_(es, xs, decay=d)
    return ema


__all__ = [
    "ema_setup", "ema_update",
    "AbstractRule", "Leaf", "Descent", "Momentum", "Nesterov", "RMSProp", "AdaGrad", "Adam", "AdamW",
    "Lion", "AdaMax", "AMSGrad", "NAdam", "AdaBelief", "AdaDelta", "LARS", "LAMB",
    "WeightDecay", "ClipGrad", "ClipNorm", "OptimiserChain", "OptimizerChain", "setup", "update", "update_",
    "update_inplace", "freeze_", "thaw_", "adjust_",
]
