"""Inputs, float64 references with derived per-element bounds, fp32 emulations and planted defects for
the fused optimiser kernels (``csrc/kernels/optim.hip``, ``optim_rules.hip``, ``optim_layerwise.hip``).
No fixtures, no tests: ``test_optim_edges_gpu.py`` drives it. Nothing here reads the extension.

One program per rule
--------------------
Each update rule is written ONCE (``_rule``, ``_grad``, the ``_lars_*`` / ``_lamb_*`` pieces), from the
formula tables in the headers of the three ``.hip`` files (the Optimisers.jl forms), over an arithmetic
object ``A``. Three arithmetics evaluate the same text:

* ``Tracked(u)``: values-with-error ``V(val, err)`` in float64 tensors. ``val`` is the float64 result,
  ``err`` the first-order forward error of an evaluation in the compute type with unit roundoff ``u``
  (2^-24 for bf16 / fp16 / fp32 leaves, 2^-53 for fp64 leaves). This is the reference AND the bound.
* ``Plain(torch.float64)``: the float64 closed form of the exact cases.
* ``Plain(torch.float32)``: the fp32 emulation that the planted defects are applied to
  (``emulate``). The project's own CPU paths (``adam_reference_`` ...) are the other emulation.

Charges of ``V``: every ``+ - *`` costs ``u |result|`` on top of the propagated input errors (an fma is
charged as a multiply and an add, so the bound does not depend on contraction); every ``/`` and
``sqrt`` costs ``2u |result|`` and propagates its input errors through the interval ends (``sqrt`` of
``[max(v - e, 0), v + e]``, a quotient by the end of ``[|b| - e_b, |b| + e_b]`` nearer zero), which keeps
``v = 0``, ``acc = 0`` and ``u = 0`` finite; ``max``, ``abs`` and ``clamp`` are 1-Lipschitz (``err =
max(...)`` or unchanged). The prologue ``g = clamp(g_in * (gs [* dev_gscale]) [* tscale], +-delta)``
and the epilogue ``dx += wd * x; x -= dx`` (SGD: ``g += wd * x``) are part of the tracked program. A
stored output of dtype T gets ``u_T |val|`` on top (``norm_edges.UT``; fp64: 2^-53; fp16 also the 2^-25
subnormal term), and every bound gets 1e-30. Nothing is fitted to kernel output.

Which scalar values the reference takes
---------------------------------------
Tensor inputs: the values the device holds (the tensors are made on the CPU in their device dtype, or
copied back before the launch). ``grad_scale`` and ``clip_delta`` are ``float`` in ``api.h``: their
float32 roundings. The device blocks ``dev_hyper`` / ``dev_lr`` / ``dev_gscale`` are fp32 by design: their
fp32 contents (Adam then forms ``1 - beta^t`` in the compute type, one charged subtraction). ``tscale``:
its stored value. Everything else: the caller's Python double for fp64 leaves, its float32 rounding for
fp32-compute leaves (the kernels round once). ``1 - beta`` is a charged subtraction in the compute type.

Checks
------
Master combinations: the master is held to the compute-precision bound and the low-precision parameter
must equal ``master.to(P)`` bit for bit. No master: the parameter is held to ``err_x + u_T |x|``.
Lion: where ``|b1 m + (1 - b1) g| <= err`` the sign is undecided; there ``x`` may be the value of any
computed sign (+1, -1, or 0 when the computed argument is exactly zero), the state is still bounded,
and at most ``UNDECIDED_CAP`` of a case may be undecided (a condition on the inputs, asserted for the
reference alone by a CPU test).
LARS / LAMB: (1) the ratio the kernel stored against the float64 ratio. Each of the two sums of squares
is bounded by ``sum err(t) + L E sum |t|`` with E = 2^-23 (fp64: 2^-52) per addition and

    L(n) = 16 + 9 + ceil(nb / 256) + 9,   nb = ceil(n / 4096)

(one thread's kVec * kIters = 16 additions over its chunk; the workgroup sum, 6 wave levels and 3 wave
totals; the fixed-order fold of ceil(nb / 256) partials per thread; its workgroup sum — a closed form
that may over-count), pushed through ``sqrt`` and the quotient by ``V``. (2) The element update with the
device's own stored ratio as an input; for LAMB the device's stored ``m``, ``v`` are inputs too (``u``
is formed from the stored moments), and ``m`` / ``v`` are checked against their own bound from the
inputs. Multi-step runs do not compound bounds: the second step's reference starts from what was stored
after the first.
"""
import math

import torch

from . import mfma_edges as E
from .mfma_edges import TINY
from .norm_edges import SUB, UT

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
U_T = {**UT, F64: 2.0 ** -53}
SUB_T = {**SUB, F64: 0.0}
UNDECIDED_CAP = 1e-3
CLAMP_SHARE = (0.3, 0.7)

# (parameter, gradient, state, fp32 master): the 11 combinations the kernels are built for
COMBOS = [
    (F32, F32, F32, False), (F32, BF16, F32, False), (BF16, BF16, BF16, False), (BF16, BF16, F32, False),
    (BF16, BF16, F32, True), (BF16, F32, F32, True), (F16, F16, F16, False), (F16, F16, F32, False),
    (F16, F16, F32, True), (F16, F32, F32, True), (F64, F64, F64, False),
]
_N = {F32: "fp32", F64: "fp64", BF16: "bf16", F16: "fp16"}


def combo_id(c):
    return f"{_N[c[0]]}-{_N[c[1]]}-{_N[c[2]]}{'-master' if c[3] else ''}"


PATH_COMBOS = [COMBOS[0], COMBOS[4], COMBOS[6]]  # fp32, bf16 + master, fp16 / fp16 / fp16

RULES = ["adam", "adamw", "descent", "momentum", "nesterov", "rmsprop", "adagrad", "lion", "adamax", "amsgrad",
         "nadam", "adabelief", "adadelta", "lars", "lamb"]
SGD = ("descent", "momentum", "nesterov")
LAYERWISE = ("lars", "lamb")
# state slots by what they hold: m (signed, ~g), v (>= 0, ~g^2), u (>= 0, ~|g|), buf (signed velocity), D (AdaDelta)
SLOTS = {"adam": "mv", "adamw": "mv", "descent": "", "momentum": "b", "nesterov": "b", "rmsprop": "v", "adagrad": "v",
         "lion": "m", "adamax": "mu", "amsgrad": "mvV", "nadam": "mv", "adabelief": "mv", "adadelta": "vD",
         "lars": "b", "lamb": "mv"}
READS_BT = ("adam", "adamw", "adamax", "nadam", "adabelief", "lamb")
HYPER = {
    "adam": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0),
    "adamw": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01),
    "descent": dict(lr=0.1, b1=0.0, b2=0.0, eps=0.0, wd=0.01),
    "momentum": dict(lr=0.1, b1=0.9, b2=0.0, eps=0.0, wd=0.01),
    "nesterov": dict(lr=0.1, b1=0.9, b2=0.0, eps=0.0, wd=0.01),
    "rmsprop": dict(lr=1e-3, b1=0.9, b2=0.0, eps=1e-8, wd=0.01),
    "adagrad": dict(lr=0.1, b1=0.0, b2=0.0, eps=1e-8, wd=0.01),
    "lion": dict(lr=1e-3, b1=0.9, b2=0.99, eps=0.0, wd=0.01),
    "adamax": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01),
    "amsgrad": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01),
    "nadam": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01),
    "adabelief": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-16, wd=0.01),
    "adadelta": dict(lr=0.0, b1=0.9, b2=0.0, eps=1e-7, wd=0.01),
    "lars": dict(lr=0.1, b1=0.9, b2=0.02, eps=1e-9, wd=0.01),     # b1: momentum, b2: trust
    "lamb": dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-6, wd=0.01),
}
FAMILIES = ("uniform", "first_step", "t1000", "tiny", "big_x", "clipped")


def ct_of(pd):
    return F64 if pd == F64 else F32


def rt(dtype, v):
    """Rounding of ``v`` to a stored value of ``dtype``."""
    return U_T[dtype] * v.abs() + SUB_T[dtype]


def lw_L(n):
    """Additions on the longest path of a layer-wise sum of squares over ``n`` elements (docstring)."""
    nb = -(-n // 4096)
    return 16 + 9 + -(-nb // 256) + 9


# ------------------------------------------------------------------------------------ the value-with-error type

class V:
    __slots__ = ("val", "err", "u")

    def __init__(self, val, err, u):
        self.val, self.err, self.u = val, err, u

    def _l(self, o):
        if isinstance(o, V):
            return o
        t = torch.as_tensor(o, dtype=F64)
        return V(t, torch.zeros_like(t), self.u)

    def __add__(self, o):
        o = self._l(o)
        val = self.val + o.val
        return V(val, self.err + o.err + self.u * val.abs(), self.u)

    __radd__ = __add__

    def __neg__(self):
        return V(-self.val, self.err, self.u)

    def __sub__(self, o):
        return self + (-self._l(o))

    def __rsub__(self, o):
        return self._l(o) + (-self)

    def __mul__(self, o):
        o = self._l(o)
        val = self.val * o.val
        return V(val, self.val.abs() * o.err + o.val.abs() * self.err + self.err * o.err + self.u * val.abs(), self.u)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._l(o)
        val = self.val / o.val
        lo = o.val.abs() - o.err  # the end of the divisor's interval nearer zero
        err = (self.err + val.abs() * o.err) / lo
        err = torch.where(lo > 0, err, torch.full_like(err, math.inf))
        err = torch.where((self.err == 0) & (o.err == 0), torch.zeros_like(err), err)
        return V(val, err + 2 * self.u * val.abs(), self.u)

    def sqrt(self):
        val = torch.sqrt(self.val)
        hi = torch.sqrt(self.val + self.err) - val
        lo = val - torch.sqrt(torch.clamp(self.val - self.err, min=0))
        return V(val, torch.maximum(hi, lo) + 2 * self.u * val, self.u)


class Tracked:
    """Arithmetic over ``V``. ``force``: the sign Lion takes where its argument is undecided."""

    def __init__(self, u, force=0.0):
        self.u, self.force, self.undecided = u, force, None

    def c(self, v):
        t = torch.as_tensor(v, dtype=F64)
        return V(t, torch.zeros_like(t), self.u)

    def lift(self, t):
        return self.c(t.to(F64))

    def sqrt(self, x):
        return x.sqrt()

    def abs(self, x):
        return V(x.val.abs(), x.err, x.u)

    def max(self, a, b):
        return V(torch.maximum(a.val, b.val), torch.maximum(a.err, b.err), a.u)

    def clamp(self, x, d):
        return V(torch.clamp(x.val, -d, d), x.err, x.u)

    def sign(self, a):
        und = a.val.abs() <= a.err
        self.undecided = und
        s = torch.where(und, torch.full_like(a.val, self.force), torch.sign(a.val))
        return V(s, torch.zeros_like(s), a.u)

    def stored(self, x, dtype):  # never used: the checks feed the device's stored moments
        raise NotImplementedError

    def segsum(self, t, idx, n, sizes):
        """Per-leaf sums of a per-element V with the summation bound L E sum|t|."""
        val = torch.zeros(n, dtype=F64).index_add_(0, idx, t.val)
        err = torch.zeros(n, dtype=F64).index_add_(0, idx, t.err)
        ab = torch.zeros(n, dtype=F64).index_add_(0, idx, t.val.abs())
        L = torch.tensor([lw_L(s) for s in sizes], dtype=F64)
        return V(val, err + L * (2 * self.u) * ab, self.u)

    def where(self, c, a, b):
        b = a._l(b)
        return V(torch.where(c, a.val, b.val), torch.where(c, a.err, b.err), a.u)

    def value(self, x):
        return x.val


class Plain:
    """Arithmetic over plain tensors of one dtype: float64 (the closed form of the exact cases) or
    float32 (the emulation). ``trunc``: stores truncate (a planted defect)."""

    def __init__(self, dtype, trunc=False, unrounded=False):
        self.dt, self.trunc, self.unrounded = dtype, trunc, unrounded

    def c(self, v):
        return torch.as_tensor(v, dtype=F64).to(self.dt)

    def lift(self, t):
        return t.to(self.dt)

    def sqrt(self, x):
        return torch.sqrt(x)

    def abs(self, x):
        return x.abs()

    def max(self, a, b):
        return torch.maximum(a, b)  # either operand NaN -> NaN, as the kernels' nan_max

    def clamp(self, x, d):
        return torch.clamp(x, -d, d)

    def sign(self, a):  # 0 -> 0, NaN -> NaN
        return torch.where(a > 0, torch.ones_like(a), torch.where(a < 0, -torch.ones_like(a), a * 0))

    def stored(self, x, dtype):
        if self.unrounded or self.dt == F64:
            return x
        return store(x, dtype, self.trunc).to(self.dt)

    def segsum(self, t, idx, n, sizes):  # one rounding of the float64 sum: a tree's accuracy, not a running sum's
        return torch.zeros(n, dtype=F64).index_add_(0, idx, t.to(F64)).to(self.dt)

    def where(self, c, a, b):
        return torch.where(c, a, torch.as_tensor(b, dtype=self.dt))

    def value(self, x):
        return x


def store(x, dtype, trunc=False):
    """``x`` (compute type) as a stored ``dtype``: round to nearest even, or truncated toward zero."""
    r = x.to(dtype)
    if trunc and dtype in (BF16, F16):
        over = r.to(x.dtype).abs() > x.abs()
        r = torch.where(over, (r.view(torch.int16) - 1).view(dtype), r)  # one step toward zero
    return r


# ------------------------------------------------------------------------------------ the rules, written once

def resolve(case, ct):
    """The scalar values the compute sees (module docstring)."""
    f32 = lambda v: float(torch.tensor(v, dtype=F32))
    r = float if ct == F64 else f32
    dev = bool(case.get("dev"))
    h = {k: r(case[k]) for k in ("b1", "b2", "eps", "wd")}
    h["dev"] = dev
    for k in ("lr", "bt1", "bt2"):
        h[k] = f32(case[k]) if dev and (k == "lr" or case["rule"] in READS_BT) else r(case[k])
    h["bc1"], h["bc2"] = r(1.0 - case["bt1"]), r(1.0 - case["bt2"])  # Adam's host arguments
    h["gs"] = f32(case["gs"])
    h["dgs"] = None if case.get("dgs") is None else f32(case["dgs"])
    h["delta"] = f32(case.get("delta", 0.0))
    return h


def _grad(A, g_in, h, ts, defect=None):
    s = A.c(h["gs"])
    if h["dgs"] is not None:
        s = s * A.c(h["dgs"])
    if defect == "scale_after_clamp" and h["delta"]:
        g = g_in if ts is None else g_in * ts
        return A.clamp(g, h["delta"]) * s
    g = g_in * s
    if ts is not None:
        g = g * ts
    if h["delta"]:
        g = A.clamp(g, h["delta"])
    return g


def _rule(A, rule, g, x, s, h, defect=None, x_wd=None):
    """(new x, new states) of one step of a per-element rule; ``x_wd``: what weight decay reads."""
    c = A.c
    lr, b1, b2, eps, wd = c(h["lr"]), c(h["b1"]), c(h["b2"]), c(h["eps"]), h["wd"]
    x_wd = x if x_wd is None else x_wd
    s = list(s)
    if rule in SGD:
        if wd and defect != "wd_on_dx":
            g = g + c(wd) * x_wd
        if rule == "descent":
            dx = g * lr
        elif rule == "momentum":
            s[0] = b1 * s[0] + lr * g
            dx = s[0]
        else:
            dx = -(b1 * b1) * s[0] + (1.0 + b1) * lr * g
            s[0] = b1 * s[0] + lr * g if defect == "nesterov_sign" else b1 * s[0] - lr * g
        if wd and defect == "wd_on_dx":
            dx = dx + c(wd) * x_wd
        return x - dx, s
    if rule in ("adam", "adamw"):
        s[0] = b1 * s[0] + (1.0 - b1) * g
        s[1] = b2 * s[1] + (1.0 - b2) * (g * g)
        bc1, bc2 = (1.0 - c(h["bt1"]), 1.0 - c(h["bt2"])) if h["dev"] else (c(h["bc1"]), c(h["bc2"]))
        if defect == "eps_in_sqrt":
            dx = s[0] / bc1 / A.sqrt(s[1] / bc2 + eps) * lr
        else:
            dx = s[0] / bc1 / (A.sqrt(s[1] / bc2) + eps) * lr
    elif rule == "rmsprop":
        s[0] = b1 * s[0] + (1.0 - b1) * (g * g)
        dx = g * lr / (A.sqrt(s[0]) + eps)
    elif rule == "adagrad":
        s[0] = s[0] + g * g
        dx = g * lr / (A.sqrt(s[0]) + eps)
    elif rule == "lion":
        if defect == "lion_m_first":
            s[0] = b2 * s[0] + (1.0 - b2) * g
            dx = lr * A.sign(b1 * s[0] + (1.0 - b1) * g)
        else:
            a = b1 * s[0] + (1.0 - b1) * g
            s[0] = b2 * s[0] + (1.0 - b2) * g
            dx = lr * A.sign(a)
    elif rule == "adamax":
        s[0] = b1 * s[0] + (1.0 - b1) * g
        s[1] = A.max(b2 * s[1], A.abs(g))
        dx = lr / (1.0 - c(h["bt1"])) * s[0] / (s[1] + eps)
    elif rule == "amsgrad":
        v_old = s[1]
        s[0] = b1 * s[0] + (1.0 - b1) * g
        s[1] = b2 * s[1] + (1.0 - b2) * (g * g)
        s[2] = A.max(s[2], v_old if defect == "vhat_old_v" else s[1])
        dx = lr * s[0] / (A.sqrt(s[2]) + eps)
    elif rule == "nadam":
        bt1, bt2 = c(h["bt1"]), c(h["bt2"])
        s[0] = b1 * s[0] + (1.0 - b1) * g
        s[1] = b2 * s[1] + (1.0 - b2) * (g * g)
        num = b1 * s[0] / (1.0 - b1 * bt1) + (1.0 - b1) * g / (1.0 - bt1)
        dx = num / (A.sqrt(s[1] * b2 / (1.0 - bt2)) + eps) * lr
    elif rule == "adabelief":
        s[0] = b1 * s[0] + (1.0 - b1) * g
        d = g - s[0]
        s[1] = b2 * s[1] + (1.0 - b2) * (d * d) + eps
        dx = lr * s[0] / (1.0 - c(h["bt1"])) / (A.sqrt(s[1] / (1.0 - c(h["bt2"]))) + eps)
    elif rule == "adadelta":
        s[0] = b1 * s[0] + (1.0 - b1) * (g * g)
        dx = g * A.sqrt(s[1] + eps) / A.sqrt(s[0] + eps)
        if defect != "delta_post_decay":
            s[1] = b1 * s[1] + (1.0 - b1) * (dx * dx)
    else:
        raise ValueError(rule)
    if wd:
        dx = dx + (c(wd) * lr if defect == "wd_times_lr" else c(wd)) * x_wd
    if rule == "adadelta" and defect == "delta_post_decay":
        s[1] = b1 * s[1] + (1.0 - b1) * (dx * dx)
    return x - dx, s


def _lamb_moments(A, g, m, v, h):
    b1, b2 = A.c(h["b1"]), A.c(h["b2"])
    return b1 * m + (1.0 - b1) * g, b2 * v + (1.0 - b2) * (g * g)


def _lamb_u(A, m, v, x, h):
    u = m / (1.0 - A.c(h["bt1"])) / (A.sqrt(v / (1.0 - A.c(h["bt2"]))) + A.c(h["eps"]))
    return u + A.c(h["wd"]) * x if h["wd"] else u


def _ratio(A, rule, sx, sy, h):
    xn, yn = A.sqrt(sx), A.sqrt(sy)
    q = xn / yn if rule == "lamb" else A.c(h["b2"]) * xn / (yn + A.c(h["wd"]) * xn + A.c(h["eps"]))
    return A.where((A.value(xn) > 0) & (A.value(yn) > 0), q, 1.0)


def _lars_apply(A, g, x, vel, q, h):
    d = g + A.c(h["wd"]) * x if h["wd"] else g
    vel = A.c(h["b1"]) * vel + A.c(h["lr"]) * (q * d)
    return x - vel, vel


def _lamb_apply(A, x, u, q, h):
    return x - (A.c(h["lr"]) * q) * u


# ------------------------------------------------------------------------------------ one step over a whole call

def _flat(ts):
    return torch.cat([t.reshape(-1) for t in ts]) if ts else torch.zeros(0)


def _split(t, sizes):
    return list(torch.split(t, sizes))


def _leaf_idx(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def _step(A, case, combo, inp, defect=None, q_in=None, mv_in=None):
    """One step over the concatenated leaves of ``inp`` in arithmetic ``A``. Returns a dict of flat results:
    ``x``, ``st`` (list), and for the layer-wise rules ``q`` (per leaf, from the inputs). ``q_in`` (per
    leaf) / ``mv_in`` (flat m, v): the device's stored ratio / moments as inputs of the element update."""
    rule, (pd, gd, sd, master) = case["rule"], combo
    sizes = [t.numel() for t in inp["p"]]
    h = resolve(case, ct_of(pd))
    idx = _leaf_idx(sizes)
    g_in = A.lift(_flat(inp["g"]))
    x = A.lift(_flat(inp["w"] if master else inp["p"]))
    st = [A.lift(_flat(s)) for s in inp["st"]]
    ts = None if case.get("ts") is None or rule in LAYERWISE else A.lift(case["ts"][idx])
    if rule not in LAYERWISE:
        g = _grad(A, g_in, h, ts, defect)
        x_wd = A.lift(_flat(inp["p"])) if defect == "wd_from_lowp" and master else None
        xn, st = _rule(A, rule, g, x, st, h, defect, x_wd)
        return {"x": xn, "st": st}
    g = _grad(A, g_in, {**h, "delta": 0.0}, None)
    n = len(sizes)
    if rule == "lars":
        q = _ratio(A, rule, A.segsum(x * x, idx, n, sizes), A.segsum(g * g, idx, n, sizes), h)
        qe = A.lift(q_in) if q_in is not None else q
        xn, vel = _lars_apply(A, g, x, st[0], _expand(A, qe, idx), h)
        return {"x": xn, "st": [vel], "q": q}
    m, v = _lamb_moments(A, g, st[0], st[1], h)
    ms, vs = (A.lift(mv_in[0]), A.lift(mv_in[1])) if mv_in is not None else (A.stored(m, sd), A.stored(v, sd))
    u = _lamb_u(A, ms, vs, x, h)
    q = _ratio(A, rule, A.segsum(x * x, idx, n, sizes), A.segsum(u * u, idx, n, sizes), h)
    qe = A.lift(q_in) if q_in is not None else q
    return {"x": _lamb_apply(A, x, u, _expand(A, qe, idx), h), "st": [m, v], "q": q}


def _expand(A, q, idx):
    return V(q.val[idx], q.err[idx], q.u) if isinstance(q, V) else q[idx]


def emulate(case, combo, inp, defect=None):
    """The fp32 emulation (fp64 leaves: fp64) of one step with an optional planted defect: the same program
    in plain tensors of the compute type, outputs stored round-to-nearest. Returns an ``out`` dict."""
    pd, gd, sd, master = combo
    ct = ct_of(pd)
    sizes = [t.numel() for t in inp["p"]]
    c = dict(case)
    if defect == "eps_dropped":
        c["eps"] = 0.0
    elif defect == "stale_bt":  # beta^t of the previous step
        c["bt1"], c["bt2"] = c["bt1"] / c["b1"], c["bt2"] / c["b2"]
    elif defect == "lr_off":
        c["lr"] = c["lr"] * 1.001
    elif defect == "f32_beta2":
        c["b2"] = float(torch.tensor(c["b2"], dtype=F32))
    if defect == "fp64_in_fp32":
        ct = F32
    trunc = defect == "trunc_store"
    A = Plain(ct, trunc=trunc, unrounded=defect == "lamb_unrounded_u")
    if defect == "fp64_in_fp32":
        r = _step(A, {**c, "ts": None if c.get("ts") is None else c["ts"].to(F32)}, (F32, F32, F32, False), inp, defect)
    else:
        r = _step(A, c, combo, inp, defect)
    out = {"g": inp["g"], "q": None}
    out["st"] = [_split(store(s, sd, trunc), sizes) for s in r["st"]]
    if master:
        out["w"] = _split(r["x"].to(F32), sizes)
        if defect == "p_from_p_minus_dx":
            dx = _flat(inp["w"]) - r["x"]
            out["p"] = _split((_flat(inp["p"]).to(F32) - dx).to(pd), sizes)
        else:
            out["p"] = _split(store(r["x"].to(F32), pd, trunc), sizes)
    else:
        out["w"] = None
        out["p"] = _split(store(r["x"], pd, trunc), sizes)
    if "q" in r:
        out["q"] = r["q"].to(ct_of(pd))
    if defect == "last_untouched":  # the last element of the 4097-element leaf
        i = sizes.index(4097)
        for new, old in [(out["p"], inp["p"])] + [(a, b) for a, b in zip(out["st"], inp["st"])] + \
                ([(out["w"], inp["w"])] if master else []):
            new[i] = new[i].clone()
            new[i][-1] = old[i][-1]
    return out


def closed_form(case, combo, inp):
    """The float64 closed form of one step (the exact cases): flat ``x``, ``st``, per-leaf ``q``."""
    return _step(Plain(F64), case, combo, inp)


# ------------------------------------------------------------------------------------ the check

def _frac(got, val, bound):
    d = (got.to(F64) - val).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
    return d / bound


def check(case, combo, inp, out):
    """Hold one step's stored outputs ``out`` to the bounds derived from its stored inputs ``inp``.
    Returns ``(fracs, msgs, info)``: the worst observed error as a fraction of its bound per output, the
    violations, and ``info['undecided']`` (Lion's share)."""
    rule, (pd, gd, sd, master) = case["rule"], combo
    u = 2.0 ** -53 if pd == F64 else 2.0 ** -24
    sizes = [t.numel() for t in inp["p"]]
    fr, msgs, info = {}, [], {"undecided": 0.0}
    xd = F32 if master else pd
    got_x = _flat(out["w"] if master else out["p"])
    got_st = [_flat(s) for s in out["st"]]

    def hold(name, got, v, dtype, mask=None):
        bound = v.err + rt(dtype, v.val) + TINY
        if not bool(torch.isfinite(bound).all()):
            msgs.append(f"{name}: the bound is not finite on {int((~torch.isfinite(bound)).sum())} elements")
        f = _frac(got, v.val, bound)
        if mask is not None:
            f = f[~mask]
        worst = float(f.max()) if f.numel() else 0.0
        fr[name] = max(fr.get(name, 0.0), worst)
        if worst > 1:
            msgs.append(f"{name}: {int((f > 1).sum())} of {f.numel()} elements outside the bound, worst {worst:.3g}x")
        return f

    if rule in LAYERWISE:
        mv = (got_st[0], got_st[1]) if rule == "lamb" else None
        A = Tracked(u)
        r = _step(A, case, combo, inp, mv_in=mv)  # the ratio from the inputs (LAMB: and the stored moments)
        hold("ratio", out["q"], r["q"], ct_of(pd))
        r = _step(A, case, combo, inp, q_in=out["q"], mv_in=mv)
        for k, (g_, v_) in enumerate(zip(got_st, r["st"])):
            hold(f"state{k}", g_, v_, sd)
        hold("x", got_x, r["x"], xd)
    elif rule == "lion":
        runs = []
        for force in (1.0, -1.0, 0.0):
            A = Tracked(u, force)
            runs.append((_step(A, case, combo, inp), A.undecided))
        und = runs[0][1]
        info["undecided"] = float(und.double().mean()) if und.numel() else 0.0
        if info["undecided"] > UNDECIDED_CAP:
            msgs.append(f"lion: {info['undecided']:.2%} of the elements undecided, the cap is {UNDECIDED_CAP:.1%}")
        hold("state0", got_st[0], runs[0][0]["st"][0], sd)
        hold("x", got_x, runs[0][0]["x"], xd, mask=und)
        if bool(und.any()):
            fs = torch.stack([_frac(got_x, r["x"].val, r["x"].err + rt(xd, r["x"].val) + TINY)[und] for r, _ in runs])
            worst = float(fs.min(0).values.max())
            fr["x"] = max(fr["x"], worst)
            if worst > 1:
                msgs.append(f"x: an undecided element matches none of the three signs, worst {worst:.3g}x")
    else:
        r = _step(Tracked(u), case, combo, inp)
        for k, (g_, v_) in enumerate(zip(got_st, r["st"])):
            hold(f"state{k}", g_, v_, sd)
        hold("x", got_x, r["x"], xd)
    if master:
        want = _flat(out["w"]).to(pd)
        same = _flat(out["p"]).view(torch.int16) == want.view(torch.int16)
        fr["p==round(master)"] = 0.0 if bool(same.all()) else math.inf
        if not bool(same.all()):
            msgs.append(f"p: {int((~same).sum())} elements are not master.to({_N[pd]}) bit for bit")
    return fr, msgs, info


# ------------------------------------------------------------------------------------ input families

_BASE: dict = {}


def _u(gen, n, lo, hi):
    return lo + (hi - lo) * torch.rand(n, generator=gen, dtype=F64)


def leaf_scale(sizes):
    """Per-element gradient scale of its leaf: 2^((i mod 5) - 2)."""
    return torch.tensor([2.0 ** ((i % 5) - 2) for i in range(len(sizes))], dtype=F64)[_leaf_idx(sizes)]


def family_case(rule, family, combo, sizes):
    """(case, inp) of one family: the hyper-parameters and the CPU tensors in their device dtypes. The
    float64 draws depend on (rule, family) only; each combination rounds them to its own dtypes."""
    pd, gd, sd, master = combo
    ct = ct_of(pd)
    N = sum(sizes)
    case = {"rule": rule, "gs": 0.5, "dgs": None, "ts": None, "delta": 0.0, "dev": False, **HYPER[rule]}
    t = {"first_step": 1, "t1000": 1000}.get(family, 3)
    case["t"] = t
    if family == "tiny":
        case["eps"] = 2.0 ** -14 if gd == F16 else 1e-8
    key = (rule, family, tuple(sizes), case["eps"])
    if key not in _BASE:
        gen = E._gen("optim", rule, family)
        sc = leaf_scale(sizes)
        sign = lambda: 1.0 - 2.0 * (torch.rand(N, generator=gen) < 0.5).to(F64)
        if family == "tiny":
            eps = case["eps"]
            g = sign() * torch.exp(_u(gen, N, math.log(eps / 100), math.log(eps * 100)))
        else:
            g = _u(gen, N, -1, 1) * sc
        ge = g.abs() * case["gs"] if family == "tiny" else sc * case["gs"]
        x = torch.randn(N, generator=gen, dtype=F64)
        if family == "big_x":
            x = sign() * 2.0 ** 10 * _u(gen, N, 1, 2)
        st = []
        for k in SLOTS[rule]:
            if family == "first_step":
                fill = case["eps"] if rule in ("adagrad", "amsgrad") else 0.0
                st.append(torch.full((N,), fill, dtype=F64))
            elif k == "m":
                st.append(_u(gen, N, -1, 1) * ge * 0.5)
            elif k in "vV":
                st.append((_u(gen, N, 0.2, 1.0 if k == "v" else 1.4) * ge) ** 2)
            elif k == "u":
                st.append(_u(gen, N, 0.2, 1) * ge)
            elif k == "b":
                st.append(_u(gen, N, -1, 1) * ge * case["lr"] * 5)
            else:  # AdaDelta's running average of dx^2
                st.append(_u(gen, N, 0.2, 1) * (1e-4 if family != "tiny" else 1e-12))
        extra = _u(gen, len(sizes), 0.8, 1.25)
        _BASE[key] = (g, x, st, extra, sc)
    g, x, st, extra, sc = _BASE[key]
    if family == "clipped":
        case["gs"], case["dgs"] = 1.0 / 3.0, 0.7
        if rule not in LAYERWISE:
            lsc = torch.tensor([2.0 ** ((i % 5) - 2) for i in range(len(sizes))], dtype=F64)
            case["ts"] = (extra / lsc).to(ct)
            case["delta"] = 0.5 * (1.0 / 3.0) * 0.7
    case["bt1"], case["bt2"] = case["b1"] ** t, case["b2"] ** t
    inp = {"g": _split(g.to(gd), sizes), "st": [_split(s.to(sd), sizes) for s in st]}
    if master:
        inp["w"] = _split(x.to(F32), sizes)
        inp["p"] = [w.to(pd) for w in inp["w"]]
    else:
        inp["w"] = None
        inp["p"] = _split(x.to(pd), sizes)
    return case, inp


def next_step(case, out):
    """The second step: from what the first stored, the same gradients, ``beta^t`` advanced."""
    c = dict(case)
    c["t"] = case["t"] + 1
    c["bt1"], c["bt2"] = case["bt1"] * case["b1"], case["bt2"] * case["b2"]
    return c, {"p": out["p"], "g": out["g"], "st": out["st"], "w": out["w"]}


def clamp_share(case, inp, sizes):
    """Share of clamped elements per leaf scale class (i mod 5) of a ``clipped`` case."""
    h = resolve(case, F64)
    idx = _leaf_idx(sizes)
    g = _flat(inp["g"]).double() * h["gs"] * h["dgs"] * case["ts"].double()[idx]
    hit = g.abs() > h["delta"]
    cls = idx % 5
    return [float(hit[cls == k].double().mean()) for k in range(5)]


# ------------------------------------------------------------------------------------ exact cases

EXACT_SIZES = [1, 7, 8, 33, 4097, 24]
EXACT_LW_SIZES = [1, 4, 16, 64, 4096, 16384]
EXACT_KINDS = ("main", "zeros", "tie", "nonfinite")


def exact_case(rule, kind, combo):
    """(case, inp) of an exact case: dyadic scalars (lr = 2^-3, beta1 = rho = 0.5, beta2 = 0.75 — 0.25 for
    NAdam, whose root is of ``v * beta2``, 0.5 for AdaMax, whose ``beta2 * u`` must stay a power of two
    times ``|g|`` —, wd = 0.25, beta^t = 0, eps = 0 — 2^-10 for ``zeros`` —, grad_scale = 0.5), gradients
    k * 2^j with k in {1, 3} and parameters that are multiples of 1/4 below 2^5. ``v0 = g^2`` gives ``v = g^2`` and a root of
    ``|g|``; ``m0`` in {g, 3g} gives quotients of +-1 and +-2; AdaGrad's ``acc0 = 3 g^2`` and AMSGrad's
    ``vhat0`` in {g^2 / 4, 4 g^2}, AdaDelta's ``D0`` in {1/4, 1/16} are powers of four times ``g^2``.
    LARS / LAMB: every ``|x|`` of a leaf equal and leaves of 4^k elements, so the norms are exact
    (LAMB: ``sign x = sign g`` and ``|x| = 4 |m / g|``, so every ``|u|`` is equal too).
    ``tie`` (Lion): ``m0 = -g``, wd = 0. ``zeros``: g = 0 on zero states, |x| <= 4. ``nonfinite``: ``main``
    with one NaN and one +inf gradient, each in the middle of an aligned 8-vector of the 24-element leaf.
    Every intermediate is representable in fp32, so the fp32 result is the float64 one; a bf16 / fp16
    store is its one rounding."""
    pd, gd, sd, master = combo
    lw = rule in LAYERWISE
    sizes = EXACT_LW_SIZES if lw else EXACT_SIZES
    N = sum(sizes)
    idx = _leaf_idx(sizes)
    gen = E._gen("optim-exact", rule, "main" if kind == "nonfinite" else kind)
    b2 = {"nadam": 0.25, "adamax": 0.5, "lars": 0.25}.get(rule, 0.75)
    case = {"rule": rule, "lr": 0.125, "b1": 0.5, "b2": b2, "eps": 0.0, "wd": 0.25, "gs": 0.5, "dgs": None, "ts": None,
            "delta": 0.0, "dev": False, "bt1": 0.0, "bt2": 0.0, "t": 1}
    pick = lambda vals, n=N: torch.tensor(vals, dtype=F64)[torch.randint(len(vals), (n,), generator=gen)]
    mags = [0.5, 1.0, 2.0, 4.0, 1.5, 3.0, 6.0, 12.0]
    g_in = pick(mags) * pick([-1.0, 1.0])
    x = pick([0.25 * k for k in range(-16, 17)])
    if lw:
        per_leaf = pick([1.0, 2.0], len(sizes))[idx]  # |g| per leaf
        g_in = per_leaf * pick([-1.0, 1.0])
    g = g_in * 0.5
    mc = pick([1.0, 3.0])  # m0 = mc * g
    st = []
    if rule == "lars":
        x = 4 * g.abs() * pick([-1.0, 1.0])  # ||x|| = 4 ||g||: q = trust * 4 / (1 + wd * 4) = 1/2
        st = [pick([0.25 * k for k in range(-8, 9)])]
    elif rule == "lamb":
        c_leaf = pick([1.0, 3.0], len(sizes))[idx]
        mc = c_leaf                               # m = (mc + 1) / 2 * g: |m / g| = 1 or 2 over the whole leaf
        x = 4 * (mc + 1) / 2 * torch.sign(g)      # |u| = |m / g| + |x| / 4 = 2 |m / g|, q = ||x|| / ||u|| = 2
        st = [mc * g, g * g]
    for k in ("" if lw else SLOTS[rule]):
        if k == "m":
            st.append(mc * g)
        elif k == "v":
            st.append(3 * g * g if rule == "adagrad" else g * g)
        elif k == "V":
            st.append(g * g * pick([0.25, 4.0]))
        elif k == "u":
            st.append(g.abs() * pick([1.0, 4.0]))
        elif k == "b":
            st.append(pick([0.25 * k for k in range(-8, 9)]))
        else:
            st.append(pick([0.25, 0.0625]))
    if rule == "adabelief":  # m0 in {3g, -g}: d = -+g, s = 0.75 g^2 + 0.25 g^2
        st[0] = pick([3.0, -1.0]) * g
    if kind == "tie":
        st[0] = -g
        case["wd"] = 0.0
    if kind == "zeros":
        case["eps"] = 2.0 ** -10
        g_in = torch.zeros(N, dtype=F64)
        st = [torch.zeros(N, dtype=F64) for _ in st]
        x = pick([0.25 * k for k in range(-16, 17)])
    if kind == "nonfinite":
        at = sum(sizes[:sizes.index(24)])
        g_in = g_in.clone()
        g_in[at + 3], g_in[at + 12] = math.nan, math.inf
    inp = {"g": _split(g_in.to(gd), sizes), "st": [_split(s.to(sd), sizes) for s in st]}
    for a, b in zip([g_in, x, *st], [_flat(inp["g"]), x.to(pd), *[_flat(s) for s in inp["st"]]]):
        ok = (a == b.to(F64)) | torch.isnan(a)
        assert bool(ok.all()), f"{rule}/{kind}: an exact input is not representable in its dtype"
    inp["w"] = _split(x.to(F32), sizes) if master else None
    inp["p"] = _split(x.to(pd), sizes)
    return case, inp


def check_exact(case, combo, inp, out):
    """``out`` against the float64 closed form, bit for bit (NaN == NaN; a stored low-precision value is
    the rounding of the closed form). Returns the list of violations."""
    pd, gd, sd, master = combo
    r = closed_form(case, combo, inp)
    msgs = []

    def same(name, got, want, dtype):
        got, want = got.to(F64), want.to(dtype).to(F64)
        ok = (got == want) | (torch.isnan(got) & torch.isnan(want))
        if not bool(ok.all()):
            i = int((~ok).nonzero()[0])
            msgs.append(f"{name}: {int((~ok).sum())} of {ok.numel()} differ, first at {i}: got {got[i].item()!r} "
                        f"want {want[i].item()!r}")

    for k, s in enumerate(r["st"]):
        same(f"state{k}", _flat(out["st"][k]), s, sd)
    if master:
        same("master", _flat(out["w"]), r["x"], F32)
        same("p", _flat(out["p"]), _flat(out["w"]), pd)
    else:
        same("x", _flat(out["p"]), r["x"], pd)
    if "q" in r:
        same("ratio", out["q"], r["q"], ct_of(pd))
    return msgs


# ------------------------------------------------------------------------------------ calling the project

def call(case, p, g, st, w, ratios=None, workspace=None):
    """One step of the project's optimiser entry on the tensors given (CUDA: the kernels; CPU: the
    ``*_reference_`` paths), the scalar tensors made on the tensors' device."""
    from fluxmpi_amd.ops import optim
    rule, dev = case["rule"], p[0].device
    ct = ct_of(p[0].dtype)
    kw = dict(weight_decay=case["wd"], grad_scale=case["gs"], masters=w)
    if case.get("dgs") is not None:
        kw["dev_gscale"] = torch.tensor([case["dgs"]], dtype=F32, device=dev)
    if rule not in LAYERWISE:
        if case.get("ts") is not None:
            kw["tscale"] = case["ts"].to(device=dev, dtype=ct)
        kw["clip_delta"] = case.get("delta", 0.0)
    block = None
    if case.get("dev"):
        block = torch.tensor([case["lr"], case["bt1"], case["bt2"]] if rule in READS_BT else [case["lr"]],
                             dtype=F32, device=dev)
    if rule in ("adam", "adamw"):
        optim.adam_(p, g, st[0], st[1], lr=case["lr"], beta1=case["b1"], beta2=case["b2"], eps=case["eps"],
                    bc1=1.0 - case["bt1"], bc2=1.0 - case["bt2"], dev_hyper=block, **kw)
    elif rule in SGD:
        optim.sgd_(p, g, st[0] if st else None, lr=case["lr"], momentum=case["b1"] if rule != "descent" else 0.0,
                   nesterov=rule == "nesterov", dev_lr=block, **kw)
    elif rule == "lars":
        optim.lars_(p, g, st[0], lr=case["lr"], momentum=case["b1"], trust=case["b2"], eps=case["eps"], dev_hyper=block,
                    ratios=ratios, workspace=workspace, **kw)
    elif rule == "lamb":
        optim.lamb_(p, g, st[0], st[1], lr=case["lr"], beta1=case["b1"], beta2=case["b2"], eps=case["eps"],
                    bt1=case["bt1"], bt2=case["bt2"], dev_hyper=block, ratios=ratios, workspace=workspace, **kw)
    else:
        optim.rule_(rule, p, g, st, lr=case["lr"], beta1=case["b1"], beta2=case["b2"], eps=case["eps"],
                    bt1=case["bt1"], bt2=case["bt2"], dev_hyper=block, **kw)


def run_cpu(case, combo, inp):
    """The project's CPU path on clones of ``inp``: the emulation the GPU tests are kept honest by."""
    p = [t.clone() for t in inp["p"]]
    st = [[t.clone() for t in s] for s in inp["st"]]
    w = [t.clone() for t in inp["w"]] if inp["w"] is not None else None
    q = torch.ones(len(p), dtype=ct_of(combo[0])) if case["rule"] in LAYERWISE else None
    call(case, p, inp["g"], st, w, ratios=q)
    return {"p": p, "g": inp["g"], "st": st, "w": w, "q": q}


# planted defect -> (rule, combination, family or exact kind) in which it must be caught
DEFECTS = {
    "eps_dropped": ("rmsprop", COMBOS[0], "tiny"),
    "eps_in_sqrt": ("adam", COMBOS[0], "tiny"),
    "stale_bt": ("adam", COMBOS[0], "first_step"),
    "lr_off": ("rmsprop", COMBOS[0], "uniform"),
    "wd_from_lowp": ("adamw", COMBOS[4], "big_x"),
    "wd_times_lr": ("rmsprop", COMBOS[0], "big_x"),
    "wd_on_dx": ("momentum", COMBOS[0], "big_x"),
    "scale_after_clamp": ("adam", COMBOS[0], "clipped"),
    "trunc_store": ("amsgrad", COMBOS[2], "uniform"),
    "p_from_p_minus_dx": ("adam", COMBOS[4], "uniform"),
    "nesterov_sign": ("nesterov", COMBOS[0], "uniform"),
    "delta_post_decay": ("adadelta", COMBOS[0], "big_x"),
    "vhat_old_v": ("amsgrad", COMBOS[0], "first_step"),
    "lion_m_first": ("lion", COMBOS[0], "uniform"),
    "lamb_unrounded_u": ("lamb", COMBOS[2], "uniform"),
    "fp64_in_fp32": ("nadam", COMBOS[10], "uniform"),
    "f32_beta2": ("adam", COMBOS[10], "uniform"),
    "last_untouched": ("adabelief", COMBOS[0], "uniform"),
}
