"""Inputs, float64 references, derived bounds, a float32 emulation and planted defects for the fused
softmax cross-entropy (``csrc/kernels/xent.hip``), shared by ``test_xent.py`` and ``test_xent_gpu.py``
(plain helper module: no fixtures, no tests). The checker, the guard bands and the constants are those
of ``mfma_edges``; the stored-value rounding ``rt`` is ``norm_edges``'.

Conventions. u = 2^-24 is fp32's unit roundoff, u_T the stored dtype's. Each fp32 addition of a
reduction is charged E = 2^-23, each multiplication and each stored value one unit roundoff, an fma one
multiplication and one addition (so the bounds do not depend on contraction). ``v_exp_f32`` and
``v_log_f32``, and nothing else, are charged 1 ulp = 2u on the device. 1e-30 is added to each bound.
Everything is first order in u. Nothing is fitted to kernel output. The smoothing eps and lam are
passed as fp32 values (``EPS``), so they carry no error of their own; 1 - eps is rounded once.
log2(e) and ln(2) are used as head + tail pairs, so the constants carry no error either.

Reduction lengths (closed forms that may over-count): a lane adds n = 8 VPL terms on the register path
(C % 8 == 0, C <= 8192, aligned; VPL the smallest of {1, 2, 3, 4, 6, 8, 12, 16} >= ceil(C / 512)) or
n = ceil(C / 64) on the general path, then 6 wave levels: L = n + 6. The finish adds L_f =
ceil(B / 256) + 8.

Per row, with m = max x (exact: a maximum of stored values), D_j = |x_j - m|:

    de_j  = e_j (2u (1 + D_j log2e ln2) + 2u + R)
            (x_j - m rounds once, its product with log2(e) once: 2u D_j log2e in the exponent, times
            ln2 in e; v_exp_f32 2u. R = 0 on the register path. On the general path the online sum
            multiplies a lane's partial by exp(m_old - m_new) each time its running maximum rises, at
            most n times, and once more at the wave merge: the arguments telescope to x_j - m (already
            counted), every factor costs 2u (exp) + u (product): R = 3u (n + 1).)
    ds    = L E s + sum_j de_j
    dlse  = ds / s + 2u |ln s| + 2u |lse|       (v_log_f32; the two fma roundings of m + ln2 log2 s)
    dmean = L E mean|x| + 2u |mean|             (mean = sum x * fl(1 / C))
    hard    d = (1 - eps) x_y + eps mean:
            dd = 2u |(1 - eps) x_y| + eps dmean + u |eps mean| + u |d|;  W = 1, dW = 0
    mixed   d = (1 - eps)(lam x_y + rest x_yp) + W eps mean, W = fl(lam + rest), dW = u |W|:
            dd = 4u (1 - eps)(|lam x_y| + |rest x_yp|) + |W| eps dmean + 3u |W eps mean| + u |d|
    dense   t'_j = t_j (1 - eps) + eps / C, T_j = |t_j| (1 - eps) + eps / C, dt'_j = 3u T_j:
            dd = (L E + 4u) sum_j T_j |x_j|,  dW = (L E + 3u) sum_j T_j
    row loss l = W lse - d:
            dl = |W| dlse + |lse| dW + dd + u |W lse| + u |l|
    reduced loss: sum: dsum = sum_b dl_b + L_f E sum_b |l_b|;  mean: dsum / B + 2u |loss|
            (fl(1 / B) and the product)

Backward, with r = fl(1 / s) a true division:

    dp_j  = p_j (de_j / e_j [R = 0: no online chain here] + ds / s + 2u)
    dt_j  = 5u T_j    (label forms: T_j = |(1 - eps) lam| [j = y] + |(1 - eps) rest| [j = y_p] + |W| eps / C;
                       1 - eps, its product with lam, W eps / C and the two additions)
    q_j   = p_j W - t_j:  dq_j = |W| dp_j + p_j dW + dt_j + u p_j |W| + u |q_j|
    dx_j  = T(q_j gs), gs = g fl(1 / B) ("mean": 2u) or g:
            ddx_j = |gs| dq_j + 3u |dx_j| + u_T |dx_j|   (+ 2^-25 for fp16, below its normal range)

The float32 emulation (``emulate``) evaluates the kernel's arithmetic in torch with no fma (exp2, log2
and the division correctly rounded) and must fit the same bounds. Planted defects (``DEFECTS``), each
rejected by at least one case: a dropped max subtraction, 1 / C in place of 1 / B, the partner taken as
b + 1, the weight W dropped on a dense row that does not sum to 1, a tie counted the wrong way.
"""
import numpy as np
import torch

from fluxmpi_amd.ops import xent as X

from . import mfma_edges as E
from .mfma_edges import E23, TINY
from .norm_edges import U32, rt

EPS = float(np.float32(0.1))  # the smoothing of the tests, an fp32 value
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
DEFECTS = ("no_max", "inv_c", "partner_next", "drop_w", "tie_wrong")
_LADDER = (1, 2, 3, 4, 6, 8, 12, 16)


def ceil_div(a, b):
    return -(-a // b)


def lane_terms(C, general=False):
    """``(n, general)``: the terms a lane adds, and whether the row takes the general path."""
    if general or C % 8 != 0 or C > 8192:
        return ceil_div(C, 64), True
    return 8 * next(v for v in _LADDER if v >= ceil_div(C, 512)), False


# ------------------------------------------------------------------------------------------ inputs

def logits(B, C, dtype, seed=0, scale=3.0, shift=0.0):
    g = E._gen("xent", B, C, seed)
    return (torch.randn(B, C, generator=g) * scale + shift).to(dtype)


def labels(B, C, seed=0, dtype=torch.int64, coincide=True):
    """Seeded labels; with ``coincide`` (and B >= 2) rows 0 and B - 1 share one label, so a mixed row's
    two weights fall on one class (the middle row of an odd B is its own partner anyway)."""
    y = torch.randint(0, C, (B,), generator=E._gen("xent-y", B, C, seed))
    if coincide and B >= 2:
        y[B - 1] = y[0]
    return y.to(dtype)


def dense_target(B, C, dtype=torch.float32, seed=0):
    """Non-negative rows that do NOT sum to 1 (row b sums to about 0.5 + b / B)."""
    t = torch.rand(B, C, generator=E._gen("xent-t", B, C, seed))
    t = t / t.sum(1, keepdim=True) * (0.5 + torch.arange(B).view(B, 1) / B)
    return t.to(dtype)


def plant_ties(x, y):
    """Copies of the label's logit planted at one lower and two higher indices (where there is room), and
    one strictly larger value: rank = 1 + #(ties below)."""
    x = x.clone()
    B, C = x.shape
    for b in range(B):
        yb = int(y[b])
        v = x[b, yb].clone()
        x[b] = torch.where(x[b] >= v, v - 1, x[b])  # nothing at or above the label's value ...
        x[b, yb] = v
        if yb > 0:
            x[b, 0] = v  # a tie below: counts
        if yb + 2 < C:
            x[b, C - 2:] = v  # two ties above: they do not (and a rule that counts them instead gives another number)
        if 0 < yb - 1:
            x[b, yb - 1] = v + 1  # ... but this one
    return x


# ---------------------------------------------------------------------------------- reference, bounds

def refs(x, kw, reduction="mean", g=1.0, general=False):
    """The float64 reference of ``softmax_cross_entropy(x, **kw)`` with incoming gradient ``g`` (a number,
    or a ``[B]`` tensor for ``"none"``) and the derived bounds: a dict with ``loss_row, loss, dx, rank`` and
    ``b_loss_row, b_loss, b_dx``. Computed once per case on the CPU."""
    x = x.detach().cpu()
    kw = {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    if isinstance(kw.get("target"), X.MixedLabels):
        ml = kw["target"]
        kw = dict(kw, target=X.MixedLabels(ml.labels.cpu(), ml.lam.cpu() if isinstance(ml.lam, torch.Tensor) else ml.lam,
                                           ml.label_smoothing))
    B, C = x.shape
    dt = x.dtype
    spec = X._parse("xent_edges", x, kw["target"], kw.get("label_smoothing", 0.0), kw.get("lam"), kw.get("labels"))
    eps = spec.eps
    loss, loss_row, dx1, rank = X.xent_reference(x, reduction=reduction, **kw)
    n, gen = lane_terms(C, general)
    L = n + 6
    u = U32
    xs = x.double()
    m = xs.max(1, keepdim=True).values
    D = (xs - m).abs()
    e = torch.exp(xs - m)
    s = e.sum(1, keepdim=True)
    lse = m + torch.log(s)
    R = 3 * u * (n + 1) if gen else 0.0
    rel_e = 2 * u * (1 + D * LOG2E * LN2) + 2 * u
    ds = L * E23 * s + (e * (rel_e + R)).sum(1, keepdim=True)
    dlse = (ds / s + 2 * u * torch.log(s).abs() + 2 * u * lse.abs()).squeeze(1)
    mean = xs.sum(1) / C
    dmean = L * E23 * xs.abs().sum(1) / C + 2 * u * mean.abs()
    _, t, W, p = X._formulas(x, spec, torch.float64)
    W = W.squeeze(1)
    lse1 = lse.squeeze(1)
    d = W * lse1 - loss_row
    if spec.mode == X.MODE_DENSE:
        T = spec.dense.double().abs() * (1 - eps) + eps / C
        dd = (L * E23 + 4 * u) * (T * xs.abs()).sum(1)
        dW = (L * E23 + 3 * u) * T.sum(1)
    else:
        y = spec.labels.long()
        xy = xs.gather(1, y.unsqueeze(1)).squeeze(1)
        oh = torch.zeros(B, C, dtype=torch.float64).scatter_(1, y.unsqueeze(1), 1.0)
        if spec.mode == X.MODE_MIXED:
            lam, rest = (float(v) for v in X._lam_pair(spec.lam, x.device, torch.float64))
            xp = xs.gather(1, y.flip(0).unsqueeze(1)).squeeze(1)
            dW = u * W.abs()
            dd = (4 * u * (1 - eps) * ((lam * xy).abs() + (rest * xp).abs()) + W.abs() * eps * dmean
                  + 3 * u * (W * eps * mean).abs() + u * d.abs())
            T = (1 - eps) * (abs(lam) * oh + abs(rest) * oh.flip(0)) + W.abs().unsqueeze(1) * eps / C
        else:
            dW = torch.zeros(B, dtype=torch.float64)
            dd = 2 * u * ((1 - eps) * xy).abs() + eps * dmean + u * (eps * mean).abs() + u * d.abs()
            T = (1 - eps) * oh + eps / C
    dl = W.abs() * dlse + lse1.abs() * dW + dd + u * (W * lse1).abs() + u * loss_row.abs()
    Lf = ceil_div(B, 256) + 8
    dsum = dl.sum() + Lf * E23 * loss_row.abs().sum()
    if reduction == "mean":
        b_loss = dsum / B + 2 * u * loss.abs() + TINY
    elif reduction == "sum":
        b_loss = dsum + TINY
    else:
        b_loss = dl + TINY
    # backward
    gt = g.detach().cpu().double().view(B, 1) if isinstance(g, torch.Tensor) else torch.full((B, 1), float(g),
                                                                                            dtype=torch.float64)
    gs = gt / B if reduction == "mean" else gt
    dp = p * (rel_e + ds / s + 2 * u)
    Wc = W.unsqueeze(1)
    q = p * Wc - t
    dq = Wc.abs() * dp + p * dW.unsqueeze(1) + 5 * u * T + u * p * Wc.abs() + u * q.abs()
    dx = q * gs
    b_dx = gs.abs() * dq + 3 * u * dx.abs() + rt(dt, dx) + TINY
    return {"loss_row": loss_row, "loss": loss, "dx": dx, "rank": rank, "b_loss_row": dl + TINY, "b_loss": b_loss,
            "b_dx": b_dx, "dtype": dt}


def check_all(name, got, R, errs):
    """Every element of ``got`` (``loss_row``, ``loss``, ``dx``, and ``rank`` when both sides have one)
    against the reference ``R = refs(...)``: within the bounds, the rank equal. Keys missing in ``got``
    are not checked."""
    if got.get("loss_row") is not None:
        E.check(f"{name} loss_row", got["loss_row"].detach().cpu(), R["loss_row"], R["b_loss_row"], errs)
    if got.get("loss") is not None:
        E.check(f"{name} loss", got["loss"].detach().cpu(), R["loss"], R["b_loss"], errs)
    if got.get("dx") is not None:
        E.check(f"{name} dx", got["dx"].detach().cpu(), R["dx"], R["b_dx"], errs)
    if got.get("rank") is not None and R["rank"] is not None:
        E.check(f"{name} rank", got["rank"].detach().cpu(), R["rank"].double(), None, errs)


# ---------------------------------------------------------------------------------------- emulation

_F = torch.float32
_L2E_HI, _L2E_LO = 1.4426950216293335, 1.925963033500309e-8
_LN2_HI, _LN2_LO = 0.6931471824645996, -1.904654299957767e-9


def _c(v):
    return torch.tensor(v, dtype=_F)


def _exp_of(d):
    return torch.exp2(d * _c(_L2E_HI) + d * _c(_L2E_LO))


def emulate(x, kw, reduction="mean", g=1.0, defect=None):
    """``{loss_row, loss, dx, rank}`` of the kernels' arithmetic in float32 torch on the CPU, every
    operation rounded on its own (no fma), optionally with one planted defect of ``DEFECTS``."""
    assert defect is None or defect in DEFECTS, defect
    x = x.detach().cpu()
    B, C = x.shape
    spec = X._parse("xent_edges", x, kw["target"], kw.get("label_smoothing", 0.0), kw.get("lam"), kw.get("labels"))
    xs = x.to(_F)
    eps = _c(spec.eps)
    ome = _c(1.0) - eps
    inv_c = _c(1.0) / _c(float(C))
    eps_c = eps / _c(float(C))
    m = xs.max(1, keepdim=True).values
    if defect == "no_max":
        m = torch.zeros_like(m)
    e = _exp_of(xs - m)
    s = e.sum(1, keepdim=True)
    l2 = torch.log2(s)
    lse = ((_c(_LN2_HI) * l2 + m) + _c(_LN2_LO) * l2).squeeze(1)
    idx = torch.arange(C).unsqueeze(0)
    rank = None
    if spec.labels is not None:
        y = spec.labels.long().unsqueeze(1)
        xy = xs.gather(1, y)
        tie = (idx > y) if defect == "tie_wrong" else (idx < y)
        rank = ((xs > xy) | ((xs == xy) & tie)).sum(1).to(torch.int32)
    if spec.mode == X.MODE_DENSE:
        t = spec.dense.to(_F) * ome + eps_c
        d = (t * xs).sum(1)
        W = t.sum(1)
        if defect == "drop_w":
            W = torch.ones_like(W)
    else:
        mean = xs.sum(1) * inv_c
        xy = xy.squeeze(1)
        oh = torch.zeros(B, C, dtype=_F).scatter_(1, y, 1.0)
        if spec.mode == X.MODE_MIXED:
            lam, rest = X._lam_pair(spec.lam, x.device, _F)
            part = (torch.arange(B) + 1) % B if defect == "partner_next" else torch.arange(B).flip(0)
            yp = spec.labels.long()[part].unsqueeze(1)
            xp = xs.gather(1, yp).squeeze(1)
            W = (lam + rest).expand(B)
            d = ome * (lam * xy + rest * xp) + W * (eps * mean)
            ohp = torch.zeros(B, C, dtype=_F).scatter_(1, yp, 1.0)
            t = (oh * (ome * lam) + ohp * (ome * rest)) + (W * eps_c).unsqueeze(1)
        else:
            W = torch.ones(B, dtype=_F)
            d = ome * xy + eps * mean
            t = oh * ome + eps_c
    loss_row = W * lse - d
    inv_n = _c(float(np.float32(1.0 / (C if defect == "inv_c" else B))))
    total = loss_row.sum()
    loss = total * inv_n if reduction == "mean" else (total if reduction == "sum" else loss_row)
    gt = g.detach().cpu().to(_F).view(B, 1) if isinstance(g, torch.Tensor) else torch.full((B, 1), float(g), dtype=_F)
    gs = gt * inv_n if reduction == "mean" else gt
    r = _c(1.0) / s
    p = _exp_of(xs - m) * r
    dx = ((p * W.unsqueeze(1) - t) * gs).to(x.dtype)
    return {"loss_row": loss_row, "loss": loss, "dx": dx, "rank": rank}


__all__ = ["EPS", "DEFECTS", "logits", "labels", "dense_target", "plant_ties", "refs", "check_all", "emulate",
           "lane_terms", "ceil_div"]
