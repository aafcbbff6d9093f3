"""Inputs, float64 references, derived bounds, float32 emulations and planted defects for the
normalisation and pooling kernels (batchnorm.hip, layernorm.hip, groupnorm.hip, pool.hip), shared by
``test_norm_edges_gpu.py`` (plain helper module: no fixtures, no tests). The checker, the guard bands
and the addition constant are those of ``mfma_edges``.

Unit roundoffs (round to nearest, half a unit in the last of p significand bits, implicit bit included):
fp32 (p = 24) u = 2^-24, fp16 (p = 11) 2^-11, bf16 (p = 8) 2^-8 (``UT[dtype]``, written u_T for the dtype of a
stored activation). bf16 is NOT 2^-9: the correctly rounded bf16 of 1.0117 is 1.015625, 0.96 * 2^-8 away
relatively, so no kernel could meet 2^-9 (``test_unit_roundoffs_cpu`` pins all three; ``mfma_edges.U8``
is the same 2^-8). Every addition of a reduction errs by at most E = 2^-23 relatively
(as ``mfma_edges.bound``), so a sum of terms t_i along any tree whose longest chain has L additions errs
by at most L E sum|t_i|. An fma is charged like a multiplication followed by an addition (two roundings),
so the bounds do not depend on whether the compiler contracts, and the float32 emulations below, which
have no fma, must fit too. All bounds are first order in u except where a second-order term is written
out; 1e-30 is added to each. Nothing is fitted to kernel output.

Reduction lengths L (closed forms that may over-count, never read from the extension):

    BatchNorm (rows R, channels C)   cv = C / 8, rpi = max(1, 256 // cv) rows in flight per workgroup,
        min_rows = ceil(32768 / C), blocks B <= B0 = ceil(R / min_rows) and, the grid being one round of
        resident workgroups of a 256-CU device, B >= min(B0, 256): a lane adds at most
        ceil(ceil(R / min(B0, 256)) / rpi) + 1 rows, the workgroup adds rpi lane partials, a shard takes
        ceil(B0 / 16) atomics, the finalize adds 16 shards and 4 groups:
        L_bn = ceil(ceil(R / min(B0, 256)) / rpi) + 1 + rpi + ceil(B0 / 16) + 20
    LayerNorm (row length D)         VPL = the smallest of {1, 2, 3, 4, 6, 8, 12, 16} >= ceil(D / 512):
        a lane adds 8 VPL values, the wave sum has 6 levels: L_ln = 8 VPL + 6; dw / db / column sums over
        the rows: a wave adds at most R rows, the workgroup 4 waves: L_rows = R + 4 (the [blocks] partials
        are summed in float64 by the test)
    GroupNorm (HW pixels, C, G)      cv = C / 8, PL = max(1, min(256 // cv, (16384 - 2C - 2G) // (2C)))
        pixel lanes, cpg = C / G: L_px = ceil(HW / PL) + PL per channel, L_gn = L_px + cpg per group
        (``gn_refs`` / ``gn_check_fwd`` take another kernel's L_gn as ``L``, ``gn_bwd_refs`` / ``gn_check_bwd`` its
        L_px as ``Lpx``: the fused DEQ cell's are 19 + cpg and 19, ``deq_cell_edges``)

Statistics of the single-pass form (BatchNorm per channel, GroupNorm per group; n values, A1 = mean|x|,
A2 = mean x^2, kappa = (mean^2 + var) / var = A2 / var):

    dmean = L E A1 + 2u |mean|                                    (s * fl(1 / n): two roundings)
    dvar  = var kappa ((L + 3) E + 4u) + 2 |mean| dmean + dmean^2 (= A2 (...): the sum of squares, its
            product with 1 / n, mean * mean and the subtraction all err relative to A2 = var kappa)
    invstd lies in [rsqrt(var + dvar + eps), rsqrt(max(var - dvar, 0) + eps)] (the kernels clamp a
    negative variance to 0), widened by 4u relatively for the device's rsqrt (2 ulp):
    dinv = the larger distance of that interval's ends from the float64 invstd. First order this is
    invstd dvar / (2 (var + eps)), i.e. relative kappa (L + 3) E / 2 when eps << var: the kappa term.
    LayerNorm's two-pass variance has no kappa: dvar = var ((L + 3) E + 4u) + dmean^2 (sum (x - mean) = 0
    cancels the first order in dmean).

Forward output y = T(act(x scale + shift [+ r])), scale = w invstd, shift = b - mean scale:

    dscale = |w| dinv + u |scale|
    dz = |x - mean| dscale + |scale| dmean + dscale dmean
         + 2u (|x scale| + |mean scale| + |b| + |z0|) [+ 2u |z| with a residual]       (pre-activation)
    dy = dz + u_T |y|        (ReLU is 1-Lipschitz; rounding to T is monotone, so it passes through)
    (every "u_T |v|" of a stored fp16 value also carries 2^-25, half the smallest fp16 subnormal: below
    2^-14 the spacing is 2^-24 whatever |v|. The float32 emulation found this at |dx| = 1.4e-5.)
    A ReLU decision is "undecided" where |z| <= dz: either mask bit and either gradient is accepted,
    and at most 0.1 % of a case's elements may be undecided (asserted).

BatchNorm backward (mean, invstd, w, b, the mask / y are stored inputs; g = dy or dy * mask):

    db = sum g:        L E sum|g|  (+ sum over undecided |dy|)
    dw = sum g xhat:   (L + 3) E sum|g xhat|  (+ sum over undecided |dy xhat|); xhat = (x - mean) invstd
    dx = A g + (B x + D), A = w invstd, k2 = db / n, k3 = dw / n, B = -A invstd k3,
         D = A (mean invstd k3 - k2); dk2 = ddb / n + 2u |k2|, dk3 = ddw / n + 2u |k3|
    ddx = |A invstd (x - mean)| dk3 + |A| dk2
          + 4u (|B x| + |A mean invstd k3| + |A k2| + |A g|) + 2u |dx| + u_T |dx|
          (the u (|B x| + |D|) term: B x + D cancels when |mean| >> std)
    dres = g exactly (g is a value of T).

LayerNorm forward (h = T(fl32(x + r)) is reproduced exactly and is the input of the reference):
    dy = |w| (|h - mean| drstd + rstd dmean + drstd dmean) + 3u |(h - mean) rstd w| + 2u (|y| + |b|) + u_T |y|
LayerNorm backward (g = dy w, m1 = mean g, m2 = mean g xhat):
    dm1 = (L + 2) E mean|g| + 2u |m1|, dm2 = (L + 4) E mean|g xhat| + 2u |m2|
    ddx = rstd (dm1 + |xhat| dm2) + 4u rstd (|g| + |m1| + |xhat m2|) [+ 2u |dx|] + u_T |dx|
    dw: (L_rows + 3) E sum|dy xhat|, db: L_rows E sum|dy|, column sums: L_rows E sum|dx stored|

GroupNorm forward: as BatchNorm's with the group statistics on h = T(act(x + a)) (reproduced exactly).
GroupNorm backward (per sample; S_c = sum_p dy, Q_c = sum_p dy h):
    dS = L_px E sum|dy|, dQ = (L_px + 1) E sum|dy h|
    db = S exactly bounded by dS; dw = rstd (Q - mean S):
         ddw = rstd (dQ + |mean| dS + 2u (|Q| + 2 |mean S|)) + 2u |dw|   (this form cancels like the
         variance: its kappa is (sum|dy h| + |mean| sum|dy|) / sum|dy (h - mean)|, about sqrt(kappa))
    m1 = sum_c w S / M, m2 = sum_c w dw / M (M = HW cpg):
         dm1 = (sum|w| dS + (cpg + 2) E sum|w S|) / M, dm2 = (sum|w| ddw + (cpg + 3) E sum|w dw|) / M
    ddh = rstd (dm1 + |xhat| dm2) + 4u rstd (|dy w| + |m1| + |xhat m2|) + u_T |dh|; h > 0 is exact.

Pool: scale and shift are signed powers of two and x lies on a small grid, so fma(x, scale, shift) is
exact: y, idx and the backward's dz must EQUAL the reference (first maximum in scan order; 0xFF where
the maximum is <= 0).
"""
import math

import torch

from . import mfma_edges as E
from .mfma_edges import E23, TINY

U32 = 2.0 ** -24
UT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUB = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}  # half the smallest subnormal
UNDECIDED_CAP = 1e-3
X_STD = 4 / math.sqrt(12)  # of U[-2, 2)


def rt(dtype, v):
    """The rounding of v to a stored activation of ``dtype``: u_T |v|, plus half the smallest subnormal for
    fp16 (below 2^-14 its spacing is 2^-24 whatever |v|; bf16 and fp32 share fp32's exponent range)."""
    return UT[dtype] * v.abs() + SUB[dtype]


def ceil_div(a, b):
    return -(-a // b)


def guarded_bytes(n, device):
    """``n`` bytes (0xA5) between two 64-byte bands of 0x5A: a ReLU mask or a pool index array, which
    ``mfma_edges.guarded`` (16- and 32-bit elements) does not cover."""
    buf = torch.full((n + 128,), 0x5A, dtype=torch.uint8, device=device)
    view = buf[64:64 + n]
    view.fill_(0xA5)
    return buf, view


def take_bytes(name, buf, view, errs):
    out = view.clone()
    view.fill_(0x5A)
    broken = int((buf != 0x5A).sum())
    if broken:
        errs.append(f"{name}: {broken} guard bytes overwritten")
    return out


# ------------------------------------------------------------------------------- geometry (documented formulas)

def bn_geometry(rows, C, cap=256):
    """(cv, rpi, rows_per_block, blocks) of batchnorm.hip's row reductions at a grid cap of ``cap``."""
    cv = C // 8
    rpi = max(1, 256 // cv)
    min_rows = ceil_div(32768, C)
    blocks = max(1, min(ceil_div(rows, min_rows), cap))
    rpb = ceil_div(ceil_div(rows, blocks), rpi) * rpi
    return cv, rpi, rpb, ceil_div(rows, rpb)


def bn_fixed(C):
    return 256 % (C // 8) == 0


def bn_L(rows, C):
    rpi = max(1, 256 // (C // 8))
    b0 = ceil_div(rows, ceil_div(32768, C))
    return ceil_div(ceil_div(rows, min(b0, 256)), rpi) + 1 + rpi + ceil_div(b0, 16) + 20


def ln_vpl(D):
    need = ceil_div(D // 8, 64)
    return next(c for c in (1, 2, 3, 4, 6, 8, 12, 16) if c >= need)


def ln_L(D):
    return 8 * ln_vpl(D) + 6


def gn_pl(C, G):
    return max(1, min(256 // (C // 8), (16384 - 2 * C - 2 * G) // (2 * C)))


def gn_Lpx(HW, C, G):
    pl = gn_pl(C, G)
    return ceil_div(HW, pl) + pl


# ------------------------------------------------------------------------------- inputs

def _g(*key):
    return E._gen("norm", *key)


def _uni(g, shape, lo, hi):
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _sign(g, shape):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def affine(g, C):
    """w in +-[0.5, 1.5), |b| in [2^-4, 1)."""
    return _uni(g, (C,), 0.5, 1.5) * _sign(g, (C,)), _uni(g, (C,), 2.0 ** -4, 1.0) * _sign(g, (C,))


def balanced(g, n, C):
    """[n, C] with every column a seeded permutation of n/4 each of 1, -1, 2, -2 (sum 0, sum of squares 2.5 n)."""
    base = torch.tensor([1.0, -1.0, 2.0, -2.0]).repeat(n // 4)
    order = torch.rand(n, C, generator=g).argsort(0)
    return base[order]


def rows_inputs(family, rows, C, dtype, ratio=0, seed=0):
    """x, res, dy [rows, C] of ``dtype`` and fp32 w, b [C]. The statistics run over dim 0 (BatchNorm: per
    channel); LayerNorm and GroupNorm transpose / reshape this. families: uniform, offset (mean / std =
    ``ratio`` per channel, alternating sign), constant (channel 0 constant 0.5; constant1000: also channel 1 at 1000),
    integer (x balanced in {+-1, +-2}, res in {-2, 0, 2}, dy in {-2 .. 2}, w = +-1, b = 0.25)."""
    g = _g(family, rows, C, str(dtype), ratio, seed)
    if family == "integer":
        assert rows % 4 == 0
        x = balanced(g, rows, C)
        res = (torch.randint(0, 3, (rows, C), generator=g) - 1).float() * 2
        dy = (torch.randint(0, 5, (rows, C), generator=g) - 2).float()
        w, b = _sign(g, (C,)), torch.full((C,), 0.25)
    else:
        x, res, dy = _uni(g, (rows, C), -2, 2), _uni(g, (rows, C), -2, 2), _uni(g, (rows, C), -1, 1)
        w, b = affine(g, C)
        if family == "offset":
            x = x + ratio * X_STD * (1 - 2 * (torch.arange(C) % 2)).float()
            if ratio >= 32:  # dz grows with kappa |z0 - b|: |b| = 2^-4 and |res| < 2^-3 keep the undecided band
                b, res = b.sign() * 2.0 ** -4, res / 16  # |z| <= dz inside the cap
        elif family in ("constant", "constant1000"):
            x[:, 0] = 0.5
            if family == "constant1000":  # E[x^2] - mean^2 of 1e6 may come out negative; without a ReLU
                x[:, 1] = 1000.0          # (its bound there exceeds |b|: the whole channel would be undecided)
        elif family != "uniform":
            raise ValueError(family)
    return dict(x=x.to(dtype), res=res.to(dtype), dy=dy.to(dtype), w=w, b=b)


# ------------------------------------------------------------------------------- statistics

def stats_ref(x, dim):
    """float64 mean, biased variance, mean|x| and mean x^2 over ``dim``."""
    xd = x.double()
    mean = xd.mean(dim)
    return mean, ((xd - mean.unsqueeze(dim)) ** 2).mean(dim), xd.abs().mean(dim), (xd * xd).mean(dim)


def inv_interval(var, dvar, eps):
    """(invstd, dinv): the float64 value and the derived bound of its computed counterpart."""
    inv = (var + eps).rsqrt()
    hi = ((var - dvar).clamp_min(0) + eps).rsqrt() * (1 + 4 * U32)
    lo = (var + dvar + eps).rsqrt() * (1 - 4 * U32)
    return inv, torch.maximum(hi - inv, inv - lo)


def single_pass_bounds(L, mean, var, a1, a2, eps):
    """(invstd, dmean, dinv, kappa) of the single-pass E[x^2] - mean^2 form."""
    dmean = L * E23 * a1 + 2 * U32 * mean.abs()
    kappa = a2 / var.clamp_min(1e-300)
    dvar = a2 * ((L + 3) * E23 + 4 * U32) + 2 * mean.abs() * dmean + dmean ** 2  # a2 = var kappa
    inv, dinv = inv_interval(var, dvar, eps)
    return inv, dmean, dinv, kappa


def two_pass_bounds(L, mean, var, a1, eps):
    dmean = L * E23 * a1 + 2 * U32 * mean.abs()
    dvar = var * ((L + 3) * E23 + 4 * U32) + dmean ** 2
    inv, dinv = inv_interval(var, dvar, eps)
    return inv, dmean, dinv


def affine_fwd_ref(x, w, b, res, relu, mean, inv, dmean, dinv, dtype):
    """z (float64 pre-activation), y reference, dz, dy of y = T(act(x scale + shift [+ res])). x [n, C] with
    per-channel (broadcastable) mean / inv / w / b in float64; w, b None = 1, 0."""
    xd = x.double()
    wd = torch.ones_like(mean) if w is None else w.double()
    bd = torch.zeros_like(mean) if b is None else b.double()
    scale = wd * inv
    dscale = wd.abs() * dinv + U32 * scale.abs()
    z0 = (xd - mean) * scale + bd
    z = z0 + res.double() if res is not None else z0
    dz = ((xd - mean).abs() * dscale + scale.abs() * dmean + dscale * dmean
          + 2 * U32 * ((xd * scale).abs() + (mean * scale).abs() + bd.abs() + z0.abs()))
    if res is not None:
        dz = dz + 2 * U32 * z.abs()
    y = z.clamp_min(0) if relu else z
    return z, y, dz + TINY, dz + rt(dtype, y) + TINY


def mask_bytes(pos):
    """Bit j of byte v = element 8 v + j of the flattened boolean tensor."""
    p = pos.reshape(-1, 8).to(torch.int32)
    return (p << torch.arange(8, device=p.device, dtype=torch.int32)).sum(1).to(torch.uint8)


def mask_bits(mask, shape):
    m = mask.to(torch.int32).unsqueeze(1) >> torch.arange(8, device=mask.device, dtype=torch.int32)
    return (m & 1).bool().reshape(shape)


def undecided(z, dz, name, errs):
    und = z.abs() <= dz
    n = int(und.sum())
    print(f"{name}: {n} undecided ReLU elements of {z.numel()}")
    if n > UNDECIDED_CAP * z.numel():
        errs.append(f"{name}: {n} undecided ReLU elements exceed 0.1 % of {z.numel()}")
    return und


def check_either(name, got, ref, alt, bnd, und, errs):
    """``E.check`` where an undecided element may match either reference."""
    gd = got.double()
    pick = und & ((gd - alt).abs() < (gd - ref).abs())
    E.check(name, got, torch.where(pick, alt, ref), bnd, errs)


def check_mask(name, mask, z, und, errs):
    bits = mask_bits(mask, z.shape)
    bad = (bits != (z > 0)) & ~und
    if bool(bad.any()):
        errs.append(f"{name}: {int(bad.sum())} mask bits differ from the decided reference")


def ulps32(got, ref32):
    """Distance in float32 ulps between two float32 tensors of like sign."""
    return (got.contiguous().view(torch.int32).long() - ref32.contiguous().view(torch.int32).long()).abs()


# ------------------------------------------------------------------------------- BatchNorm

def bn_check_fwd(tag, inp, out, relu, use_res, affine_on, dtype, errs, eps=1e-5, momentum=0.1, running=None,
                 exact=False):
    """One training forward: ``out`` holds mean, inv, y and optionally mask, rm, rv (kernel or emulation);
    ``running``: the (running_mean, running_var) before the call. Returns (z, dz, und)."""
    x = inp["x"]
    rows, C = x.shape
    mean, var, a1, a2 = stats_ref(x, 0)
    inv, dmean, dinv, kappa = single_pass_bounds(bn_L(rows, C), mean, var, a1, a2, eps)
    print(f"{tag}: rows {rows} C {C} kappa max {float(kappa.max()):.3g}")
    E.check(f"{tag} save_mean", out["mean"], mean, dmean + TINY, errs)
    E.check(f"{tag} save_invstd", out["inv"], inv, dinv + TINY, errs)
    rel = ((out["inv"].double() - inv).abs() / inv).max()
    print(f"{tag} save_invstd: worst relative error {float(rel):.3g}")
    w, b = (inp["w"], inp["b"]) if affine_on else (None, None)
    res = inp["res"] if use_res else None
    z, y, dz, dy = affine_fwd_ref(x, w, b, res, relu, mean, inv, dmean, dinv, dtype)
    E.check(f"{tag} y", out["y"], y, dy, errs)
    und = undecided(z, dz, tag, errs) if relu else torch.zeros_like(z, dtype=torch.bool)
    if out.get("mask") is not None:
        check_mask(f"{tag} mask", out["mask"], z, und, errs)
    unb = var * rows / max(rows - 1, 1)
    if running is not None and out.get("rm") is not None:
        rm0, rv0 = (t.double() for t in running)
        dunb = (inv ** -3) * 2 * dinv * rows / max(rows - 1, 1) + 4 * U32 * unb  # var = invstd^-2 - eps
        E.check(f"{tag} running_mean", out["rm"], (1 - momentum) * rm0 + momentum * mean,
                momentum * dmean + 4 * U32 * (rm0.abs() + mean.abs()) + TINY, errs)
        E.check(f"{tag} running_var", out["rv"], (1 - momentum) * rv0 + momentum * unb,
                momentum * dunb + 4 * U32 * (rv0.abs() + unb) + TINY, errs)
    if exact:  # the integer family: sums below 2^24, any order
        s = x.double().sum(0)
        q = (x.double() ** 2).sum(0)
        assert float(q.max()) < 2 ** 24
        inv_n = torch.tensor(1.0 / rows, dtype=torch.float32, device=x.device)
        m32 = s.float() * inv_n
        if not torch.equal(out["mean"], m32):
            errs.append(f"{tag}: save_mean is not fl(s fl(1 / n)) exactly")
        v32 = (q.float() * inv_n - m32 * m32).clamp_min(0)
        i32 = torch.rsqrt(v32 + torch.tensor(eps, dtype=torch.float32, device=x.device))
        mom = torch.tensor(momentum, dtype=torch.float32, device=x.device)
        keep = 1 - mom  # 1.f - momentum in float32, as the kernel forms it
        for name, got, ref in [("save_invstd", out["inv"], i32)] + ([] if out.get("rm") is None else [
                ("running_mean", out["rm"], keep * running[0].float() + mom * m32),
                ("running_var", out["rv"], keep * running[1].float() + mom * (v32 * float(rows) / float(rows - 1)))]):
            d = int(ulps32(got.float(), ref.float()).max())
            if d > 2:
                errs.append(f"{tag}: {name} is {d} ulp from the float32 evaluation")
        if out.get("mask") is not None and not torch.equal(out["mask"], mask_bytes(out["y"].float() > 0)):
            errs.append(f"{tag}: mask bytes differ from the bits of y > 0")
    return z, dz, und


def bn_bwd_ref(inp, mean32, inv32, g, affine_on, dtype, und=None):
    """float64 dx / dw / db of the backward from the stored statistics and g = dy_eff, with bounds.
    ``und``: elements whose ReLU decision may go either way (their |dy| widens the sums' bounds)."""
    x, dyd = inp["x"].double(), inp["dy"].double()
    rows, C = x.shape
    L = bn_L(rows, C)
    mean, inv = mean32.double(), inv32.double()
    wd = inp["w"].double() if affine_on else torch.ones_like(mean)
    xhat = (x - mean) * inv
    db, dw = g.sum(0), (g * xhat).sum(0)
    ddb = L * E23 * g.abs().sum(0)
    ddw = (L + 3) * E23 * (g * xhat).abs().sum(0)
    if und is not None:
        ddb = ddb + (dyd.abs() * und).sum(0)
        ddw = ddw + ((dyd * xhat).abs() * und).sum(0)
    A = wd * inv
    k2, k3 = db / rows, dw / rows
    dk2, dk3 = ddb / rows + 2 * U32 * k2.abs(), ddw / rows + 2 * U32 * k3.abs()
    B = -A * inv * k3
    dx = A * g + B * x + A * (mean * inv * k3 - k2)
    ddx = ((A * inv * (x - mean)).abs() * dk3 + A.abs() * dk2
           + 4 * U32 * ((B * x).abs() + (A * mean * inv * k3).abs() + (A * k2).abs() + (A * g).abs())
           + 2 * U32 * dx.abs() + rt(dtype, dx))
    return dict(dx=dx, dw=dw, db=db, ddx=ddx + TINY, ddw=ddw + TINY, ddb=ddb + TINY, A=A)


def bn_check_bwd(tag, inp, out, mean32, inv32, g, affine_on, dtype, errs, und=None, exact=False):
    """``out``: dx, dw, db and optionally dres of one backward; g the float64 dy_eff of the reference."""
    r = bn_bwd_ref(inp, mean32, inv32, g, affine_on, dtype, und)
    E.check(f"{tag} db", out["db"], r["db"], None if exact else r["ddb"], errs)
    E.check(f"{tag} dw", out["dw"], r["dw"], r["ddw"], errs)
    dyd = inp["dy"].double()
    if und is not None and bool(und.any()):
        flip = torch.where(g == 0, dyd, torch.zeros_like(dyd))  # the other decision's dy_eff
        check_either(f"{tag} dx", out["dx"], r["dx"], r["dx"] + r["A"] * (flip - g), r["ddx"], und, errs)
        if out.get("dres") is not None:
            check_either(f"{tag} dres", out["dres"], g, flip, torch.zeros_like(g), und, errs)
    else:
        E.check(f"{tag} dx", out["dx"], r["dx"], r["ddx"], errs)
        if out.get("dres") is not None:
            E.check(f"{tag} dres", out["dres"], g, None, errs)
    return r


def seqsum(t):
    """float32 sum over dim 0, one addition at a time."""
    s = torch.zeros_like(t[0])
    for i in range(t.shape[0]):
        s = s + t[i]
    return s


def lane_sum(t, rpi):
    """Rows r0, r0 + rpi, ... added in sequence per lane r0, then the lanes in sequence (float32)."""
    pad = (-t.shape[0]) % rpi
    if pad:
        t = torch.cat([t, torch.zeros(pad, *t.shape[1:])])
    return seqsum(seqsum(t.view(-1, rpi, *t.shape[1:])))


def bn_reduce_emulated(a, b, rows, C, ws, defect=None):
    """batchnorm.hip's block partials -> shards -> finalize in float32; ``ws`` [16, 2, C] persists between
    calls and is left as the kernel (or the planted defect) leaves it."""
    _, rpi, rpb, blocks = bn_geometry(rows, C)
    for blk in range(blocks):
        lo, hi = blk * rpb, min(rows, (blk + 1) * rpb)
        if defect == "drop_last_row":
            hi -= 1
        ws[blk % 16, 0] += lane_sum(a[lo:hi], rpi)
        ws[blk % 16, 1] += lane_sum(b[lo:hi], rpi)
    keep = [k for k in range(16) if not (defect == "stale_shard" and k == 0)]
    s, q = seqsum(ws[keep, 0]), seqsum(ws[keep, 1])
    ws[keep] = 0
    return s, q


def bn_emulate_fwd(inp, relu, use_res, affine_on, dtype, ws, running=None, eps=1e-5, momentum=0.1, defect=None):
    """The training forward of batchnorm.hip in float32 PyTorch (no fma), with optional planted defects."""
    x = inp["x"].float()
    rows, C = x.shape
    s, q = bn_reduce_emulated(x, x * x, rows, C, ws, defect)
    inv_n = torch.tensor(1.0 / rows, dtype=torch.float32)
    mean = s * inv_n
    var = (q * inv_n - mean * mean).clamp_min(0)
    inv = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    out = dict(mean=mean, inv=inv)
    if running is not None:
        unb = var if defect == "biased_running_var" else var * float(rows) / float(max(rows - 1, 1))
        out["rm"] = (1 - momentum) * running[0] + momentum * mean
        out["rv"] = (1 - momentum) * running[1] + momentum * unb
    sc = (inp["w"] if affine_on else torch.ones(C)) * inv
    sh = (inp["b"] if affine_on else torch.zeros(C)) - mean * sc
    if defect == "coef_off_by_vector":  # the LDS index (v * 8) % C one vector ahead
        sc, sh = sc.roll(-8), sh.roll(-8)
    o = x * sc + sh
    pos = o > 0
    if use_res:
        o = o + inp["res"].float()
    if defect != "relu_before_residual":
        pos = o > 0
    if relu:
        o = torch.where(pos, o, torch.zeros_like(o))
        bits = pos.reshape(-1, 8).flip(1) if defect == "mask_reversed" else pos
        out["mask"] = mask_bytes(bits)
    out["y"] = E.trunc_bf16(o) if defect == "truncate" else o.to(dtype)
    return out


def bn_emulate_bwd(inp, mean, inv, g32, affine_on, dtype, ws, defect=None):
    x, rows, C = inp["x"].float(), *inp["x"].shape
    xhat = (x - mean) * inv
    db, dw = bn_reduce_emulated(g32, g32 * xhat, rows, C, ws)
    inv_n = torch.tensor(1.0 / rows, dtype=torch.float32)
    sc = (inp["w"] if affine_on else torch.ones(C)) * inv
    k2, k3 = db * inv_n, dw * inv_n
    if defect == "no_mean_dy":
        k2 = torch.zeros_like(k2)
    B, D = -sc * inv * k3, sc * (mean * inv * k3 - k2)
    return dict(dx=(sc * g32 + (B * x + D)).to(dtype), dres=g32.to(dtype), dw=dw, db=db)


# ------------------------------------------------------------------------------- LayerNorm

def ln_refs(h, w, b, dtype, eps=1e-5):
    """float64 mean / rstd / y of LayerNorm over the last dim of the stored h [rows, D], with bounds."""
    D = h.shape[1]
    mean, var, a1, _ = stats_ref(h, 1)
    rstd, dmean, drstd = two_pass_bounds(ln_L(D), mean, var, a1, eps)
    hd = h.double()
    wd = torch.ones(D, dtype=torch.float64, device=h.device) if w is None else w.double()
    bd = torch.zeros(D, dtype=torch.float64, device=h.device) if b is None else b.double()
    c = hd - mean[:, None]
    y = c * rstd[:, None] * wd + bd
    dy = (wd.abs() * (c.abs() * drstd[:, None] + (rstd * dmean)[:, None] + (drstd * dmean)[:, None])
          + 3 * U32 * (c * rstd[:, None] * wd).abs() + 2 * U32 * (y.abs() + bd.abs()) + rt(dtype, y))
    return dict(mean=mean, rstd=rstd, y=y, dmean=dmean + TINY, drstd=drstd + TINY, dy=dy + TINY)


def ln_check_fwd(tag, h, w, b, out, dtype, errs, eps=1e-5):
    r = ln_refs(h, w, b, dtype, eps)
    E.check(f"{tag} mean", out["mean"], r["mean"], r["dmean"], errs)
    E.check(f"{tag} rstd", out["rstd"], r["rstd"], r["drstd"], errs)
    E.check(f"{tag} y", out["y"], r["y"], r["dy"], errs)


def ln_bwd_refs(dy, h, mean32, rstd32, w, dh_ext, dtype):
    rows, D = h.shape
    L, Lr = ln_L(D), rows + 4
    dyd, hd = dy.double(), h.double()
    wd = torch.ones(D, dtype=torch.float64, device=h.device) if w is None else w.double()
    rs = rstd32.double()[:, None]
    xh = (hd - mean32.double()[:, None]) * rs
    g = dyd * wd
    m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dm1 = (L + 2) * E23 * g.abs().mean(1, keepdim=True) + 2 * U32 * m1.abs()
    dm2 = (L + 4) * E23 * (g * xh).abs().mean(1, keepdim=True) + 2 * U32 * m2.abs()
    dx = rs * (g - m1 - xh * m2)
    ddx = rs * (dm1 + xh.abs() * dm2) + 4 * U32 * rs * (g.abs() + m1.abs() + (xh * m2).abs())
    if dh_ext is not None:
        dx = dx + dh_ext.double()
        ddx = ddx + 2 * U32 * dx.abs()
    ddx = ddx + rt(dtype, dx)
    return dict(dx=dx, ddx=ddx + TINY, dw=(dyd * xh).sum(0), ddw=(Lr + 3) * E23 * (dyd * xh).abs().sum(0) + TINY,
                db=dyd.sum(0), ddb=Lr * E23 * dyd.abs().sum(0) + TINY, Lr=Lr)


def ln_check_bwd(tag, dy, h, mean32, rstd32, w, dh_ext, out, dtype, errs, exact=False):
    """``out``: dx and the float64 sums dw, db (and cs) of the kernel's partials."""
    r = ln_bwd_refs(dy, h, mean32, rstd32, w, dh_ext, dtype)
    E.check(f"{tag} dx", out["dx"], r["dx"], r["ddx"], errs)
    E.check(f"{tag} dw", out["dw"], r["dw"], r["ddw"], errs)
    E.check(f"{tag} db", out["db"], r["db"], None if exact else r["ddb"], errs)
    if out.get("cs") is not None:  # of the stored dx
        sd = out["dx"].double()
        E.check(f"{tag} colsum", out["cs"], sd.sum(0), r["Lr"] * E23 * sd.abs().sum(0) + TINY, errs)


def ln_lanes(t, defect=None):
    """(lanes, wave): ``t`` [rows, D] float32 laid out as layernorm.hip holds it, [rows, slot i, lane, j] (lane l
    holds vectors l, l + 64, ...; a masked lane re-reads vector 0), and the wave sum of such a tensor: every
    lane adds its 8 VPL values in sequence, then the lanes are added in sequence (masked slots count as 0)."""
    rows, D = t.shape
    nv, vpl = D // 8, ln_vpl(D)
    idx = torch.arange(vpl * 64)
    act = idx < nv
    pick = torch.where(act, idx, torch.zeros_like(idx))
    use = torch.ones_like(act) if defect == "masked_lane_counted" else act
    m = use.view(1, vpl, 64, 1).float()

    def lanes(u):
        return u.reshape(rows, nv, 8)[:, pick].view(rows, vpl, 64, 8)

    def wave(u):
        return seqsum(seqsum((u * m).permute(1, 3, 0, 2).reshape(vpl * 8, rows, 64)).t())

    return lanes, wave


def ln_emulate_fwd(x, r, w, b, dtype, eps=1e-5, defect=None):
    """layernorm.hip's forward in float32 with its lane layout."""
    rows, D = x.shape
    h = x.float() if r is None else (x.float() + r.float()).to(dtype).float()
    to_lanes, wave = ln_lanes(h, defect)
    lanes = to_lanes(h)

    inv_d = torch.tensor(1.0 / D, dtype=torch.float32)
    mean = wave(lanes) * inv_d
    d = lanes - mean.view(rows, 1, 1, 1)
    rstd = torch.rsqrt(wave(d * d) * inv_d + torch.tensor(eps, dtype=torch.float32))
    wv = torch.ones(D) if w is None else w.float()
    bv = torch.zeros(D) if b is None else b.float()
    y = ((h - mean[:, None]) * rstd[:, None] * wv + bv).to(dtype)
    return dict(h=h.to(dtype), y=y, mean=mean, rstd=rstd)


def ln_emulate_bwd(dy, h, mean, rstd, w, dh_ext, dtype):
    """layernorm.hip's backward in float32: the two wave sums per row, dx, and dw / db / column sums added
    row after row (one wave walking every row: the longest chain the grid allows)."""
    rows, D = h.shape
    to_lanes, wave = ln_lanes(h.float())
    d, hf = dy.float(), h.float()
    wv = torch.ones(D) if w is None else w.float()
    xh = (hf - mean[:, None]) * rstd[:, None]
    g = d * wv
    inv_d = torch.tensor(1.0 / D, dtype=torch.float32)
    m1, m2 = wave(to_lanes(g)) * inv_d, wave(to_lanes(g * xh)) * inv_d
    dx = rstd[:, None] * (g - m1[:, None] - xh * m2[:, None])
    if dh_ext is not None:
        dx = dx + dh_ext.float()
    dx = dx.to(dtype)
    return dict(dx=dx, dw=seqsum(d * xh), db=seqsum(d), cs=seqsum(dx.float()) if dh_ext is not None else None)


# ------------------------------------------------------------------------------- GroupNorm

def gn_h(x, a, relu):
    """The stored h = T(act(fl32(x + a))) exactly as the kernel rounds it."""
    v = x.float()
    if a is not None:
        v = v + a.float()
    if relu:
        v = v.clamp_min(0)
    return v.to(x.dtype)


def gn_groups(t, G):
    """[N, HW, C] -> [N, G, HW * cpg]."""
    N, HW, C = t.shape
    return t.view(N, HW, G, C // G).permute(0, 2, 1, 3).reshape(N, G, -1)


def gn_refs(h, w, b, G, dtype, eps=1e-5, L=None):
    """h [N, HW, C] (the stored h). float64 mean / rstd [N, G], y [N, HW, C] and their bounds. ``L``: the
    per-group reduction length L_gn of another kernel (default: groupnorm.hip's)."""
    N, HW, C = h.shape
    cpg = C // G
    mean, var, a1, a2 = stats_ref(gn_groups(h, G), 2)
    rstd, dmean, drstd, kappa = single_pass_bounds(gn_Lpx(HW, C, G) + cpg if L is None else L, mean, var, a1, a2, eps)
    print(f"    kappa max {float(kappa.max()):.3g}")
    ex = lambda t: t.repeat_interleave(cpg, 1)[:, None, :]  # [N, G] -> [N, 1, C]
    _, y, _, dy = affine_fwd_ref(h, w, b, None, False, ex(mean), ex(rstd), ex(dmean), ex(drstd), dtype)
    return dict(mean=mean, rstd=rstd, y=y, dmean=dmean + TINY, drstd=drstd + TINY, dy=dy)


def gn_check_fwd(tag, h, w, b, G, out, dtype, errs, eps=1e-5, L=None):
    r = gn_refs(h, w, b, G, dtype, eps, L)
    E.check(f"{tag} mean", out["mean"], r["mean"], r["dmean"], errs)
    E.check(f"{tag} rstd", out["rstd"], r["rstd"], r["drstd"], errs)
    E.check(f"{tag} y", out["y"], r["y"], r["dy"], errs)


def gn_bwd_refs(dy, h, mean32, rstd32, w, G, relu, dtype, Lpx=None):
    """The float64 backward from the stored h and statistics and the gradient dy [N, HW, C] (any float
    dtype), with its bounds: dict(dh, ddh (the stored dh's, u_T |dh| included), dw, ddw, db, ddb).
    ``Lpx``: the per-channel reduction length L_px of another kernel (default: groupnorm.hip's)."""
    N, HW, C = h.shape
    cpg, M, Lp = C // G, HW * (C // G), gn_Lpx(HW, C, G) if Lpx is None else Lpx
    dyd, hd = dy.double(), h.double()
    wd = torch.ones(C, dtype=torch.float64, device=h.device) if w is None else w.double()
    ex = lambda t: t.double().repeat_interleave(cpg, 1)  # [N, G] -> [N, C]
    mu, rs = ex(mean32), ex(rstd32)
    S, Q = dyd.sum(1), (dyd * hd).sum(1)
    dS, dQ = Lp * E23 * dyd.abs().sum(1), (Lp + 1) * E23 * (dyd * hd).abs().sum(1)
    dw = rs * (Q - mu * S)
    ddw = rs * (dQ + mu.abs() * dS + 2 * U32 * (Q.abs() + 2 * (mu * S).abs())) + 2 * U32 * dw.abs()
    grp = lambda t: t.view(N, G, cpg).sum(2).repeat_interleave(cpg, 1)  # group sums, per channel
    m1, m2 = grp(wd * S) / M, grp(wd * dw) / M
    dm1 = (grp(wd.abs() * dS) + (cpg + 2) * E23 * grp((wd * S).abs())) / M
    dm2 = (grp(wd.abs() * ddw) + (cpg + 3) * E23 * grp((wd * dw).abs())) / M
    xh = (hd - mu[:, None]) * rs[:, None]
    dh = rs[:, None] * (dyd * wd - m1[:, None] - xh * m2[:, None])
    ddh = (rs[:, None] * (dm1[:, None] + xh.abs() * dm2[:, None])
           + 4 * U32 * rs[:, None] * ((dyd * wd).abs() + m1.abs()[:, None] + (xh * m2[:, None]).abs()))
    if relu:
        dh, ddh = dh * (hd > 0), ddh * (hd > 0)
    return dict(dh=dh, ddh=ddh + rt(dtype, dh) + TINY, dw=dw, ddw=ddw, db=S, ddb=dS)


def gn_check_bwd(tag, dy, h, mean32, rstd32, w, G, relu, out, dtype, errs, exact=False, Lpx=None):
    """``out``: dh [N, HW, C] and optionally part [N, 2, C] (dw, db per sample). Returns the per-sample
    references and bounds (dw, ddw, db, ddb)."""
    r = gn_bwd_refs(dy, h, mean32, rstd32, w, G, relu, dtype, Lpx)
    dw, ddw, S, dS = r["dw"], r["ddw"], r["db"], r["ddb"]
    E.check(f"{tag} dh", out["dh"], r["dh"], r["ddh"], errs)
    if out.get("part") is not None:
        E.check(f"{tag} dw", out["part"][:, 0], dw, ddw + TINY, errs)
        E.check(f"{tag} db", out["part"][:, 1], S, None if exact else dS + TINY, errs)
    return dw, ddw, S, dS


def gn_emulate_fwd(h, w, b, G, dtype, eps=1e-5, defect=None):
    """groupnorm.hip's statistics and apply pass in float32 on the stored h [N, HW, C]."""
    N, HW, C = h.shape
    cpg, pl = C // G, gn_pl(C, G)
    hf = h.float()
    s = torch.stack([lane_sum(hf[n], pl) for n in range(N)])           # [N, C]
    q = torch.stack([lane_sum(hf[n] * hf[n], pl) for n in range(N)])
    gs, gq = seqsum(s.view(N, G, cpg).permute(2, 0, 1)), seqsum(q.view(N, G, cpg).permute(2, 0, 1))
    inv_m = torch.tensor(1.0 / (HW * cpg), dtype=torch.float32)
    mu = gs * inv_m
    r = torch.rsqrt((gq * inv_m - mu * mu).clamp_min(0) + torch.tensor(eps, dtype=torch.float32))
    c = torch.arange(C)
    gi = (c // 8 * 8) // cpg if defect == "group_per_vector" else c // cpg
    sc = r[:, gi] * (torch.ones(C) if w is None else w.float())
    sh = (torch.zeros(C) if b is None else b.float()) - mu[:, gi] * sc
    return dict(mean=mu, rstd=r, y=(hf * sc[:, None] + sh[:, None]).to(dtype))


def gn_emulate_bwd(dy, h, mean, rstd, w, G, relu, dtype):
    """groupnorm.hip's backward in float32 on the stored h, statistics and dy [N, HW, C]."""
    N, HW, C = h.shape
    cpg, pl = C // G, gn_pl(C, G)
    d, hf = dy.float(), h.float()
    wv = torch.ones(C) if w is None else w.float()
    S = torch.stack([lane_sum(d[n], pl) for n in range(N)])
    Q = torch.stack([lane_sum(d[n] * hf[n], pl) for n in range(N)])
    gi = torch.arange(C) // cpg
    mu, rs = mean[:, gi], rstd[:, gi]
    dw = rs * (Q - mu * S)
    inv_m = torch.tensor(1.0 / (HW * cpg), dtype=torch.float32)
    s1 = seqsum((wv * S).view(N, G, cpg).permute(2, 0, 1)) * inv_m
    s2 = seqsum((wv * rs * (Q - mu * S)).view(N, G, cpg).permute(2, 0, 1)) * inv_m
    xh = (hf - mu[:, None]) * rs[:, None]
    dh = rs[:, None] * (d * wv - s1[:, gi][:, None] - xh * s2[:, gi][:, None])
    if relu:
        dh = torch.where(hf > 0, dh, torch.zeros_like(dh))
    return dict(dh=dh.to(dtype), part=torch.stack([dw, S], 1))


# ------------------------------------------------------------------------------- pool

def pool_inputs(n, c, h, w, dtype, seed=0):
    """x on the grid {-2, -1.5, .. 2} with whole windows <= 0 (a block of -1), scale +-2^k, shift k / 4."""
    g = _g("pool", n, c, h, w, seed)
    x = (torch.randint(0, 9, (n, h, w, c), generator=g) - 4).float() / 2
    x[:, : min(3, h), : min(3, w)] = -1.0
    scale = _sign(g, (c,)) * 2.0 ** torch.randint(-2, 2, (c,), generator=g).float()
    shift = (torch.randint(0, 5, (c,), generator=g) - 2).float() / 4
    x[..., 0] = x[..., 0].abs() * -scale[0].sign()  # channel 0: z <= shift[0] everywhere ...
    shift[0] = -0.25                                # ... so every window of it is blocked
    return x.to(dtype), scale, shift


def pool_ref(x, scale, shift, k, s, p, defect=None):
    """(y, idx) [n, oh, ow, c] of relu(max over the window of x scale + shift), NHWC float32 x on the grid
    (exact): first maximum in scan order (kh outer, kw inner), 0xFF where the maximum is <= 0."""
    n, h, w, c = x.shape
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    z = x.float() * scale + shift
    best = torch.full((n, oh, ow, c), -math.inf)
    arg = torch.zeros((n, oh, ow, c), dtype=torch.int64)
    flat = z.reshape(n, h * w, c)
    for i in range(oh):
        for j in range(ow):
            for kh in range(k):
                for kw in range(k):
                    hh, ww = i * s - p + kh, j * s - p + kw
                    if hh < 0 or hh >= h or ww < 0:
                        continue
                    if ww >= w:
                        if defect != "border_wrap" or hh * w + ww >= h * w:
                            continue
                    v = flat[:, hh * w + ww]  # == z[:, hh, ww] inside the image; the wrap reads the next row
                    take = (v >= best[:, i, j]) if defect == "last_max" else (v > best[:, i, j])
                    best[:, i, j] = torch.where(take, v, best[:, i, j])
                    arg[:, i, j] = torch.where(take, torch.full_like(arg[:, i, j], kh * k + kw), arg[:, i, j])
    pos = best > 0
    return torch.where(pos, best, torch.zeros_like(best)), torch.where(pos, arg, torch.full_like(arg, 255))


def pool_bwd_ref(dy, idx, h, w, k, s, p):
    """dz [n, h, w, c] (float64): every pooled gradient scattered to its recorded argmax."""
    n, oh, ow, c = dy.shape
    dz = torch.zeros(n, h, w, c, dtype=torch.float64)
    for i in range(oh):
        for j in range(ow):
            a = idx[:, i, j]
            for kk in range(k * k):
                hh, ww = i * s - p + kk // k, j * s - p + kk % k
                if 0 <= hh < h and 0 <= ww < w:
                    dz[:, hh, ww] += torch.where(a == kk, dy[:, i, j].double(), torch.zeros((), dtype=torch.float64))
    return dz


def pool_check(tag, y, idx, x, scale, shift, k, s, p, errs):
    yr, ir = pool_ref(x, scale, shift, k, s, p)
    E.check(f"{tag} y", y, yr.double(), None, errs)
    E.check(f"{tag} idx", idx, ir.double(), None, errs)
    return ir
