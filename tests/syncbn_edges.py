"""Shards, float64 references of the concatenated batch, derived bounds and a float32 emulation for the
synchronised BatchNorm (``fluxmpi_amd/ops/syncbn.py``; the deterministic tail, fold and finalize kernels of
batchnorm.hip), shared by ``test_syncbn.py`` and ``test_syncbn_gpu.py`` (plain helper: no fixtures, no tests).
Everything numeric is ``norm_edges``' (unit roundoffs, E = 2^-23 per addition, the single-pass statistics,
the forward and backward forms, the undecided band); only the reduction length differs. Nothing is fitted.

Reduction length of the deterministic scheme (a closed form that may over-count, never read from the
extension). One shard of R rows and C channels:

    cv = C / 8, rpi = max(1, 256 // cv) rows in flight per workgroup,
    min_rows = max(ceil(32768 / C), 32), B0 = min(max(1, ceil(R / min_rows)), 512) workgroups asked for,
    rows per workgroup rpb = ceil(ceil(R / B0) / rpi) rpi, B = ceil(R / rpb) partials (a function of (R, C) alone)

      the lane's chain            rpb / rpi + 1 rows (its accumulator starts at 0)
      lane partials per workgroup rpi
      the fold's longest chain    ceil(B / 16) partials per fold group + 16 group sums
    L_shard(R, C) = rpb / rpi + 1 + rpi + ceil(B / 16) + 16

W shards summed across ranks (in any order: at most W - 1 additions on a value's path), and the global sum
of terms t errs by at most sum_r L_shard(R_r) E sum_{i in r} |t_i| + (W - 1) E sum|t|:

    L_sync = max_r L_shard(R_r, C) + (W - 1)            (an empty shard contributes exact zeros)

The PyTorch fallback of the same protocol sums a shard in an order of torch's choosing: at most R_r - 1
additions on a path, L_torch = max_r R_r + (W - 1).

Backward: the dx pass takes k2 = fl(S_g fl(1 / n)) and k3 likewise from the summed message and the global count n.
The kernels form them in a scale kernel with exactly the two roundings of the one-shard kernel and launch the
dx kernel with rows = 1 (its 1 / rows is 1.f, its products exact); the other route (sums scaled by
n_local / n_global) costs one more rounding, and the bound charges that one too, whichever route runs:
dk = dS / n + 3u |k| where ``norm_edges`` has 2u.

Exact family (``integer``: x in {+-1, +-2}, dy in {-2 .. 2}, sums of |x|, x^2, |g| below 2^24): every partial
sum of integers is exact in any order, so each shard's forward message and the sum-of-g half of the backward
message equal the float64 sums, and W shards give the bits of one shard.
"""
import torch

from . import mfma_edges as E
from . import norm_edges as N
from .norm_edges import E23, TINY, U32, ceil_div

RADIX = 4096
FOLD_GROUPS = 16
MAX_BLOCKS = 512
FLOOR_ROWS = 32


def det_geometry(rows, C):
    """(cv, rpi, rows_per_block, blocks) of the deterministic reductions: a function of (rows, C) alone."""
    cv = C // 8
    rpi = max(1, 256 // cv)
    min_rows = max(ceil_div(32768, C), FLOOR_ROWS)
    b0 = min(max(1, ceil_div(rows, min_rows)), MAX_BLOCKS)
    rpb = ceil_div(ceil_div(rows, b0), rpi) * rpi
    return cv, rpi, rpb, ceil_div(rows, rpb)


def L_shard(rows, C):
    if rows == 0:
        return 0
    _, rpi, rpb, blocks = det_geometry(rows, C)
    return rpb // rpi + 1 + rpi + ceil_div(blocks, FOLD_GROUPS) + FOLD_GROUPS


def L_sync(shard_rows, C):
    return max(L_shard(r, C) for r in shard_rows) + len(shard_rows) - 1


def L_torch(shard_rows):
    return max(shard_rows) + len(shard_rows) - 1


def split(inp, shard_rows):
    """The global inputs ``rows_inputs`` made, cut into consecutive shards (w, b shared)."""
    assert sum(shard_rows) == inp["x"].shape[0]
    out, lo = [], 0
    for r in shard_rows:
        out.append({k: (v[lo:lo + r] if k in ("x", "res", "dy") else v) for k, v in inp.items()})
        lo += r
    return out


def message_ref(x):
    """float64 (sum x, sum x^2) and the count slots of one shard."""
    xd = x.double()
    return xd.sum(0), (xd * xd).sum(0), x.shape[0] // RADIX, x.shape[0] % RADIX


def count_of(msg):
    return int(msg[-2].item()) * RADIX + int(msg[-1].item())


# ------------------------------------------------------------------------------- forward

def fwd_refs(inp, L, relu, use_res, affine_on, dtype, eps=1e-5):
    """The float64 forward of the whole batch ``inp`` with the bounds of reduction length ``L``."""
    x = inp["x"]
    mean, var, a1, a2 = N.stats_ref(x, 0)
    inv, dmean, dinv, kappa = N.single_pass_bounds(L, mean, var, a1, a2, eps)
    w, b = (inp["w"], inp["b"]) if affine_on else (None, None)
    z, y, dz, dy = N.affine_fwd_ref(x, w, b, inp["res"] if use_res else None, relu, mean, inv, dmean, dinv, dtype)
    return dict(mean=mean, var=var, inv=inv, dmean=dmean, dinv=dinv, kappa=kappa, z=z, y=y, dz=dz, dy=dy)


def check_fwd(tag, inp, out, L, relu, use_res, affine_on, dtype, errs, eps=1e-5, momentum=0.1, running=None):
    """``out``: mean, inv, y [rows, C] of the whole batch (the shards' outputs concatenated) and optionally
    mask (bytes or bool), rm, rv; ``running`` the running statistics before the call. Returns (z, dz, und)."""
    rows = inp["x"].shape[0]
    r = fwd_refs(inp, L, relu, use_res, affine_on, dtype, eps)
    print(f"{tag}: rows {rows} L {L} kappa max {float(r['kappa'].max()):.3g}")
    E.check(f"{tag} save_mean", out["mean"], r["mean"], r["dmean"] + TINY, errs)
    E.check(f"{tag} save_invstd", out["inv"], r["inv"], r["dinv"] + TINY, errs)
    E.check(f"{tag} y", out["y"], r["y"], r["dy"], errs)
    und = N.undecided(r["z"], r["dz"], tag, errs) if relu else torch.zeros_like(r["z"], dtype=torch.bool)
    m = out.get("mask")
    if m is not None:
        if m.dtype == torch.bool:
            bad = (m != (r["z"] > 0)) & ~und
            if bool(bad.any()):
                errs.append(f"{tag} mask: {int(bad.sum())} decisions differ from the decided reference")
        else:
            N.check_mask(f"{tag} mask", m, r["z"], und, errs)
    if running is not None and out.get("rm") is not None:
        unb = r["var"] * rows / max(rows - 1, 1)
        rm0, rv0 = (t.double() for t in running)
        dunb = (r["inv"] ** -3) * 2 * r["dinv"] * rows / max(rows - 1, 1) + 4 * U32 * unb
        E.check(f"{tag} running_mean", out["rm"], (1 - momentum) * rm0 + momentum * r["mean"],
                momentum * r["dmean"] + 4 * U32 * (rm0.abs() + r["mean"].abs()) + TINY, errs)
        E.check(f"{tag} running_var", out["rv"], (1 - momentum) * rv0 + momentum * unb,
                momentum * dunb + 4 * U32 * (rv0.abs() + unb) + TINY, errs)
    return r["z"], r["dz"], und


# ------------------------------------------------------------------------------- backward

def bwd_refs(inp, mean32, inv32, g, L, affine_on, dtype, und=None):
    """float64 dx / dw / db of the whole batch from the stored statistics and g = dy_eff: ``norm_edges.bn_bwd_ref``
    with the reduction length ``L`` and the extra rounding of k2 / k3 (3u where it has 2u)."""
    x, dyd = inp["x"].double(), inp["dy"].double()
    rows = x.shape[0]
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
    dk2, dk3 = ddb / rows + 3 * U32 * k2.abs(), ddw / rows + 3 * U32 * k3.abs()
    B = -A * inv * k3
    dx = A * g + B * x + A * (mean * inv * k3 - k2)
    ddx = ((A * inv * (x - mean)).abs() * dk3 + A.abs() * dk2
           + 4 * U32 * ((B * x).abs() + (A * mean * inv * k3).abs() + (A * k2).abs() + (A * g).abs())
           + 2 * U32 * dx.abs() + N.rt(dtype, dx))
    return dict(dx=dx, dw=dw, db=db, ddx=ddx + TINY, ddw=ddw + TINY, ddb=ddb + TINY, A=A)


def check_bwd(tag, inp, out, mean32, inv32, g, L, affine_on, dtype, errs, und=None, exact=False):
    """``out``: dx [rows, C] (the shards' concatenated), dw, db (summed over the shards), optionally dres."""
    r = bwd_refs(inp, mean32, inv32, g, L, affine_on, dtype, und)
    E.check(f"{tag} db", out["db"], r["db"], None if exact else r["ddb"], errs)
    E.check(f"{tag} dw", out["dw"], r["dw"], r["ddw"], errs)
    dyd = inp["dy"].double()
    if und is not None and bool(und.any()):
        flip = torch.where(g == 0, dyd, torch.zeros_like(dyd))
        N.check_either(f"{tag} dx", out["dx"], r["dx"], r["dx"] + r["A"] * (flip - g), r["ddx"], und, errs)
        if out.get("dres") is not None:
            N.check_either(f"{tag} dres", out["dres"], g, flip, torch.zeros_like(g), und, errs)
    else:
        E.check(f"{tag} dx", out["dx"], r["dx"], r["ddx"], errs)
        if out.get("dres") is not None:
            E.check(f"{tag} dres", out["dres"], g, None, errs)
    return r


def recomputed_g(inp, mean32, inv32, affine_on, dtype, tag, errs):
    """(g, und) of a ReLU whose mask the backward recomputes from x and the STORED statistics."""
    zero = torch.zeros((), dtype=torch.float64, device=inp["x"].device)
    w, b = (inp["w"], inp["b"]) if affine_on else (None, None)
    z2, _, dz2, _ = N.affine_fwd_ref(inp["x"], w, b, None, True, mean32.double(), inv32.double(), zero, zero, dtype)
    und = N.undecided(z2, dz2, tag, errs)
    return inp["dy"].double() * (z2 > 0), und


# ------------------------------------------------------------------------------- float32 emulation

def fold_emulated(parts):
    """[B, C] float32 partials -> [C]: group g adds partials g, g + 16, ... in sequence, then the 16 group sums
    are added 0, 1, ... 15 (groups past B hold 0)."""
    groups = []
    for g in range(FOLD_GROUPS):
        sel = parts[g::FOLD_GROUPS]
        groups.append(N.seqsum(sel) if sel.shape[0] else torch.zeros_like(parts[0]))
    return N.seqsum(torch.stack(groups))


def reduce_emulated(t, C):
    """One shard's deterministic row reduction of ``t`` [rows, C] in float32 (no fma)."""
    rows = t.shape[0]
    _, rpi, rpb, blocks = det_geometry(rows, C)
    parts = torch.stack([N.lane_sum(t[b * rpb:min(rows, (b + 1) * rpb)], rpi) for b in range(blocks)])
    return fold_emulated(parts)


def emulate_messages(shards):
    """The summed forward message (s, q, n) of the shards, rank after rank."""
    C = shards[0]["x"].shape[1]
    s, q, n = torch.zeros(C), torch.zeros(C), 0
    for sh in shards:
        x = sh["x"].float()
        if x.shape[0]:
            s, q = s + reduce_emulated(x, C), q + reduce_emulated(x * x, C)
        n += x.shape[0]
    return s, q, n


def emulate_finalize(s, q, n, eps=1e-5, momentum=0.1, running=None):
    inv_n = torch.tensor(1.0 / float(torch.tensor(n, dtype=torch.int64).float()), dtype=torch.float32)
    mean = s * inv_n
    var = (q * inv_n - mean * mean).clamp_min(0)
    out = dict(mean=mean, inv=torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32)))
    if running is not None:
        unb = var * float(n) / float(max(n - 1, 1))
        out["rm"] = (1 - momentum) * running[0] + momentum * mean
        out["rv"] = (1 - momentum) * running[1] + momentum * unb
    return out


def emulate(shards, relu, use_res, affine_on, dtype, running=None, eps=1e-5, momentum=0.1):
    """The whole synchronised forward + backward of the shards in float32 PyTorch (fixed-order fold, no fma):
    (fwd out of the whole batch, bwd out with dx concatenated and dw / db summed, g32)."""
    C = shards[0]["x"].shape[1]
    s, q, n = emulate_messages(shards)
    out = emulate_finalize(s, q, n, eps, momentum, running)
    mean, inv = out["mean"], out["inv"]
    w = shards[0]["w"] if affine_on else torch.ones(C)
    b = shards[0]["b"] if affine_on else torch.zeros(C)
    sc = w * inv
    sh = b - mean * sc
    ys, gs, poss, sg, sgx = [], [], [], torch.zeros(C), torch.zeros(C)
    for shd in shards:
        x = shd["x"].float()
        o = x * sc + sh
        if use_res:
            o = o + shd["res"].float()
        pos = o > 0
        poss.append(pos)
        if relu:
            o = torch.where(pos, o, torch.zeros_like(o))
        ys.append(o.to(dtype))
        g = shd["dy"].float() * (pos if relu else 1)
        gs.append(g)
        if x.shape[0]:
            sg, sgx = sg + reduce_emulated(g, C), sgx + reduce_emulated(g * ((x - mean) * inv), C)
    out["y"] = torch.cat(ys)
    g32 = torch.cat(gs)
    out["mask"] = torch.cat(poss) if relu else None
    inv_n = torch.tensor(1.0 / float(torch.tensor(n, dtype=torch.int64).float()), dtype=torch.float32)
    k2, k3 = sg * inv_n, sgx * inv_n
    B, D = -sc * inv * k3, sc * (mean * inv * k3 - k2)
    x_all = torch.cat([s_["x"] for s_ in shards]).float()
    back = dict(dx=(sc * g32 + (B * x_all + D)).to(dtype), dres=g32.to(dtype), dw=sgx, db=sg)
    return out, back, g32


# ------------------------------------------------------------------------------- one process plays W ranks

MODES = {"none": (False, False), "relu": (True, False), "relu_res": (True, True)}


class OpPlayer:
    """The op-level functions of ``fluxmpi_amd.ops.syncbn`` (HIP kernels on GPU tensors, PyTorch elsewhere)."""

    def __init__(self):
        from fluxmpi_amd.ops import syncbn
        self.S = syncbn

    def fwd_msg(self, sh):
        return self.S.forward_message(sh["x"])

    def apply(self, sh, msg, relu, use_res, affine_on, running, eps, momentum):
        w, b = (sh["w"], sh["b"]) if affine_on else (None, None)
        rm, rv = (running[0].clone(), running[1].clone()) if running is not None else (None, None)
        y, mask, mean, inv = self.S.apply_from_message(sh["x"], msg, w, b, rm, rv, momentum, eps, relu,
                                                       sh["res"] if use_res else None)
        return dict(y=y, mask=mask, mean=mean, inv=inv, rm=rm, rv=rv)

    def bwd_msg(self, sh, fw, relu, affine_on):
        w, b = (sh["w"], sh["b"]) if affine_on else (None, None)
        return self.S.backward_message(sh["dy"], sh["x"], fw["mask"], w, b, fw["mean"], fw["inv"], relu)

    def dx(self, sh, fw, msg, count, relu, want_dres, affine_on):
        w, b = (sh["w"], sh["b"]) if affine_on else (None, None)
        return self.S.dx_from_message(sh["dy"], sh["x"], fw["mask"], w, b, fw["mean"], fw["inv"], msg, count, relu,
                                      want_dres)


def rank_sum(msgs):
    """The cross-rank SUM, rank after rank (float32)."""
    tot = msgs[0].clone()
    for m in msgs[1:]:
        tot = tot + m
    return tot


def play(P, shards, mode, affine_on, running, errs, tag, eps=1e-5, momentum=0.1, local_count=False):
    """Forward and backward of every shard through ``P`` with the messages summed by hand. Returns (fwd, bwd):
    the whole batch's y / mask / dx / dres concatenated in shard order, the statistics every shard was handed
    (checked to be the same bits on each), dw / db summed over the shards, and the messages.
    ``local_count`` (one shard only): the dx pass takes the shard's own sums and row count (the world-size-1 path)."""
    relu, use_res = MODES[mode]
    fmsgs = [P.fwd_msg(s) for s in shards]
    ftot = rank_sum(fmsgs)
    fws = [P.apply(s, ftot, relu, use_res, affine_on, running, eps, momentum) for s in shards]
    for k in ("mean", "inv", "rm", "rv"):
        if fws[0][k] is not None and not all(torch.equal(fws[0][k], f[k]) for f in fws[1:]):
            errs.append(f"{tag}: the shards were handed different {k}")
    bms = [P.bwd_msg(s, f, relu, affine_on) for s, f in zip(shards, fws)]
    btot = rank_sum([m[0] for m in bms])
    count = None if local_count else ftot[-2:].clone()
    dxs = [P.dx(s, f, btot, count, relu, use_res, affine_on) for s, f in zip(shards, fws)]
    masks = [f["mask"] for f in fws if f["mask"] is not None]
    fwd = dict(mean=fws[0]["mean"], inv=fws[0]["inv"], rm=fws[0]["rm"], rv=fws[0]["rv"],
               y=torch.cat([f["y"] for f in fws]), mask=torch.cat(masks) if masks else None, msgs=fmsgs, msg=ftot)
    bwd = dict(dx=torch.cat([d[0] for d in dxs]), dres=torch.cat([d[1] for d in dxs]) if use_res else None,
               dw=rank_sum([m[1] for m in bms]), db=rank_sum([m[2] for m in bms]), msgs=[m[0] for m in bms], msg=btot)
    return fwd, bwd


def check_play(tag, inp, fwd, bwd, L, mode, affine_on, dtype, errs, running=None, eps=1e-5, momentum=0.1,
               exact=False):
    """Every output of :func:`play` against the float64 reference of the whole batch ``inp``."""
    relu, use_res = MODES[mode]
    rows, C = inp["x"].shape
    _, _, und = check_fwd(tag, inp, fwd, L, relu, use_res, affine_on, dtype, errs, eps, momentum, running)
    mean32, inv32 = fwd["mean"], fwd["inv"]
    und_b = None
    if not relu:
        g = inp["dy"].double()
    elif fwd["mask"] is not None:  # the stored decision is an input of the backward
        m = fwd["mask"]
        g = inp["dy"].double() * (m if m.dtype == torch.bool else N.mask_bits(m, (rows, C)))
    else:
        g, und_b = recomputed_g(inp, mean32, inv32, affine_on, dtype, tag + " recomputed mask", errs)
    check_bwd(tag + " bwd", inp, bwd, mean32, inv32, g, L, affine_on, dtype, errs, und_b, exact)
    return g
