"""Inputs, float64 references, derived bounds, float32 emulations and planted defects shared by
``test_stem_edges_gpu.py`` (plain helper module: no fixtures, no tests; made on the CPU, seeded, nothing
here touches the GPU extension). The generic pieces (``bound``, ``check``, ``check_out``, ``check_colsums``,
guard bands, ``patterns``, ``rn_bf16``) are ``mfma_edges``'; this module adds what is particular to
``stem.hip`` (the packed-K im2col, the pool-gradient gather, the three GEMMs and their combine) and to
``conv_c3.hip``. ``test_stem_edges_gpu.py``'s docstring derives every bound used here.
"""
import math

import torch

from . import mfma_edges as E
from .mfma_edges import E23, TINY

CO, KK = 64, 256
IH = IW = 224
OH = OW = 112
PH = PW = 56
PIX = OH * OW                 # conv-output pixels per image
PART = 2 * KK * CO + KK       # floats of one workgroup's partial: G1 [256][64], G2 [256][64], G3 [256]
NNZ = 96                      # non-zero taps per filter of the ternary stem family: |y| <= 96; E[y^2] = 64 per pixel
BN_EPS = 1e-5


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------- the packed K layout

def k_offsets():
    """Per packed k: (image row offset, image column offset, channel) relative to (2 oy, 2 ox), as the kernel
    header defines them: k = 8 kc + e, kc = (by * 4 + ax) * 4 + ay, e = bx * 4 + c; row 2 ay + by - 4, column
    2 ax + bx - 4. The 7x7 tap is (ky, kx) = offsets + 3; ky = -1 or kx = -1 and c = 3 are pseudo-taps."""
    k = torch.arange(KK)
    kc, e = k >> 3, k & 7
    ay, ax, by = kc & 3, (kc >> 2) & 3, kc >> 4
    bx, c = e >> 2, e & 3
    return 2 * ay + by - 4, 2 * ax + bx - 4, c


def real_taps():
    dy, dx, c = k_offsets()
    return (dy >= -3) & (dx >= -3) & (c < 3)


def im2col(x4, dtype=torch.float64, shift_k=None, raw_border_k=None, odd_row_shift=0):
    """``A [n * 12544, 256]`` of the NHWC4 image ``x4 [n, 224, 224, 4]``: ``ops.stem.emulate_conv``'s gather in
    ``dtype``. Planted defects: ``shift_k`` reads one column too far at that k; ``raw_border_k`` clamps the
    column at that k instead of zeroing it; ``odd_row_shift`` moves the image row of every odd conv row."""
    n = x4.shape[0]
    xf = x4.to(dtype)
    dy, dx, c = k_offsets()
    oy, ox = torch.arange(OH), torch.arange(OW)
    a = torch.empty(n, PIX, KK, dtype=dtype)
    for k in range(KK):
        iy = 2 * oy + int(dy[k]) + odd_row_shift * (oy & 1)
        ix = 2 * ox + int(dx[k]) + (1 if k == shift_k else 0)
        vy = (iy >= 0) & (iy < IH)
        vx = (ix >= 0) & (ix < IW) if k != raw_border_k else torch.ones_like(ix, dtype=torch.bool)
        g = xf[:, iy.clamp(0, IH - 1)][:, :, ix.clamp(0, IW - 1), int(c[k])]
        a[:, :, k] = torch.where(vy[:, None] & vx[None, :], g, torch.zeros((), dtype=dtype)).reshape(n, PIX)
    return a.view(n * PIX, KK)


def pack_nat(w, dtype=torch.float64):
    """[64, 3, 7, 7] -> W' [64, 256] with NATURAL channel rows (the kernel's operand is ``ops.stem.pack_filter``,
    the same entries with the rows permuted; the reference does not use it, so it tests it)."""
    dy, dx, c = k_offsets()
    real = real_taps()
    wp = torch.zeros(CO, KK, dtype=dtype)
    wp[:, real] = w.to(dtype)[:, c[real], dy[real] + 3, dx[real] + 3]
    return wp


def unpack_nat(t):
    """[64, 256] (natural channel rows) -> [64, 3, 7, 7]: the real taps, pseudo-taps dropped."""
    dy, dx, c = k_offsets()
    real = real_taps()
    out = torch.zeros(CO, 3, 7, 7, dtype=t.dtype)
    out[:, c[real], dy[real] + 3, dx[real] + 3] = t[:, real]
    return out


def to_x4(x, ch3=None):
    """NCHW [n, 3, 224, 224] -> NHWC4 bf16 with channel 3 zero (or ``ch3 [n, 224, 224]``)."""
    n = x.shape[0]
    x4 = torch.zeros(n, IH, IW, 4, dtype=torch.bfloat16)
    x4[..., :3] = x.permute(0, 2, 3, 1)
    if ch3 is not None:
        x4[..., 3] = ch3
    return x4


# ------------------------------------------------------------------------------- stem forward

FWD_FAMILIES = ("uniform", "cancel", "ternary", "gather")
# (n, max_blocks): every family runs the first three, uniform and ternary all six
FWD_CASES = [(1, 0), (1, 1), (1, 4), (2, 3), (2, 5), (3, 0)]


def fwd_inputs(family, n, launch=0):
    """bf16 image ``[n, 3, 224, 224]`` and filter ``[64, 3, 7, 7]``. gather: launch j puts a single 1.0 at flat
    (ci, ky, kx) tap 64 j + co of channel co (none when that is 147 or more); x holds bit patterns."""
    g = E._gen("stemfwd", family, n)
    if family == "uniform":
        x, w = E._uni(g, n, 3, IH, IW), E._uni(g, CO, 3, 7, 7) * 147 ** -0.5
    elif family == "cancel":  # channels 0 / 1 cancel under equal weights; the odd third channel is zero on both sides
        u = E._uni(g, n, IH, IW)
        x = torch.zeros(n, 3, IH, IW)
        x[:, 0], x[:, 1] = u, -u * (1 + 2.0 ** -6 * torch.rand(u.shape, generator=g))
        w = torch.zeros(CO, 3, 7, 7)
        w[:, 0] = w[:, 1] = E._uni(g, CO, 7, 7) * 147 ** -0.5
    elif family == "ternary":
        x = (torch.randint(0, 3, (n, 3, IH, IW), generator=g) - 1).float()
        w = E._sparse_ternary(g, CO, 147, NNZ).view(CO, 3, 7, 7)
    elif family == "gather":
        x = E.patterns(n, 3, IH, IW).float()
        w = torch.zeros(CO, 147)
        t = 64 * launch + torch.arange(CO)
        w[torch.arange(CO)[t < 147], t[t < 147]] = 1.0
        w = w.view(CO, 3, 7, 7)
    else:
        raise ValueError(family)
    return x.bfloat16(), w.bfloat16()


def fwd_reference(x4, w):
    """(R, A) = (A W'^T, |A| |W'|^T) in float64, ``[n * 12544, 64]`` with natural channel columns."""
    a, wn = im2col(x4), pack_nat(w)
    return a @ wn.t(), a.abs() @ wn.abs().t()


def fwd_grid(n, max_blocks, resident):
    """(workgroups launched, row groups per workgroup) of the forward launcher."""
    groups = n * (OH // 8)
    blocks = min(groups, min(max_blocks, resident) if max_blocks > 0 else resident)
    per = ceil_div(groups, blocks)
    return ceil_div(groups, per), per


def fwd_check(tag, family, y, shards, r, a, errs):
    """y [rows, 64] and the statistics shards [64, 2, 64]: |y - R| <= u |R| + 256 2^-23 A; the shards against
    float64 sums of the stored y (rows 2^-23 sum |y|, likewise y^2); ternary and gather EQUAL."""
    E.check_out(tag, family, y, r, a, KK, "bf16", errs)
    if family != "gather" and shards is not None:
        E.check_colsums(tag, family, shards, y, errs)


def fwd_emulate(x4, w, max_blocks=0, resident=256, **defect):
    """The forward in float32, sequentially over the 256 k; statistics per workgroup pixel by pixel, then into
    shard ``block % 64`` (the least favourable order of the kernel's geometry)."""
    n = x4.shape[0]
    a, wn = im2col(x4, torch.float32, **defect), pack_nat(w, torch.float32)
    acc = torch.zeros(n * PIX, CO)
    for k in range(KK):
        acc += a[:, k:k + 1] * wn[:, k]
    y = E.rn_bf16(acc)
    blocks, per = fwd_grid(n, max_blocks, resident)
    yf = y.float().view(n * (OH // 8), 8 * OW, CO)
    shards = torch.zeros(64, 2, CO)
    for b in range(blocks):
        s, q = torch.zeros(CO), torch.zeros(CO)
        for row in yf[b * per:(b + 1) * per].reshape(-1, CO):
            s += row
            q += row * row
        shards[b % 64, 0] += s
        shards[b % 64, 1] += q
    return y, shards


# ------------------------------------------------------------------------------- stem backward

BWD_FAMILIES = ("uniform", "integer", "overlap", "blocked", "gather")
BWD_EXACT = ("integer", "overlap")


def bwd_grids(blocks3):
    """(n, blocks); ``blocks3`` = stem_bwd_blocks(3). integer and uniform run all, the rest the first two."""
    return [(1, 1), (1, 5), (1, 56), (1, 40), (2, 3), (3, blocks3)]


def gather_pixels():
    """The 64 conv pixels (oy, ox) of the backward gather family: the four corners, the four edge mid-points,
    pooled column 55 with an odd conv column (ox = 111: one window only; ox = 109: its second window is
    column 55), pooled row 55 (oy = 109 .. 111), both rows and both column parities of several row pairs."""
    px = [(0, 0), (0, 111), (111, 0), (111, 111), (0, 56), (56, 0), (111, 56), (56, 111),
          (55, 111), (1, 111), (110, 111), (2, 109), (3, 109), (109, 109), (109, 3), (110, 4), (111, 5),
          (2, 10), (3, 10), (2, 11), (3, 11), (54, 54), (55, 55), (54, 55), (55, 54), (1, 0), (0, 1), (1, 1),
          (110, 0), (111, 1), (109, 110), (108, 111)]
    i = 0
    while len(px) < CO:
        p = ((7 * i + 3) % OH, (11 * i + 5) % OW)
        if p not in px:
            px.append(p)
        i += 1
    return px


def small_patterns(*shape):
    """4096 distinct bf16 bit patterns (both signs, exponents 2^-7 .. 2^8, every significand), scrambled as
    ``mfma_edges.patterns``: the backward also sums the im2col operand over all pixels (G3, and G2 against c),
    which the full exponent range would overflow in fp32."""
    i = (torch.arange(math.prod(shape), dtype=torch.int64) * 2473 + 12345) % 4096
    r = i // 2
    bits = ((i % 2) << 15) | ((120 + r // 128) << 7) | (r % 128)
    bits = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16)
    return bits.view(torch.bfloat16).reshape(shape)


def _window_of(o, alt):
    """A pooled window coordinate and position (p, k) covering conv coordinate o: 2 p - 1 + k = o. An odd o has
    two (k = 2 of p = (o - 1) / 2, or k = 0 of the next window where that exists): ``alt`` picks."""
    if o % 2 == 0:
        return o // 2, 1
    if alt and (o + 1) // 2 < PH:
        return (o + 1) // 2, 0
    return (o - 1) // 2, 2


def bwd_inputs(family, n, true_stats=None):
    """x4 [n, 224, 224, 4], c [n, 112, 112, 64], dp [n, 56, 56, 64] (bf16), idx (uint8), mean, inv, w (fp32).
    |dp| in [2^-4, 1] or small integers, so a gather sum of at most four terms is exact in fp32. Positions
    outside the image (ky = 0 of pooled row 0, kx = 0 of pooled column 0) are never generated. uniform takes
    the true batch statistics of c at n = 1 (the terms of dC then cancel) and arbitrary ones otherwise."""
    g = E._gen("stembwd", family, n)
    true_stats = (n == 1) if true_stats is None else true_stats
    ints = family in BWD_EXACT
    if ints:
        x4 = torch.randint(-2, 3, (n, IH, IW, 4), generator=g).float()
        c = torch.randint(-2, 3, (n, OH, OW, CO), generator=g).float()
        dp = torch.randint(-2, 3, (n, PH, PW, CO), generator=g).float()
        mean, inv, w = torch.zeros(CO), torch.ones(CO), torch.ones(CO)
    else:
        x4 = small_patterns(n, IH, IW, 4).float() if family == "gather" else E._uni(g, n, IH, IW, 4)
        c = (E._uni(g, n, OH, OW, CO) * 2 + E._uni(g, CO)).bfloat16().float()
        sign = torch.randint(0, 2, (n, PH, PW, CO), generator=g) * 2.0 - 1
        dp = sign * (2.0 ** -4 + torch.rand(n, PH, PW, CO, generator=g) * (1 - 2.0 ** -4))
        mean, inv = E._uni(g, CO) * 0.5, 0.5 + torch.rand(CO, generator=g)
        w = (0.5 + torch.rand(CO, generator=g)) * (torch.randint(0, 2, (CO,), generator=g) * 2.0 - 1)
        if true_stats and family == "uniform":
            cd = c.double().view(-1, CO)
            mean = cd.mean(0).float()
            inv = (1 / torch.sqrt(cd.var(0, unbiased=False) + BN_EPS)).float()
    if family in ("uniform", "integer"):
        idx = torch.randint(0, 10, (n, PH, PW, CO), generator=g)
        idx = torch.where(idx == 9, torch.full_like(idx, 255), idx)
        idx[:, 0] = torch.where(idx[:, 0] < 3, torch.full_like(idx[:, 0], 255), idx[:, 0])
        idx[:, :, 0] = torch.where((idx[:, :, 0] % 3 == 0) & (idx[:, :, 0] < 9), torch.full_like(idx[:, :, 0], 255),
                                   idx[:, :, 0])
    elif family == "overlap":
        py, px = torch.arange(PH).view(PH, 1), torch.arange(PW).view(1, PW)
        idx = torch.tensor([8, 6, 2, 0])[(py & 1) * 2 + (px & 1)].view(1, PH, PW, 1).expand(n, PH, PW, CO).clone()
    elif family == "blocked":
        idx = torch.full((n, PH, PW, CO), 255)
    elif family == "gather":
        idx = torch.full((n, PH, PW, CO), 255)
        dp = torch.zeros(n, PH, PW, CO)
        for ch, (oy, ox) in enumerate(gather_pixels()):
            (py, ky), (px, kx) = _window_of(oy, ch & 1), _window_of(ox, (ch >> 1) & 1)
            idx[ch % n, py, px, ch] = ky * 3 + kx
            dp[ch % n, py, px, ch] = 1.0
    else:
        raise ValueError(family)
    return dict(n=n, x4=x4.bfloat16(), c=c.bfloat16(), dp=dp.bfloat16(), idx=idx.to(torch.uint8), mean=mean, inv=inv,
                w=w)


def scatter_dz(dp, idx, dtype=torch.float64):
    """dz [n, 112, 112, 64]: every pooled window adds its gradient at the conv pixel its index names
    (2 py - 1 + ky, 2 px - 1 + kx); 0xFF, and a position outside the image, add nothing. One ``index_add_``."""
    n = dp.shape[0]
    k = idx.long()
    ky, kx = k // 3, k % 3
    nn = torch.arange(n).view(n, 1, 1, 1)
    oy = 2 * torch.arange(PH).view(1, PH, 1, 1) - 1 + ky
    ox = 2 * torch.arange(PW).view(1, 1, PW, 1) - 1 + kx
    ok = (k < 9) & (oy >= 0) & (oy < OH) & (ox >= 0) & (ox < OW)
    flat = ((nn * OH + oy) * OW + ox) * CO + torch.arange(CO).view(1, 1, 1, CO)
    dz = torch.zeros(n * PIX * CO, dtype=dtype)
    dz.index_add_(0, flat[ok], dp.to(dtype)[ok])
    return dz.view(n, OH, OW, CO)


def gather_dz(dp, idx, dtype=torch.float32, drop_kx0=None):
    """The same sum the way the kernel walks it: per window position, shifted strided slices. ``drop_kx0``
    plants the loss of the second window column (the kx = 0 visits): "55" at pooled column 55 only, "all"."""
    n = dp.shape[0]
    dz = torch.zeros(n, OH, OW, CO, dtype=dtype)
    for k in range(9):
        ky, kx = divmod(k, 3)
        v = torch.where(idx == k, dp.to(dtype), torch.zeros((), dtype=dtype))
        if kx == 0 and drop_kx0 == "all":
            continue
        if kx == 0 and drop_kx0 == "55":
            v[:, :, 55] = 0
        py0, px0 = int(ky == 0), int(kx == 0)
        dz[:, 2 * py0 - 1 + ky::2, 2 * px0 - 1 + kx::2][:, :PH - py0, :PW - px0] += v[:, py0:, px0:]
    return dz


def bwd_reference(inp):
    """Everything the backward checks need, in float64 on the bf16 / fp32 operands."""
    n = inp["n"]
    pix = n * PIX
    dz = scatter_dz(inp["dp"], inp["idx"]).view(pix, CO)
    dz32 = scatter_dz(inp["dp"], inp["idx"], torch.float32).view(pix, CO)
    assert torch.equal(dz32.double(), dz), "the fp32 gather sum is not exact for these dp"
    dzb = E.rn_bf16(dz).double()
    a = im2col(inp["x4"])
    c = inp["c"].double().view(pix, CO)
    m, iv = inp["mean"].double(), inp["inv"].double()
    xhat = c * iv - m * iv
    r = dict(n=n, pix=pix, dz=dz, dzb=dzb, arow=a,
             G1=a.t() @ dzb, G2=a.t() @ c, G3=a.sum(0),
             A1=a.abs().t() @ dzb.abs(), A2=a.abs().t() @ c.abs(), A3=a.abs().sum(0),
             sdz=dz.sum(0), sdzx=(dz * xhat).sum(0), mag_dz=dz.abs().sum(0), mag_dzxh=(dz * xhat).abs().sum(0),
             mag_x=(dz.abs() * ((c * iv).abs() + (m * iv).abs())).sum(0))
    return r


def coefficients(w, mean, inv, sdzx, sdz, pix):
    """sc, cb, cd of stem_wgrad_combine_kernel in float64, and ``cdm`` >= |cd| in term magnitudes
    (|sc| (|m iv k3| + |k2|): the two terms of cd cancel when the statistics are the batch's own)."""
    iv, m = inv.double(), mean.double()
    sc = (torch.ones(CO, dtype=torch.float64) if w is None else w.double()) * iv
    k2, k3 = sdz.double() / pix, sdzx.double() / pix
    cb = -sc * iv * k3
    cd = sc * (m * iv * k3 - k2)
    cdm = sc.abs() * ((m * iv * k3).abs() + k2.abs())
    return sc, cb, cd, cdm


def split_part(p):
    """[..., PART] -> G1 [..., 256, 64], G2 [..., 256, 64], G3 [..., 256]."""
    lead = p.shape[:-1]
    return (p[..., :KK * CO].reshape(*lead, KK, CO), p[..., KK * CO:2 * KK * CO].reshape(*lead, KK, CO),
            p[..., 2 * KK * CO:])


COMBINE_UNITS = 10  # roundings on the longest path of the combine: cd (7), cd * g3 (1), two fmas (2)


def bwd_bounds(family, inp, ref):
    """The bounds of checks 1 and 2 (None: must be equal)."""
    pix = ref["pix"]
    exact = family in BWD_EXACT
    if exact:
        for k in ("A1", "A2", "A3", "mag_dz", "mag_x"):
            assert float(ref[k].max()) < 2 ** 24, f"{family}: {k} {float(ref[k].max())} not below 2^24"
    b = {}
    b["G1"] = None if exact or family in ("blocked", "gather") else E.bound(ref["G1"], ref["A1"], pix, "f32")
    b["G2"] = None if exact else E.bound(ref["G2"], ref["A2"], pix, "f32")
    b["G3"] = None if exact else E.bound(ref["G3"], ref["A3"], pix, "f32")
    b["db"] = None if exact or family in ("blocked", "gather") else pix * E23 * ref["mag_dz"] + TINY
    b["dw"] = None if exact or family == "blocked" else pix * E23 * ref["mag_dzxh"] + 2 * E23 * ref["mag_x"] + TINY
    return b


def _or_zero(b, like):
    return torch.zeros_like(like) if b is None else b


def bwd_check(tag, family, inp, ref, out, blocks, errs):
    """Checks 1 .. 4 and the NaN pre-fill parts of 6 / 7 on ``out`` = dict(part [blocks, PART], db_bn, dw_bn
    [64], dwp [64, 256]); the guard bands and the workspace are the caller's."""
    pix = ref["pix"]
    bnd = bwd_bounds(family, inp, ref)
    part = out["part"].double()
    if not bool(torch.isfinite(part).all()):
        errs.append(f"{tag} part: {int((~torch.isfinite(part)).sum())} non-finite of {part.numel()} "
                    f"(blocks {sorted(set(torch.nonzero(~torch.isfinite(part))[:, 0].tolist()))[:8]})")
        return
    g1, g2, g3 = split_part(part.sum(0))
    for name, got in (("G1", g1), ("G2", g2), ("G3", g3)):                                   # check 1
        E.check(f"{tag} part {name}", got, ref[name], bnd[name], errs)
    E.check(f"{tag} bnsum db_bn", out["db_bn"], ref["sdz"], bnd["db"], errs)                      # check 2
    E.check(f"{tag} bnsum dw_bn", out["dw_bn"], ref["sdzx"], bnd["dw"], errs)
    # check 3: the combine against float64 on the kernel's OWN part / dw_bn / db_bn
    sc, cb, cd, cdm = coefficients(inp["w"], inp["mean"], inp["inv"], out["dw_bn"], out["db_bn"], pix)
    p1, p2, p3 = split_part(part.abs().sum(0))
    own = sc * g1 + cb * g2 + cd * g3.view(KK, 1)
    mag = sc.abs() * g1.abs() + cb.abs() * g2.abs() + cdm * g3.abs().view(KK, 1)
    magb = sc.abs() * p1 + cb.abs() * p2 + cdm * p3.view(KK, 1)
    E.check(f"{tag} combine", out["dwp"].double().t(), own, COMBINE_UNITS * E23 * mag + blocks * E23 * magb + TINY, errs)
    # check 4: the real taps against the filter gradient of the float64 dC = sc (dz - xhat k3 - k2)
    sc, cb, cd, cdm = coefficients(inp["w"], inp["mean"], inp["inv"], ref["sdzx"], ref["sdz"], pix)
    iv, m = inp["inv"].double(), inp["mean"].double()
    dk3, dk2 = _or_zero(bnd["dw"], sc) / pix, _or_zero(bnd["db"], sc) / pix
    G1, G2, G3 = ref["G1"], ref["G2"], ref["G3"].view(KK, 1)
    A1, A2, A3 = ref["A1"], ref["A2"], ref["A3"].view(KK, 1)
    want = sc * G1 + cb * G2 + cd * G3
    b4 = (sc.abs() * _or_zero(bnd["G1"], G1) + cb.abs() * _or_zero(bnd["G2"], G2)
          + cdm * _or_zero(bnd["G3"], ref["G3"]).view(KK, 1)
          + (sc * iv).abs() * dk3 * G2.abs() + sc.abs() * ((m * iv).abs() * dk3 + dk2) * G3.abs()
          + COMBINE_UNITS * E23 * (sc.abs() * G1.abs() + cb.abs() * G2.abs() + cdm * G3.abs())
          + blocks * E23 * (sc.abs() * A1 + cb.abs() * A2 + cdm * A3) + TINY)
    E.check(f"{tag} dW", unpack_nat(out["dwp"].double()), unpack_nat(want.t().contiguous()),
            unpack_nat(b4.t().contiguous()) + TINY, errs)


def _fma(a, b, c):
    """fp32 fma: the product is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def bwd_emulate(inp, blocks, defect=None):
    """The backward in float32 with the kernel's formulas and geometry: ``blocks`` workgroups of
    ceil(56 n / blocks) row pairs, each row pair as 7 k-steps of 32 pixels accumulated one after the other,
    BN sums row pair by row pair, block partials summed in block order, then the combine. Defects: see
    ``BWD_DEFECTS``."""
    n = inp["n"]
    total, pix = n * PH, n * PIX
    per = ceil_div(total, blocks)
    a = im2col(inp["x4"], torch.float32, odd_row_shift=1 if defect == "rowoff" else 0).view(total, 2 * OW, KK)
    dz = gather_dz(inp["dp"], inp["idx"], drop_kx0={"drop_w55": "55", "drop_w_all": "all"}.get(defect))
    dz = dz.view(total, 2 * OW, CO)
    dzb = E.rn_bf16(dz).float()
    c = inp["c"].float().view(total, 2 * OW, CO)
    mean, inv = inp["mean"], inp["inv"]
    xhat = _fma(c, inv, -mean * inv)
    part = torch.full((blocks, PART), float("nan"))
    s1, s2 = torch.zeros(blocks, CO), torch.zeros(blocks, CO)
    for b in range(blocks):
        its = range(b * per, min(total, (b + 1) * per))
        if defect == "idle_unwritten" and len(its) == 0:
            continue
        g1, g2, g3 = torch.zeros(KK, CO), torch.zeros(KK, CO), torch.zeros(KK)
        for it in its:
            ai = a[it - 1] if defect == "stale_stage" and it == b * per + 1 else a[it]
            for ks in range(7):
                sl = slice(32 * ks, 32 * ks + 32)
                g1 += ai[sl].t() @ dzb[it, sl]
                g2 += ai[sl].t() @ c[it, sl]
                if defect != "g3_half" or ks % 2 == 0:
                    g3 += ai[sl].sum(0)
            s1[b] += dz[it].sum(0)
            s2[b] += (dz[it].double() * xhat[it].double()).float().sum(0)
        part[b] = torch.cat([g1.reshape(-1), g2.reshape(-1), g3])
    db, dw = torch.zeros(CO), torch.zeros(CO)
    t1, t2, t3 = torch.zeros(KK, CO), torch.zeros(KK, CO), torch.zeros(KK)
    for b in range(blocks):
        db += s1[b]
        dw += s2[b]
        p1, p2, p3 = split_part(part[b])
        t1, t2, t3 = t1 + p1, t2 + p2, t3 + p3
    w = torch.ones(CO) if inp["w"] is None else inp["w"]
    inv_n = torch.tensor(1.0) / torch.tensor(float(pix))
    sc = w * inv
    k2, k3 = db * inv_n, dw * inv_n
    cb = -sc * inv * k3
    cd = sc * (mean * inv * k3 - k2)
    if defect == "cd_sign":
        cd = -cd
    dwp = _fma(sc, t1, _fma(cb, t2, cd * t3.view(KK, 1))).t().contiguous()
    return dict(part=part, db_bn=db, dw_bn=dw, dwp=dwp)


BWD_DEFECTS = ("drop_w55", "drop_w_all", "stale_stage", "rowoff", "g3_half", "idle_unwritten", "cd_sign")


# ------------------------------------------------------------------------------- conv_c3.hip

# (N, H, W, stride, Cout)
C3_SHAPES = [(1, 1, 1, 1, 128), (1, 2, 2, 2, 128), (3, 7, 9, 1, 256), (1, 16, 16, 1, 128), (1, 1, 257, 1, 128),
             (1, 257, 1, 1, 128), (2, 16, 16, 1, 128), (1, 19, 27, 1, 128), (5, 17, 13, 2, 384), (2, 8, 6, 2, 128)]
C3_FWD_PX, C3_WG_PX = 256, 512


def c3_out(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def c3_fwd_inputs(family, n, h, w, stride, co):
    """bf16 image [n, 3, h, w] and filter [co, 3, 3, 3] (OIHW values). gather: channel co holds a 1.0 at flat
    (kh, kw, ci) tap co mod 27 and x holds bit patterns."""
    if family != "gather":
        return E.conv_inputs(family, n, 3, h, w, co, nnz=27)
    f = torch.zeros(co, 27)
    f[torch.arange(co), torch.arange(co) % 27] = 1.0
    return E.patterns(n, 3, h, w), f.view(co, 3, 3, 3).permute(0, 3, 1, 2).contiguous().bfloat16()


def c3_gather_pixels(pixels):
    """Both ends of the pixel range, both sides of every 256 / 512 boundary, the (unpaired, when the count is odd)
    last pixel and its neighbour."""
    cand = [0, 1, pixels - 2, pixels - 1]
    for b in range(C3_FWD_PX, pixels + 1, C3_FWD_PX):
        cand += [b - 1, b]
    return sorted({p for p in cand if 0 <= p < pixels})


def c3_wgrad_inputs(family, n, h, w, stride, co):
    """bf16 image [n, 3, h, w] and output gradient [n, co, ho, wo]; the reduction runs over the pixels, so the
    family's structure lies along them: cancel pairs adjacent pixels of opposite dy over an image that is nearly
    constant along its rows; ternary has at most 256 non-zero pixels per channel (|dW| <= 256: exact in bf16
    too); gather is one-hot per channel at ``c3_gather_pixels``."""
    ho, wo = c3_out(h, w, stride)
    px = n * ho * wo
    g = E._gen("c3wg", family, n, h, w, stride, co)
    if family == "uniform":
        dyt, x = E._uni(g, co, px), E._uni(g, n, 3, h, w)
    elif family == "cancel":
        dyt = E.gemm_inputs("cancel", co, 1, px, seed=h)[0].float()
        x = E._uni(g, n, 3, h, 1).expand(n, 3, h, w) + 2.0 ** -6 * E._uni(g, n, 3, h, w)
    elif family == "ternary":
        dyt = E._sparse_ternary(g, co, px, 256)
        x = (torch.randint(0, 3, (n, 3, h, w), generator=g) - 1).float()
    elif family == "gather":
        sel = torch.tensor(c3_gather_pixels(px))
        dyt = torch.zeros(co, px)
        dyt[torch.arange(co), sel[torch.arange(co) % len(sel)]] = 1.0
        x = E.patterns(n, 3, h, w).float()
    else:
        raise ValueError(family)
    dy = dyt.t().reshape(n, ho, wo, co).permute(0, 3, 1, 2)
    return x.bfloat16().contiguous(), dy.bfloat16().contiguous()


def c3_rows(y):
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def c3_fwd_reference(x, wt, stride):
    """(P, Q, R, A): windows [pixels, 27] and filter [co, 27] in (kh, kw, ci) order, R = P Q^T, A = |P| |Q|^T."""
    p, q = E.im2col(x, stride), E.taps(wt)
    return (p, q) + E.ref_gemm(p, q)


def c3_wgrad_reference(x, dy, stride):
    """(R, A) [co, 27] of dW = dy^T im2col(x)."""
    return E.ref_gemm(c3_rows(dy).t(), E.im2col(x, stride).t())


def c3_fwd_emulate(x, wt, stride, defect=None):
    """float32, sequentially over the 27 taps. Defect ``pair13``: the high half of k-pair 13 is not zero but
    repeats k = 26 (image and filter side), so that tap counts twice."""
    p, q = E.im2col(x.float(), stride), E.taps(wt.float())
    acc = torch.zeros(p.shape[0], q.shape[0])
    for k in list(range(27)) + ([26] if defect == "pair13" else []):
        acc += p[:, k:k + 1] * q[:, k]
    return E.rn_bf16(acc)


def c3_wgrad_emulate(x, dy, stride, defect=None):
    """float32 partials [blocks, co, 27]: 512 pixels per block, pixel after pixel. Defect ``last_twice``: the
    partner slot of an unpaired last pixel repeats that pixel instead of holding zeros."""
    p, d = E.im2col(x.float(), stride), c3_rows(dy.float())
    px = p.shape[0]
    blocks = ceil_div(px, C3_WG_PX)
    part = torch.zeros(blocks, d.shape[1], 27)
    for i in range(px):
        part[i // C3_WG_PX] += d[i].view(-1, 1) * p[i].view(1, -1)
    if defect == "last_twice" and px % 2 == 1:
        part[(px - 1) // C3_WG_PX] += d[px - 1].view(-1, 1) * p[px - 1].view(1, -1)
    return part


def c3_check_wgrad(tag, family, got, r, a, pixels, errs, bf16_store=False):
    """fp32 (sum of partials): pixels 2^-23 A + 2^-24 |R|; through the wrapper's bf16 store one more u |R|."""
    if family in E.EXACT:
        E.check(tag, got, r, None, errs)
    else:
        E.check(tag, got, r, E.bound(r, a, pixels, "f32") + (E.U8 * r.abs() if bf16_store else 0), errs)
