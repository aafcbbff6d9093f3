"""Inputs, float64 references, derived bounds, a float32 emulation and planted defects for the fused DEQ
cell kernels of ``csrc/kernels/deq_cell.hip`` (``deq_cell_fwd_kernel``, ``deq_cell_vjp_kernel``), shared by
``test_deq_cell_edges_gpu.py`` (plain helper module: no fixtures, no tests). The checker, the convolution
reference (``im2col`` / ``taps`` / ``taps_t`` / ``ref_gemm`` / ``bound``), the input families and the guard
bands are those of ``mfma_edges``; the GroupNorm references and bounds are those of ``norm_edges`` at the
cell's reduction length. Nothing is fitted to kernel output.

Layout: every activation is "rows", [N, H W, 48] (the kernels' NHWC sample-major order); a filter is its
[48, 432] matrix, k = tap * 48 + channel (``taps(W)`` forward, ``taps_t(W)`` for the input gradients).

    f(z, x) = GN3(h3),  h3 = relu(z + GN2(h2)),  h2 = conv2(GN1(h1)) + x,  h1 = relu(conv1 z)

Constants: u = 2^-24 (fp32 unit roundoff), u_b = 2^-8 (bf16), E = 2^-23 per fp32 addition (``mfma_edges``),
Kred = 432. An fma is charged as two roundings, so no bound depends on contraction.

Reduction length. Per channel a lane adds its (at most) 7 pixels, ``row_sum16`` has 4 levels, one thread adds
the 8 waves' partials: L_px = 7 + 4 + 8 = 19; a group adds its cpg channels: L_gn = 19 + cpg (``cell_L``).

LDS (``lds_bytes``, the documented formula): (H + 2) ((W + 2) 48 + 32) 2 + 48 * 464 * 2 + 4 (768 + 96 + 144)
bytes, refused above 160 KB.

Forward, stage by stage FROM THE KERNEL'S OWN STORED STATE (h1, h2, h3 and the three mean / rstd pairs), so
that no stage's error is charged to the next (``check_fwd``):

    h1      R1 = im2col(z) taps(W1)^T, A1 = |im2col(z)| |taps(W1)|^T:
            |h1 - relu(R1)| <= u_b |R1| + 432 E A1   (= bound(R1, A1, 432, "bf16"); ReLU is 1-Lipschitz and
            commutes with the rounding). ternary, gather and chain: h1 EQUALS relu(R1).
    stats   mean_k / rstd_k against the float64 statistics of the stored h_k: ``norm_edges``' single-pass
            dmean / dinv at L = L_gn (``gn_refs(..., L=cell_L(G))``).
    h2      GN1's output a1 is not stored. a1* = h1 sc + sh in float64 from the stored h1, mean1, rstd1 and the
            affine (sc = rstd w, sh = b - mean sc). The kernel's a1 = bf16(fl(h1 sc + sh)) with sc, mean sc, the
            subtraction and the fma (two) rounded:
                da1 = u_b |a1*| + 4u (|h1 sc| + |mean sc| + |b|)
            R2 = im2col(a1*) taps(W2)^T, A2 likewise with absolute values. The kernel rounds the accumulator to
            bf16, adds x in fp32 and rounds to bf16:
                |h2 - (R2 + x)| <= u_b |R2| + u_b |R2 + x| + u |R2 + x| + 432 E A2 + im2col(da1) |taps(W2)|^T
            The last, propagated, term is the largest by far (432 products of u_b |a1| |w|, added in absolute
            value where the true errors are signed): a ratio far below 1 is expected at this stage.
    chain   the exact chain: W1 a gather filter, z signed powers of two {+-1, +-2, +-4}, GN1's bias 0. Then h1
            is in {0, 1, 2, 4}, h1 sc is exact and sh = -fl(mean sc) however the compiler contracts, so
            a1 = bf16(fl32(h1 sc + sh)) is reproduced bit for bit in float32 on the CPU from the stored
            mean1 / rstd1. W2 a gather filter: h2 EQUALS bf16(fl32(a1[selected] + x)).
    h3      a2* and da2 as a1* and da1 from the stored h2, mean2, rstd2:
                |h3 - relu(z + a2*)| <= da2 + u |z + a2*| + u_b |relu(z + a2*)|
    out     ``gn_refs``' output bound on the stored h3 (dz + u_b |y| of ``norm_edges``).
    gather  at stage 1 only: the bit patterns reach 3e38, whose squares overflow fp32, so the later stages of
            that launch are not finite by construction; their guard bands are still checked.

VJP (``vjp_refs``). The state is an INPUT (h_k, mean_k, rstd_k, w_k supplied by the test); the intermediates
d3, d2, da1, d1 are not observable, so the bound is composed by absolute-value propagation. Every stage is
linear in its incoming gradient: if the incoming gradient is within B_in of the reference's, the stage's output
is within M(B_in) + (the stage's own bound at the reference input), M the stage's absolute-value map:

    GroupNorm backward  dh = rstd (dy w - m1 - xhat m2), m1 = sum_c w S_c / M, m2 = sum_c w rstd (Q_c - mean S_c) / M:
        M(d) = |rstd w| d + rstd (sum_c |w| sum_p d / M + |xhat| rstd sum_c |w| sum_p d |h - mean| / M), times
        the ReLU mask (``gn_abs``); own bound ``gn_bwd_refs``' ddh + u_b |dh| at L_px = 19
    convolution         M(d) = im2col(d) |taps_t(W)|^T (``conv_abs``); own bound bound(R, A, 432, "bf16"), and
                        "res" (u_b |R| + u_b |R + d3| + 432 E A) for the last one, which adds the parked d3
                        (whose own bound B3 is added too)

    B3 = own3(u);  B2 = M2(B3) + own2(d3*);  Ba = Mc2(B2) + own(conv2^T);  B1 = M1(Ba) + own1(da1*);
    Bout = Mc1(B1) + B3 + own_res(conv1^T)

No fitted constant. The propagated terms dominate at the convolution stages (ratios far below 1 expected).

The exact VJP case (``vjp_exact_inputs``; needs H, W >= 3): u ternary, at most 1/16 dense, zero on the
one-pixel border ring, interior pixels paired in raster order with u(p') = -u(p); h3 and h2 arbitrary bf16
values of magnitude >= 2^-6 (so that the fp32 sums of dy h are exact in any order), equal within each pair
(mixed signs on h3: the ReLU mask is equal within a pair); h1 constant per channel, most channels positive, a
few <= 0 (a whole channel masked); rstd in {1, 2}, mean a multiple of 1/4, affine weights +-1; W2^T dense
ternary; W1^T with 4 non-zeros per row at seeded positions. Then every per-channel sum dy and sum dy h is an
exact zero at all three GroupNorm backwards (the border ring keeps the shifted sums after conv2^T zero), so
d = A dy exactly, every partial sum is an integer below 2^24 and every rounded intermediate is bf16-exact:
``vjp_exact_asserts`` checks exactly that (the float64 chain is unchanged by rounding to bf16 at each of the
kernel's five rounding points, and at the sixth with ``grad``). The kernel's output must EQUAL the chain;
with an integer ``grad`` u_new EQUALS the reference and ss_part[n] the integer sum (u_new - u)^2.

Float32 emulation (``emulate_fwd`` / ``emulate_vjp``): the kernels' formulas in float32 PyTorch (no fma),
rounded to bf16 where the kernels round, the GroupNorm sums in the kernels' order (``cell_sums``: 7 per lane,
the 16-lane tree, 8 waves, then cpg channels). Planted defects (``defect=``): "ktail" (k = 416 .. 431 dropped
in one 16 x 16 fragment), "shifted_tap" (tap (1, 2) reads past the right border), "lost_block" (the 49th pixel
block computed by no wave), "neighbour_group" (a lane's 4 channels take the first one's group at cpg = 3),
"h3_for_stage2" (the VJP's second GroupNorm backward reads h3), "truncation" (instead of round to nearest).
"""
import torch

from . import mfma_edges as E
from . import norm_edges as NE
from .mfma_edges import E23, TINY, U8
from .norm_edges import U32, seqsum

C = 48
KRED = 9 * C
BF = torch.bfloat16
GROUPS = (1, 2, 3, 4, 6, 8, 12, 16)
L_PX = 19
LDS_LIMIT = 160 * 1024
EXACT_FWD = ("ternary", "gather", "chain")


def cell_L(G):
    return L_PX + C // G


def lds_bytes(H, W):
    return (H + 2) * ((W + 2) * 48 + 32) * 2 + 48 * 464 * 2 + 4 * (768 + 96 + 144)


def supported_ref(H, W, ch, G):
    """The documented acceptance rule of the launcher."""
    return (ch == C and G in GROUPS and (H * W) % 16 == 0 and 1 <= H * W // 16 <= 56
            and lds_bytes(H, W) <= LDS_LIMIT)


# ------------------------------------------------------------------------------- layout

def rows(x):
    """[n, c, h, w] -> [n, h w, c]."""
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1]).contiguous()


def image(r, H, W):
    """[n, h w, c] -> [n, c, h, w]."""
    return r.reshape(r.shape[0], H, W, r.shape[2]).permute(0, 3, 1, 2)


def conv_ref(r, tm, H, W, dtype=torch.float64):
    """(R, A) [N, HW, C] of the 3x3 convolution of rows ``r`` with the filter matrix ``tm`` [C, 432]."""
    R, A = E.ref_gemm(E.im2col(image(r.to(dtype), H, W)), tm, dtype)
    return R.view(r.shape[0], H * W, -1), A.view(r.shape[0], H * W, -1)


def conv_abs(d, tm, H, W):
    """The convolution's absolute-value map of a bound ``d`` [N, HW, C]."""
    return (E.im2col(image(d, H, W)) @ tm.double().abs().t()).view(d.shape[0], H * W, -1)


def _ex(t, G):
    """[N, G] -> [N, C] float64."""
    return t.double().repeat_interleave(C // G, 1)


# ------------------------------------------------------------------------------- inputs

def _affine3(g, null=False):
    if null:
        return [None] * 3, [None] * 3
    wb = [NE.affine(g, C) for _ in range(3)]
    return [w for w, _ in wb], [b for _, b in wb]


def fwd_inputs(family, N, H, W, seed=0, ratio=0, null_affine=False):
    """z, x rows (bf16), the 4-D filters w1, w2 and their matrices t1, t2, the affine gw / gb [3] (fp32 or
    None). families: the four of ``mfma_edges`` (``conv_inputs`` per convolution), "chain" and "offset"
    (uniform, x shifted by ``ratio`` standard deviations: GN2's E[h^2] - mean^2 cancellation)."""
    fam = {"chain": "gather", "offset": "uniform"}.get(family, family)
    zi, w1 = E.conv_inputs(fam, N, C, H, W, C, seed=seed)
    _, w2 = E.conv_inputs(fam, N, C, H, W, C, seed=seed + 1)
    g = E._gen("deq_cell", family, N, H, W, seed, ratio)
    x = NE._uni(g, (N, H * W, C), -2, 2)
    gw, gb = _affine3(g, null_affine)
    z = rows(zi)
    if family == "chain":
        z = (NE._sign(g, z.shape) * 2.0 ** torch.randint(0, 3, z.shape, generator=g)).to(BF)
        if not null_affine:
            gb[0] = torch.zeros(C)
    elif family == "offset":
        x = x + ratio * NE.X_STD
    return dict(family=family, H=H, W=W, z=z, x=x.to(BF), w1=w1, w2=w2, t1=E.taps(w1).contiguous(),
                t2=E.taps(w2).contiguous(), gw=gw, gb=gb)


def vjp_inputs(family, N, H, W, G, seed=0, ratio=0, filt="conv"):
    """A supplied state (h_k bf16 rows, mean_k / rstd_k the fp32-rounded statistics of h_k, affine weights),
    u and the transposed filter matrices. families: uniform, cancel (on u and the filters, ``conv_inputs``
    with dgrad), offset (uniform with the h_k shifted by ``ratio`` standard deviations). ``filt``: "conv",
    "zero_w1" (out = d3 exactly) or "identity" (centre taps: both convolutions exact identities)."""
    fam = "uniform" if family == "offset" else family
    ui, w2 = E.conv_inputs(fam, N, C, H, W, C, seed=seed, dgrad=True)
    _, w1 = E.conv_inputs(fam, N, C, H, W, C, seed=seed + 1, dgrad=True)
    if filt == "identity":
        w1 = torch.zeros(C, C, 3, 3)
        w1[torch.arange(C), torch.arange(C), 1, 1] = 1.0
        w1 = w2 = w1.to(BF)
    elif filt == "zero_w1":
        w1 = torch.zeros(C, C, 3, 3, dtype=BF)
    g = E._gen("deq_cell_vjp", family, N, H, W, G, seed, ratio)
    hs = []
    for k in range(3):
        h = NE._uni(g, (N, H * W, C), -2, 2)
        if family == "offset":
            h = h + ratio * NE.X_STD * (1 + (torch.arange(C) // (C // G)) % 2).float()
        hs.append(h.to(BF))
    st = state_of(hs, _affine3(g)[0], G, 1e-5)
    return dict(family=family, H=H, W=W, u=rows(ui), t2t=E.taps_t(w2).contiguous(), t1t=E.taps_t(w1).contiguous(),
                w1=w1, w2=w2, grad=None, **st)


def state_of(hs, gw, G, eps):
    """The VJP state of three stored GroupNorm inputs: their float64 statistics rounded to fp32."""
    mean, rstd = [], []
    for h in hs:
        m, var, _, _ = NE.stats_ref(NE.gn_groups(h, G), 2)
        mean.append(m.float())
        rstd.append((var + eps).rsqrt().float())
    return dict(h=list(hs), mean=mean, rstd=rstd, gw=list(gw))


def vjp_exact_inputs(N, H, W, G, seed=0, with_grad=True):
    """The exact VJP case (module docstring)."""
    assert H >= 3 and W >= 3
    g = E._gen("deq_cell_exact", N, H, W, G, seed)
    HW = H * W
    inter = torch.tensor([y * W + x for y in range(1, H - 1) for x in range(1, W - 1)])
    npair = len(inter) // 2
    pa, pb = inter[0:2 * npair:2], inter[1:2 * npair:2]
    dens = 1 / 16 if HW <= 256 else 1 / 128  # thinned at the large images: sum (u_new - u)^2 stays below 2^24
    s = (torch.randint(0, 3, (N, npair, C), generator=g) - 1).float() * (torch.rand(N, npair, C, generator=g) < dens)
    u = torch.zeros(N, HW, C)
    u[:, pa], u[:, pb] = s, -s
    hs = []
    for _ in range(2):  # h3, h2
        v = torch.randn(N, HW, C, generator=g)
        v = (v.sign() + (v == 0)) * v.abs().clamp_min(2.0 ** -6)
        v[:, pb] = v[:, pa]
        hs.append(v.to(BF))
    h1c = (1 + torch.randint(0, 3, (C,), generator=g)).float()
    h1c[5::11] = torch.tensor([0.0, -1.0, 0.0, -2.0, 0.0])[: len(h1c[5::11])]
    h1 = h1c.view(1, 1, C).expand(N, HW, C).contiguous().to(BF)
    mean = [(torch.randint(-4, 5, (N, G), generator=g).float() / 4) for _ in range(3)]
    rstd = [2.0 ** torch.randint(0, 2, (N, G), generator=g).float() for _ in range(3)]
    gw = [NE._sign(g, (C,)) for _ in range(3)]
    t2t = (torch.randint(0, 3, (C, KRED), generator=g) - 1).to(BF)
    t1t = E._sparse_ternary(g, C, KRED, 4).to(BF)
    grad = (torch.randint(-2, 3, (N, HW, C), generator=g)).to(BF) if with_grad else None
    return dict(family="exact", H=H, W=W, u=u.to(BF), t2t=t2t, t1t=t1t, grad=grad,
                h=[h1, hs[1], hs[0]], mean=mean, rstd=rstd, gw=gw)


# ------------------------------------------------------------------------------- forward reference

def affine_ref(h, mean32, rstd32, w, b, G):
    """(a*, da): the float64 GroupNorm output from the stored h and statistics, and the distance of the
    kernel's bf16 output from it."""
    hd, mu, rs = h.double(), _ex(mean32, G)[:, None], _ex(rstd32, G)[:, None]
    wd = torch.ones(C, dtype=torch.float64) if w is None else w.double()
    bd = torch.zeros(C, dtype=torch.float64) if b is None else b.double()
    sc = rs * wd
    a = hd * sc + (bd - mu * sc)
    return a, U8 * a.abs() + 4 * U32 * ((hd * sc).abs() + (mu * sc).abs() + bd.abs())


def chain_h2(inp, out, G):
    """The exact chain's h2 = bf16(fl32(a1[selected] + x)), a1 reproduced in float32 from the stored mean1 / rstd1."""
    gi = torch.arange(C) // (C // G)
    w = torch.ones(C) if inp["gw"][0] is None else inp["gw"][0].float()
    sc = out["rstd"][0].float()[:, gi] * w
    sh = -(out["mean"][0].float()[:, gi] * sc)
    a1 = (out["h"][0].float() * sc[:, None] + sh[:, None]).to(BF)
    sel, _ = conv_ref(a1, inp["t2"], inp["H"], inp["W"])
    return (sel.float() + inp["x"].float()).to(BF).double()


def check_fwd(tag, inp, out, G, eps, errs):
    """One forward's stored state and output (``out``: h [3], mean [3], rstd [3], out; CPU tensors) against
    the stage-by-stage references (module docstring)."""
    family, H, W = inp["family"], inp["H"], inp["W"]
    z, x = inp["z"].double(), inp["x"].double()
    R1, A1 = conv_ref(inp["z"], inp["t1"], H, W)
    E.check(f"{tag} h1", out["h"][0], R1.clamp_min(0), None if family in EXACT_FWD else E.bound(R1, A1, KRED, "bf16"), errs)
    if family == "gather":
        return
    L = cell_L(G)
    for k in range(3):
        r = NE.gn_refs(out["h"][k], inp["gw"][k], inp["gb"][k], G, BF, eps, L)
        E.check(f"{tag} mean{k + 1}", out["mean"][k], r["mean"], r["dmean"], errs)
        E.check(f"{tag} rstd{k + 1}", out["rstd"][k], r["rstd"], r["drstd"], errs)
    E.check(f"{tag} out", out["out"], r["y"], r["dy"], errs)
    a1, da1 = affine_ref(out["h"][0], out["mean"][0], out["rstd"][0], inp["gw"][0], inp["gb"][0], G)
    R2, A2 = conv_ref(a1, inp["t2"], H, W)
    if family == "chain":
        E.check(f"{tag} h2", out["h"][1], chain_h2(inp, out, G), None, errs)
    else:
        b2 = (U8 * R2.abs() + (U8 + U32) * (R2 + x).abs() + KRED * E23 * A2 + conv_abs(da1, inp["t2"], H, W) + TINY)
        E.check(f"{tag} h2", out["h"][1], R2 + x, b2, errs)
    a2, da2 = affine_ref(out["h"][1], out["mean"][1], out["rstd"][1], inp["gw"][1], inp["gb"][1], G)
    t = z + a2
    E.check(f"{tag} h3", out["h"][2], t.clamp_min(0), da2 + U32 * t.abs() + U8 * t.clamp_min(0) + TINY, errs)


# ------------------------------------------------------------------------------- VJP reference

def gn_abs(d, h, mean32, rstd32, w, G, relu):
    """The GroupNorm backward's absolute-value map of a bound ``d`` on its incoming gradient."""
    N, HW, _ = h.shape
    cpg = C // G
    M = HW * cpg
    hd, mu, rs = h.double(), _ex(mean32, G), _ex(rstd32, G)
    wa = torch.ones(C, dtype=torch.float64) if w is None else w.double().abs()
    grp = lambda t: t.view(N, G, cpg).sum(2).repeat_interleave(cpg, 1)
    dev = (hd - mu[:, None]).abs()
    m1 = grp(wa * d.sum(1)) / M
    m2 = grp(wa * rs * (d * dev).sum(1)) / M
    o = (rs * wa)[:, None] * d + rs[:, None] * (m1[:, None] + dev * rs[:, None] * m2[:, None])
    return o * (hd > 0) if relu else o


def vjp_refs(inp, G):
    """The float64 chain d3, d2, da1, d1, out from the supplied state, with the composed bounds B3 .. Bout
    and the per-channel sums (db, dw) of the three GroupNorm backwards."""
    H, W = inp["H"], inp["W"]
    h, mean, rstd, gw = inp["h"], inp["mean"], inp["rstd"], inp["gw"]
    gn = lambda dy, k, relu: NE.gn_bwd_refs(dy, h[k], mean[k], rstd[k], gw[k], G, relu, BF, L_PX)
    ab = lambda d, k, relu: gn_abs(d, h[k], mean[k], rstd[k], gw[k], G, relu)
    r3 = gn(inp["u"], 2, True)
    d3, B3 = r3["dh"], r3["ddh"]
    r2 = gn(d3, 1, False)
    d2, B2 = r2["dh"], ab(B3, 1, False) + r2["ddh"]
    da1, A = conv_ref(d2, inp["t2t"], H, W)
    Ba = conv_abs(B2, inp["t2t"], H, W) + E.bound(da1, A, KRED, "bf16")
    r1 = gn(da1, 0, True)
    d1, B1 = r1["dh"], ab(Ba, 0, True) + r1["ddh"]
    R, A = conv_ref(d1, inp["t1t"], H, W)
    Bout = conv_abs(B1, inp["t1t"], H, W) + B3 + E.bound(R, A, KRED, "res", d3)
    return dict(d3=d3, d2=d2, da1=da1, d1=d1, out=R + d3, B3=B3, B2=B2, Ba=Ba, B1=B1, Bout=Bout,
                sums=[(r["db"], r["dw"]) for r in (r3, r2, r1)])


def check_vjp(tag, inp, got, G, errs, ref=None):
    ref = vjp_refs(inp, G) if ref is None else ref
    E.check(f"{tag} vjp", got, ref["out"], ref["Bout"], errs)
    return ref


def vjp_exact_asserts(inp, G):
    """The exact case's structure in float64: every GroupNorm backward sum is an exact zero and every
    rounding point of the kernel holds a bf16-exact value. Returns (out or u_new, ss_part or None)."""
    ref = vjp_refs(inp, G)
    for k, (S, dw) in enumerate(ref["sums"]):
        assert float(S.abs().max()) == 0 and float(dw.abs().max()) == 0, f"GroupNorm backward {3 - k}: sums not zero"
    exact = lambda t: bool((t.to(BF).double() == t).all())
    for name in ("d3", "d2", "da1", "d1", "out"):
        assert exact(ref[name]), f"{name} is not bf16-exact (max {float(ref[name].abs().max())})"
        assert float(ref[name].abs().max()) < 2 ** 24
    assert float((ref["out"] != 0).double().mean()) > 0, "the exact case is all zero"
    if inp["grad"] is None:
        return ref["out"], None
    un = ref["out"] + inp["grad"].double()
    assert exact(un), "u_new is not bf16-exact"
    ss = ((un - inp["u"].double()) ** 2).sum((1, 2))
    assert float(ss.max()) < 2 ** 24 and bool((ss == ss.round()).all())
    return un, ss


# ------------------------------------------------------------------------------- float32 emulation

def cell_sums(t):
    """Per-channel sums [N, C] of float32 rows [N, HW, C] in the kernels' order: lane (wave w, column c) adds
    the pixels 16 (w + 8 i) + c, i = 0 .. 6, in sequence, the 16 columns go through ``row_sum16``'s tree
    (neighbours, pairs, then the rotations by 4 and 8), one thread adds the 8 waves in sequence."""
    N, HW, ch = t.shape
    pad = torch.zeros(N, 56 * 16, ch)
    pad[:, :HW] = t
    lane = seqsum(pad.view(N, 7, 8, 16, ch).permute(1, 0, 2, 3, 4))  # [N, wave, col, C]
    idx = torch.arange(16)
    for perm in (idx ^ 1, idx ^ 2, (idx + 4) % 16, (idx + 8) % 16):
        lane = lane + lane[:, :, perm]
    return seqsum(lane[:, :, 0].permute(1, 0, 2))


def _grp_seq(t, G):
    """[N, C] -> [N, G]: the group's channels added in sequence."""
    return seqsum(t.view(t.shape[0], G, C // G).permute(2, 0, 1))


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def conv32(r, tm, H, W):
    return (E.im2col(image(r.float(), H, W)) @ tm.float().t()).view(r.shape[0], H * W, -1)


def emu_gn_fwd(v, w, b, G, eps, rnd, defect=None):
    N, HW, _ = v.shape
    cpg = C // G
    vf = v.float()
    gs, gq = _grp_seq(cell_sums(vf), G), _grp_seq(cell_sums(vf * vf), G)
    inv_m = _f32(1.0) / _f32(float(HW * cpg))
    mu = gs * inv_m
    r = torch.rsqrt((gq * inv_m - mu * mu).clamp_min(0) + _f32(eps))
    c = torch.arange(C)
    gi = (c // 4 * 4) // cpg if defect == "neighbour_group" else c // cpg
    sc = r[:, gi] * (torch.ones(C) if w is None else w.float())
    sh = (torch.zeros(C) if b is None else b.float()) - mu[:, gi] * sc
    return mu, r, rnd(vf * sc[:, None] + sh[:, None])


def emulate_fwd(inp, G, eps, defect=None):
    """deq_cell_fwd_kernel in float32: dict(h [3], mean [3], rstd [3], out)."""
    H, W = inp["H"], inp["W"]
    rnd = E.trunc_bf16 if defect == "truncation" else E.rn_bf16
    z, x = inp["z"], inp["x"]
    N, HW, _ = z.shape
    c1 = conv32(z, inp["t1"], H, W)
    if defect == "shifted_tap":
        c1 = E.shifted_tap_conv(image(z, H, W), inp["w1"]).view(N, HW, C)
    elif defect == "ktail":  # channels 16 .. 31 of the first pixel block lose the last half K chunk
        p = E.im2col(image(z.float(), H, W)).view(N, HW, KRED)
        c1[:, 0:16, 16:32] -= p[:, 0:16, 416:] @ inp["t1"].float()[16:32, 416:].t()
    h1 = rnd(rnd(c1).float().clamp_min(0))
    if defect == "lost_block":
        h1[:, 768:784] = 0
    gn = lambda v, k: emu_gn_fwd(v, inp["gw"][k], inp["gb"][k], G, eps, rnd, defect)
    m1, r1, a1 = gn(h1, 0)
    h2 = rnd(rnd(conv32(a1, inp["t2"], H, W)).float() + x.float())
    m2, r2, a2 = gn(h2, 1)
    h3 = rnd((z.float() + a2.float()).clamp_min(0))
    m3, r3, out = gn(h3, 2)
    return dict(h=[h1, h2, h3], mean=[m1, m2, m3], rstd=[r1, r2, r3], out=out)


def emu_gn_bwd(dy, h, mean, rstd, w, G, relu, rnd):
    """gn_backward of deq_cell.hip: d = A dy + (C h + B), A = r w, C = -r^2 s2, B = -r s1 - C mu."""
    N, HW, _ = h.shape
    cpg = C // G
    d, hf = dy.float(), h.float()
    wv = torch.ones(C) if w is None else w.float()
    gi = torch.arange(C) // cpg
    mu, rs = mean.float()[:, gi], rstd.float()[:, gi]
    S, Q = cell_sums(d), cell_sums(d * hf)
    inv_m = _f32(1.0) / _f32(float(HW * cpg))
    s1 = (_grp_seq(wv * S, G) * inv_m)[:, gi]
    s2 = (_grp_seq(wv * rs * (Q - mu * S), G) * inv_m)[:, gi]
    A, Cc = rs * wv, -rs * rs * s2
    B = -rs * s1 - Cc * mu
    o = A[:, None] * d + (Cc[:, None] * hf + B[:, None])
    if relu:
        o = torch.where(hf > 0, o, torch.zeros_like(o))
    return rnd(o)


def emulate_vjp(inp, G, defect=None):
    """deq_cell_vjp_kernel in float32: (out or u_new, ss_part or None)."""
    H, W = inp["H"], inp["W"]
    rnd = E.trunc_bf16 if defect == "truncation" else E.rn_bf16
    h, mean, rstd, gw = inp["h"], inp["mean"], inp["rstd"], inp["gw"]
    gn = lambda dy, k, relu, hk=None: emu_gn_bwd(dy, h[k] if hk is None else hk, mean[k], rstd[k], gw[k], G, relu, rnd)
    d3 = gn(inp["u"], 2, True)
    d2 = gn(d3, 1, False, h[2] if defect == "h3_for_stage2" else None)
    da1 = rnd(conv32(d2, inp["t2t"], H, W))
    d1 = gn(da1, 0, True)
    out = rnd(conv32(d1, inp["t1t"], H, W) + d3.float())
    if inp["grad"] is None:
        return out, None
    un = rnd(out.float() + inp["grad"].float())
    dl = un.float() - inp["u"].float()
    return un, (dl * dl).sum((1, 2))
