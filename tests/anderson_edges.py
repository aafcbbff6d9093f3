"""Inputs, float64 references, derived bounds, a float32 emulation and planted defects for the Anderson solver
kernels of ``csrc/kernels/anderson.hip`` (``gram_kernel``, ``mix_kernel``, ``solve_kernel``,
``adjoint_step_kernel``), shared by ``test_anderson_edges_gpu.py`` (plain helper module: no fixtures, no
tests). The checker, ``U32``, ``U8``, ``E23``, ``TINY`` and ``seqsum`` are those of ``mfma_edges`` /
``norm_edges``. Nothing is fitted to kernel output.

Constants: u = 2^-24 (fp32 unit roundoff), u_b = 2^-8 (bf16), E = 2^-23 = 2u charged per fp32 operation on a
summation path. A multiply-add is charged as a product and an addition (two roundings), so no bound depends on
contraction; the true first-order cost of an operation is u, and the other u of every E pays for the
higher-order terms ((1 + u)^L - 1 <= L E for every L used here).

Layout (``Layout``): a history is ``[bsz][m rows of row_stride][d]`` elements inside one flat buffer, dense
(row_stride = d, batch_stride = m d) or padded (row_stride = d + 4, batch_stride = m row_stride + 8), with a
band of 64 elements before and after. Everything that is not a row i < n of valid data is NaN: the padding, the
bands, the rows >= n, and G[fr] before a one-fresh call. An input buffer must come back bit-identical, an
output buffer bit-identical outside the rows the kernel is to write.

gram_kernel<N, ONE, FT, HT>, one workgroup per (chunk c, batch b); chunk4 = ceil(d4 / chunks), the chunk owns
the float4 vectors [c chunk4, min((c + 1) chunk4, d4)), lane t the vectors c chunk4 + t + 256 k.
    stored G    a fresh row EQUALS fl32(F - X) (fp32 history) or bf16(fl32(F - X)) (bf16 history, round to
                nearest even); every other element of the G buffer keeps its bits
    part[b][c][p(i, j)]  against the float64 sum over the chunk of g_i g_j. g is the EXACT difference F - X
                for a row the launch forms itself (every row on the all-fresh path, row fr on the one-fresh
                path: the kernel uses the unrounded fp32 difference there, whatever it stores) and the stored
                G, as supplied, for the others (the bf16 rounding of a stored row is input, not error).
                Per element of the sum: fl32(f - x) costs u per fresh factor (nf u, nf in {0, 1, 2}); one
                product; 3 additions in ``dot4``; T = ceil(chunk4 / 256) accumulations into acc; the wave
                sum, 4 DPP levels and 2 levels over the four row totals (6); the 4 waves added in sequence:
                    L_c = 1 + 3 + T + 6 + 4,    |err| <= (nf u + L_c E) sum |g_i| |g_j|
    fn = part[b][c][36]  against the float64 sum of f_last^2, the same with nf = 0
    unused slots p >= n (n + 1) / 2, p != 36, and every slot of a chunk that owns no vector: EQUAL 0
    totals      the wrapper adds the chunks with ``part.sum(1)`` (PyTorch's order: at most ``chunks - 1``
                additions on any path), ``solve_kernel`` in sequence from 0 (the first addition exact, so
                ``chunks - 1``): L = L_c + chunks - 1 (``gram_total_L``)

solve_kernel<N> (thread b owns batch element b; 1024 threads at most):
    res         a1 = sum_b g_b[last][last], a2 = sum_b fn_b, each the chunk sum (chunks - 1), the wave sum (6)
                and the waves in sequence (W = ceil(bsz / 64) <= 16); every term is non-negative, so each sum
                is within L_a E of itself, L_a = chunks - 1 + 6 + W; a square root halves a relative error and
                adds its own rounding. res = sqrt(a1) / (fl32(1e-5) + sqrt(a2)): numerator L_a E / 2 + E,
                denominator at most L_a E / 2 + E and the addition E, the division E:
                    |res - ref| <= (L_a + 4) E ref     (sqrt and division charged E although correctly rounded)
    alpha       backward error, not forward error. H = [[0, 1^T], [1, G + lam I]], M = n + 1, built in float64
                from the supplied partials (G = sum over chunks) and the fp32 value of lam. The kernel's own H
                differs by dH = (chunks - 1) E sum_c |part_c| + u |H| (chunk sums; the rounding of g + lam),
                row and column 0 exact. Gaussian elimination with partial pivoting and two triangular solves
                give (Higham, Accuracy and Stability, Thm 9.4) |P H a - P e_0| <= gamma_3M |L| |U| |a| for the
                computed factors; the products and subtractions of the kernel's fmas are the operations
                counted there; the multiplier is H[r][k] * fl(1 / H[k][k]), one rounding more than the division
                counted there: 3M + 1 roundings of u. L and U are taken from a float64 elimination with the
                kernel's pivot rule (the first largest), so the count is doubled to cover the fp32 factors
                differing from them (and a_0, below):
                    gamma = 2 (3M + 1) u = (3M + 1) E,   B = P^T gamma |L| |U| |a| + dH |a|   (per row of H)
                a_0 is not an output. Row 0 does not need it: |sum alpha - 1| <= B_0. a_0 is taken from row 1
                (a_0 = -H[1, 1:] alpha, within B_1 of the kernel's) and rows i >= 2 must satisfy
                |a_0 + H[i, 1:] alpha| <= B_i + B_1. n = 1: alpha EQUALS 1 for any Gram (the multiplier of
                the only elimination step is 0 * 1).
                Condition: every float64 pivot non-zero and the emulation finite (asserted in the CPU half).

mix_kernel<N, MIXX, Z, FT, HT>: sf = sum_i a_i f_i from 0 in sequence (the first addition exact), sx likewise,
o = beta sf + c sx with c = fl32(1 - beta); MIXX = (beta != 1), otherwise o = sf. The reference is the float64
value of the same expression with beta and c the fp32 values the kernel uses. A term passes one product, n - 1
additions, the product with beta (or c) and the last addition: n + 2 roundings (n without MIXX):
    |o - ref| <= ops E (|beta| sum |a_i f_i| + |c| sum |a_i x_i|) = B_o
    X[:, slot]  fp32 history: B_o; bf16 history: B_o + u_b (|ref| + B_o)
    z           B_o + u_z (|ref| + B_o) (+ 2^-25 for fp16, ``norm_edges.rt``); fp32 z: B_o
    EQUAL       fp32 history: z == X[:, slot].to(z dtype); bf16 history and bf16 z: z == X[:, slot]; bf16
                history and fp32 z: X[:, slot] == bf16(z); every other element of X, and all of F, keep their bits

adjoint_step_kernel<T>, lane (block, t) owns the 8-element vectors block 256 + t + k blocks 256:
    u_new       EQUALS T(fl32(vjp + grad))
    part[block] against the float64 sum of (u_new - u)^2 over the block's elements, u_new as stored.
                dlt = fl32(u_new - u) costs u, squared 2u; one product; 8 K accumulations for the lane's K
                vectors; the wave sum (6); 4 waves: L_b = 1 + 8 K + 6 + 4, |err| <= (2u + L_b E) sum dlt^2
                (K = ceil(ceil(n8 / 256) / blocks)); a block that owns no vector stores 0
    ss          the reduce over the block partials is charged ``blocks`` additions: L = L_b + blocks
    flag        ss <= thresh2: 1 at a threshold above ref (1 + 2 rel), 0 below ref (1 - 2 rel), 1 at the
                kernel's own ss and 0 one float below it; 1 at thresh2 == ss in the integer case

Exact cases (EQUAL): gram "exact" (X integers of magnitude <= 8, F - X in {-2 .. 2}: every pair sum and fn an
integer below 2^24 in any order); mix "exact" (alpha in {0, +-0.5, +-1, +-2}, F and X integers of magnitude
<= 2, beta in {1, 0.5}: every partial sum a multiple of 1/4 below 64); solve n = 1, and 2^k I with lam = 0 at
n = 2 (alpha = 1 / 2; at n = 4 and 8 the elimination divides by the pivot 3 and a correctly rounded fp32 result
is one unit in the last place from 1 / n: the bound); adjoint "int" (integers: dlt in {-1, 0, 1}, ss and every
partial an integer).

Float32 emulation (``emu_gram`` / ``emu_solve`` / ``emu_mix`` / ``emu_adjoint``): the kernels' formulas in
float32 PyTorch (no fma) on the same flat buffers and strides, in the kernels' summation order (``seqsum`` per
lane, ``wave_tree``, the waves and chunks in sequence), rounded where the kernels round. Planted defects
(``defect=``): gram "drop_vec" (the last vector of a chunk), "stale" (G[fr] read on the one-fresh path),
"fn_row0" (fn from row 0), "row_stride_d" (rows read at i d), "trunc" (bf16 store by truncation);
``sum_chunks`` "last_chunk" (the last chunk's partial not summed); solve "pidx" (pair (2, 5) reads pair
(2, 4) at n = 8), "swap_y" (a pivot swap that leaves y behind), "no_pivot" (no pivoting below row 1); mix
"swap_beta", "alpha_n8" (alpha[b * 8 + i]), "trunc", "row_stride_d"; adjoint "unrounded" (ss from
vjp + grad - u without the rounding to T).
"""
import torch

from . import mfma_edges as E
from .mfma_edges import E23, TINY, U8
from .norm_edges import U32, UT, rt, seqsum

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
CODE = {F32: 7, BF: 9, HF: 6}   # ``multi_tensor.DTYPE_CODE`` (asserted in the CPU half)
KT, KP, KOUT, M_ROWS, BAND = 256, 36, 37, 8, 64
NAN = float("nan")
GRAM_FAMILIES = ("gauss", "converging", "collinear", "scaled", "cancel", "exact")
SOLVE_FAMILIES = ("gauss", "converging", "collinear", "scaled", "cancel", "identity", "tie", "below1", "above1")
WORST = {}


def check(key, name, got, ref, bnd, errs):
    """``mfma_edges.check``; the worst |err| / bound is also kept per ``key`` (kernel, output, family)."""
    E.check(name, got, ref, bnd, errs)
    g = got.double()
    if g.shape == ref.shape and bool(torch.isfinite(g).all()) and g.numel():
        err = (g - ref).abs()
        r = float((err / bnd).max()) if bnd is not None else (0.0 if not bool((err != 0).any()) else float("inf"))
        WORST[key] = max(WORST.get(key, 0.0), r)


def worst_lines(prefix=""):
    return [f"WORST {prefix}{' '.join(map(str, k))}: {v:.3f}" for k, v in sorted(WORST.items(), key=str)]


def ceil_div(a, b):
    return -(-a // b)


def pidx(i, j, n):
    """The kernels' packed index of pair i <= j: the row-major upper triangle."""
    return i * n - i * (i - 1) // 2 + (j - i)


def pairs(n):
    return [(i, j) for i in range(n) for j in range(i, n)]


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(name, a, b, errs):
    d = bits(a) != bits(b)
    if bool(d.any()):
        errs.append(f"{name}: {int(d.sum())} elements changed their bits (first at {int(d.flatten().nonzero()[0])})")


# ------------------------------------------------------------------------------- layout and guard bands

class Layout:
    """[bsz][m rows of rs][d] inside a flat buffer with a band of ``BAND`` elements on either side."""

    def __init__(self, bsz, d, padded=False, m=M_ROWS):
        self.bsz, self.m, self.d, self.padded = bsz, m, d, padded
        self.rs = d + 4 if padded else d
        self.bs = m * self.rs + 8 if padded else m * d
        self.numel = 2 * BAND + bsz * self.bs

    def view(self, buf, rs=None):
        return torch.as_strided(buf, (self.bsz, self.m, self.d), (self.bs, self.rs if rs is None else rs, 1), BAND)

    def place(self, vals, dtype, n):
        """A NaN buffer of ``dtype`` holding ``vals[:, i]`` (float32 values, [bsz, m, d]) in the rows i < n."""
        buf = torch.full((self.numel,), NAN, dtype=dtype)
        self.view(buf)[:, :n] = vals[:, :n].to(dtype)
        return buf

    def ptr(self, buf):
        return buf.data_ptr() + BAND * buf.element_size()


def banded(n, dtype, device):
    """An output of ``n`` elements, NaN, between two NaN bands of ``BAND`` elements: (buffer, view)."""
    buf = torch.full((n + 2 * BAND,), NAN, dtype=dtype, device=device)
    return buf, buf[BAND:BAND + n]


def take_banded(name, pair, errs):
    """The view's contents on the CPU after checking that both bands kept their bits."""
    buf, view = pair
    fresh = torch.full((BAND,), NAN, dtype=buf.dtype, device=buf.device)
    for side, band in (("before", buf[:BAND]), ("after", buf[BAND + view.numel():])):
        if not torch.equal(bits(band), bits(fresh)):
            errs.append(f"{name}: the band {side} the output was overwritten")
    return view.detach().cpu().clone()


# ------------------------------------------------------------------------------- summation order

def wave_tree(t):
    """``wave_sum_dpp`` over the last dimension (64 lanes): neighbours, pairs, the rotations by 4 and 8 inside
    each row of 16, then the four row totals as (r0 + r1) + (r2 + r3)."""
    idx = torch.arange(64)
    row, col = idx // 16 * 16, idx % 16
    for perm in (idx ^ 1, idx ^ 2, row + (col + 4) % 16, row + (col + 8) % 16):
        t = t + t[..., perm]
    return (t[..., 0] + t[..., 16]) + (t[..., 32] + t[..., 48])


def block_sum(lanes):
    """[..., 256] lane values -> the workgroup's total: the wave sums, then the 4 waves in sequence from 0."""
    w = wave_tree(lanes.reshape(*lanes.shape[:-1], 4, 64))
    return seqsum(w.movedim(-1, 0))


def lane_acc(v):
    """[..., nv] per-vector values of one chunk -> [..., 256] lane accumulators (lane t adds t, t + 256, ...)."""
    nv = v.shape[-1]
    T = max(1, ceil_div(nv, KT))
    pad = torch.zeros(*v.shape[:-1], T * KT, dtype=v.dtype)
    pad[..., :nv] = v
    return seqsum(pad.reshape(*v.shape[:-1], T, KT).movedim(-2, 0))


def dot4(a, b):
    p = a * b
    return ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]


# ------------------------------------------------------------------------------- gram: geometry and inputs

def gram_chunks_ref(bsz, d):
    """The documented ``anderson_gram_chunks``: about 2048 workgroups, at least 4 vectors per lane and chunk."""
    return max(1, min(ceil_div(2048, max(bsz, 1)), ceil_div(d // 4, 4 * KT)))


def gram_geometry(d, chunks):
    """(chunk4, T, vectors of the last non-empty chunk, number of empty chunks)."""
    d4 = d // 4
    chunk4 = ceil_div(d4, chunks)
    sizes = [max(0, min(d4, (c + 1) * chunk4) - c * chunk4) for c in range(chunks)]
    full = [s for s in sizes if s > 0]
    return chunk4, ceil_div(chunk4, KT), full[-1], sizes.count(0)


def gram_chunk_L(d, chunks):
    return 1 + 3 + gram_geometry(d, chunks)[1] + 6 + 4


def gram_total_L(d, chunks):
    return gram_chunk_L(d, chunks) + chunks - 1


def gram_inputs(family, bsz, d, fdt, hdt, seed=0, m=M_ROWS):
    """(X, F): float32 values [bsz, m, d], X representable in ``hdt`` and F in ``fdt``."""
    g = E._gen("anderson_gram", family, bsz, d, seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    if family == "exact":
        X = torch.randint(-8, 9, (bsz, m, d), generator=g).float()
        F = X + torch.randint(-2, 3, (bsz, m, d), generator=g).float()
    elif family == "gauss":
        X, F = rn(bsz, m, d), rn(bsz, m, d)
    else:
        X = rn(bsz, m, d)
        if family == "converging":
            dlt = 2.0 ** -10 * rn(bsz, m, d)
        elif family == "collinear":
            dlt = rn(bsz, 1, d) + 2.0 ** -10 * rn(bsz, m, d)
        elif family == "scaled":
            s = (2.0 ** (-20.0 * torch.arange(m) / (m - 1))).view(1, m, 1)
            X = X * s
            dlt = s * rn(bsz, m, d)
        elif family == "cancel":  # odd rows (w, -w, ...), even rows (w, w, ...): odd x even sums cancel in pairs
            w = rn(bsz, m, d // 2, 1)
            sg = torch.ones(1, m, 1, 2)
            sg[:, 1::2, :, 1] = -1
            dlt = (w * sg).reshape(bsz, m, d)
            X = 0.25 * X
        else:
            raise ValueError(family)
        X = X.to(hdt).float()
        F = X + dlt
    return X.to(hdt).float(), F.to(fdt).float()


def stored(gv, hdt, trunc=False):
    """The stored form of fp32 difference rows: as they are, or bf16 (round to nearest even)."""
    if hdt == F32:
        return gv
    return (E.trunc_bf16(gv) if trunc else gv.to(BF)).float()


def _chunked(t, chunks, chunk4):
    """[bsz, r, d] -> [bsz, r, chunks, 4 chunk4], zero beyond d."""
    bsz, r, d = t.shape
    pad = torch.zeros(bsz, r, chunks * chunk4 * 4, dtype=t.dtype)
    pad[..., :d] = t
    return pad.view(bsz, r, chunks, chunk4 * 4)


def gram_refs(X, F, hdt, chunks):
    """Float64 per-chunk sums over all m rows, [bsz, chunks, m, m]: EE (both factors the exact difference), SS
    (both the stored fl / bf16 difference), ES (first exact, second stored), each with its sum of absolute
    products; FF [bsz, chunks, m] the sums of f^2. ``gs``: the stored differences [bsz, m, d]."""
    d = X.shape[2]
    chunk4 = ceil_div(d // 4, chunks)
    gs = stored(F - X, hdt)
    ge = _chunked(F.double() - X.double(), chunks, chunk4)
    gsc = _chunked(gs.double(), chunks, chunk4)
    ein = lambda a, b: torch.einsum("bicl,bjcl->bcij", a, b)
    r = dict(gs=gs, EE=ein(ge, ge), SS=ein(gsc, gsc), ES=ein(ge, gsc), aEE=ein(ge.abs(), ge.abs()),
             aSS=ein(gsc.abs(), gsc.abs()), aES=ein(ge.abs(), gsc.abs()))
    r["FF"] = (_chunked(F.double(), chunks, chunk4) ** 2).sum(3).permute(0, 2, 1)
    return r


def gram_expected(refs, n, last, one):
    """(ref, mag [bsz, chunks, 37], nf [37]) of one launch: the float64 sums, the sums of absolute products and
    the number of fresh factors per slot; unused slots have ref 0 and mag 0 (EQUAL)."""
    bsz, chunks = refs["EE"].shape[:2]
    ref = torch.zeros(bsz, chunks, KOUT, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    nfs = torch.zeros(KOUT, dtype=torch.float64)
    for i, j in pairs(n):
        if not one or (i == last and j == last):
            k, a, b, nf = "EE", i, j, 2
        elif i == last or j == last:
            k, a, b, nf = "ES", last, (j if i == last else i), 1
        else:
            k, a, b, nf = "SS", i, j, 0
        p = pidx(i, j, n)
        ref[:, :, p] = refs[k][:, :, a, b]
        mag[:, :, p] = refs["a" + k][:, :, a, b]
        nfs[p] = nf
    ref[:, :, KP] = mag[:, :, KP] = refs["FF"][:, :, last]
    return ref, mag, nfs


def gram_bound(mag, nfs, L):
    return (nfs * U32 + L * E23) * mag


def check_sums(key, tag, got, ref, mag, nfs, L, exact, errs):
    """Partials [bsz, chunks, 37] (or totals [bsz, 37]) against (nf u + L E) mag; the exact family and every
    slot whose ``mag`` is 0 (unused, or a chunk that owns no vector) EQUAL."""
    if exact:
        check(key, tag, got, ref, None, errs)
        return
    zero = mag == 0
    E.check(f"{tag} unused / empty", torch.where(zero, got.double(), torch.zeros_like(ref)), torch.zeros_like(ref), None, errs)
    check(key, tag, got, ref, gram_bound(mag, nfs, L) + TINY + zero.double() * 1e300, errs)


def sum_chunks(part, defect=None):
    """``solve_kernel``'s chunk sum: in sequence from 0 (float32)."""
    p = part[:, :-1] if defect == "last_chunk" and part.shape[1] > 1 else part
    return seqsum(p.movedim(1, 0))


# ------------------------------------------------------------------------------- gram: emulation

def emu_gram(lay, Xb, Fb, Gb, n, last, chunks, one, defect=None):
    """gram_kernel on flat CPU buffers: (part [bsz, chunks, 37] float32, the G buffer after the launch)."""
    rs = lay.d if defect == "row_stride_d" else None
    X, F = lay.view(Xb, rs)[:, :n].float(), lay.view(Fb, rs)[:, :n].float()
    hdt = Xb.dtype
    Gb = None if Gb is None else Gb.clone()
    rnd = lambda t: t if hdt == F32 else (E.trunc_bf16(t) if defect == "trunc" else t.to(BF))
    if one:
        gn = F[:, last] - X[:, last]
        g = lay.view(Gb, rs)[:, :n].float().clone()
        if defect != "stale":
            g[:, last] = gn
        lay.view(Gb, rs)[:, last] = rnd(gn)
        fl = F[:, last]
    else:
        g = F - X
        if Gb is not None:
            lay.view(Gb, rs)[:, :n] = rnd(g)
        fl = F[:, 0 if defect == "fn_row0" else last]
    bsz, d = lay.bsz, lay.d
    d4 = d // 4
    chunk4 = ceil_div(d4, chunks)
    g4 = _chunked(g, chunks, chunk4).view(bsz, n, chunks, chunk4, 4)
    f4 = _chunked(fl[:, None], chunks, chunk4).view(bsz, 1, chunks, chunk4, 4)
    I = torch.tensor([i for i, _ in pairs(n)])
    J = torch.tensor([j for _, j in pairs(n)])
    v = torch.cat([dot4(g4[:, I], g4[:, J]), dot4(f4, f4)], 1)  # [bsz, P + 1, chunks, chunk4]
    if defect == "drop_vec":
        for c in range(chunks):
            v1 = min(d4, (c + 1) * chunk4) - c * chunk4
            if v1 > 0:
                v[:, :, c, v1 - 1] = 0
    tot = block_sum(lane_acc(v))  # [bsz, P + 1, chunks]
    part = torch.zeros(bsz, chunks, KOUT)
    part[:, :, :len(I)] = tot[:, :-1].permute(0, 2, 1)
    part[:, :, KP] = tot[:, -1]
    return part, Gb


# ------------------------------------------------------------------------------- solve

def solve_rows(family, n, bsz, seed=0, dd=64, lam=1e-4):
    """Difference rows [bsz, n, dd] (float64) whose Gram matrix the synthetic partials carry."""
    g = E._gen("anderson_solve", family, n, seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    if family == "gauss":
        return 0.8 * rn(bsz, n, dd)                          # F = X + 0.1 randn at d = 4100: entries of about 41
    if family == "converging":
        return 2.0 ** -10 * rn(bsz, n, dd)
    if family == "collinear":                                # base Gram about 1, noise Gram about 6e-5: 1000 u
        return rn(bsz, 1, dd) / 8 + 2.0 ** -10 * rn(bsz, n, dd)
    if family == "scaled":
        # row norms fall by 2^-20 from the oldest to the newest row (n - 1). The Schur complement of the small
        # rows is of the order of lam and is formed by subtracting entries of the order of the largest Gram
        # entry, so fp32 loses it once lam is below u times that entry and the last pivot comes out 0. The
        # largest entry is therefore kept at about 2^13 lam (lam = 2000 u of it): 0.8 at lam 1e-4, 8e-5 at 1e-8
        s = 2.0 ** (-20.0 * torch.arange(n, dtype=torch.float64) / max(n - 1, 1))
        return rn(bsz, n, dd) * s.view(1, n, 1) * (2.0 ** 13 * lam / dd) ** 0.5
    if family == "cancel":                                   # rows in +- pairs up to noise
        r = rn(bsz, n, dd) / 8
        r[:, 1::2] = -r[:, 0:2 * (n // 2):2] + 2.0 ** -10 * rn(bsz, n // 2, dd)
        return r
    raise ValueError(family)


def solve_partials(family, n, bsz, chunks, seed=0, lam=1e-4):
    """(part [bsz, chunks, 37] float32, lam values): a Gram matrix split over ``chunks`` partials."""
    g = E._gen("anderson_solve_part", family, n, chunks, seed)
    eye = torch.eye(n, dtype=torch.float64)
    k = (torch.arange(bsz) % 5 - 2).double().view(bsz, 1, 1)
    if family == "identity":
        G, lams = 2.0 ** k * eye, (0.0,)
    elif family == "tie":       # equal candidates in every pivot column; H exactly representable
        G, lams = 2.0 ** k * (eye + 1), (0.0, 1e-4)
    elif family == "below1":    # entries below 1: |1| of row 0 outranks them at k = 1
        G, lams = 2.0 ** -4 * (eye + 0.25 + 0.125 * torch.rand(bsz, 1, 1, generator=g).double()), (1e-4, 1e-8)
    elif family == "above1":    # entries above 1: the pivot of column 1 leaves row 0
        d0 = 1 + torch.arange(n, dtype=torch.float64)
        G, lams = 16.0 * (torch.diag(d0) + 0.25 + 0.125 * torch.rand(bsz, 1, 1, generator=g).double()), (1e-4, 1e-8)
    else:
        r = solve_rows(family, n, bsz, seed, lam=lam)
        G, lams = r @ r.transpose(1, 2), (1e-4, 1e-8)
    exact = family in ("identity", "tie")
    if exact:  # split into exactly representable parts: halves
        w = torch.tensor([0.5 ** (c + 1) for c in range(chunks)], dtype=torch.float64)
        w[-1] = 1 - w[:-1].sum()
    else:
        w = torch.rand(chunks, generator=g).double() + 0.25
        w = w / w.sum()
    part = torch.zeros(bsz, chunks, KOUT)
    for i, j in pairs(n):
        part[:, :, pidx(i, j, n)] = (G[:, i, j, None] * w).float()
    fn = (G.diagonal(dim1=1, dim2=2).sum(1) * (2 + torch.rand(bsz, generator=g).double()))
    part[:, :, KP] = (fn[:, None] * w).float()
    return part, lams


def build_H(gsum, n, lam, defect=None):
    """[bsz, M, M] from chunk-summed partials [bsz, 37] in ``gsum``'s dtype."""
    bsz = gsum.shape[0]
    H = torch.zeros(bsz, n + 1, n + 1, dtype=gsum.dtype)
    H[:, 0, 1:] = 1
    H[:, 1:, 0] = 1
    lam_t = torch.tensor(lam, dtype=torch.float32).to(gsum.dtype)
    for i, j in pairs(n):
        p = pidx(i, j, n)
        if defect == "pidx" and n == 8 and (i, j) == (2, 5):
            p = pidx(2, 4, n)
        H[:, 1 + i, 1 + j] = gsum[:, p] + (lam_t if i == j else 0)
        H[:, 1 + j, 1 + i] = H[:, 1 + i, 1 + j]
    return H


def eliminate(H, defect=None):
    """solve_kernel's elimination of H a = e_0 in H's dtype without fma: dict(x, LU (multipliers below the
    diagonal, getrf layout), perm (row r of P H is row perm[r] of H), piv [M] pivot rows chosen, pivots)."""
    H = H.clone()
    B, M, _ = H.shape
    ar = torch.arange(B)
    y = torch.zeros(B, M, dtype=H.dtype)
    y[:, 0] = 1
    perm = torch.arange(M).repeat(B, 1)
    seq = []
    for k in range(M):
        if defect == "no_pivot" and k >= 1:
            piv = torch.full((B,), k)
        else:
            piv = k + torch.argmax(H[:, k:, k].abs(), dim=1)  # the first largest
        seq.append(piv)
        for t in (H, perm) if defect == "swap_y" else (H, perm, y):
            a, b = t[ar, k].clone(), t[ar, piv].clone()
            t[ar, k], t[ar, piv] = b, a
        inv = 1 / H[:, k, k]
        f = H[:, k + 1:, k] * inv[:, None]
        H[:, k + 1:, k + 1:] = H[:, k + 1:, k + 1:] - f[:, :, None] * H[:, k, None, k + 1:]
        y[:, k + 1:] = y[:, k + 1:] - f * y[:, k, None]
        H[:, k + 1:, k] = f
    x = torch.zeros(B, M, dtype=H.dtype)
    for k in range(M - 1, -1, -1):
        s = y[:, k]
        for c in range(k + 1, M):
            s = s - H[:, k, c] * x[:, c]
        x[:, k] = s / H[:, k, k]
    return dict(x=x, LU=H, perm=perm, piv=torch.stack(seq, 1), pivots=H.diagonal(dim1=1, dim2=2))


def res_L(chunks, bsz):
    return chunks - 1 + 6 + ceil_div(bsz, 64) + 4


def res_ref(part, last, n):
    """(ref, bound) of the relative residual from the supplied partials."""
    p = part.double()
    a1, a2 = p[:, :, pidx(last, last, n)].sum(), p[:, :, KP].sum()
    ref = a1.sqrt() / (float(torch.tensor(1e-5, dtype=torch.float32)) + a2.sqrt())
    return ref.reshape(1), (res_L(part.shape[1], part.shape[0]) * E23 * ref + TINY).reshape(1)


def emu_solve(part, n, last, lam, defect=None):
    """solve_kernel in float32: (alpha [bsz, n], res [1])."""
    bsz = part.shape[0]
    g = sum_chunks(part.float(), "last_chunk" if defect == "last_chunk" else None)
    W = ceil_div(bsz, 64)
    lanes = torch.zeros(2, W * 64)
    lanes[0, :bsz], lanes[1, :bsz] = g[:, pidx(last, last, n)], g[:, KP]
    a = seqsum(wave_tree(lanes.view(2, W, 64)).movedim(1, 0))
    res = a[0].sqrt() / (torch.tensor(1e-5, dtype=torch.float32) + a[1].sqrt())
    out = eliminate(build_H(g, n, lam, defect), defect)
    return out["x"][:, 1:], res.reshape(1)


def solve_gamma(n):
    return (3 * (n + 1) + 1) * E23


def solve_check(key, tag, part, n, lam, alpha, errs, extra=0.0):
    """The backward-error criterion (module docstring). Returns the float64 elimination (for the CPU half).
    ``extra``: a solver that formed its own Gram matrix, within ``extra sum |g_i| |g_j|`` of the supplied one;
    by Cauchy-Schwarz that sum is at most sqrt(G_ii G_jj), which is what dH is charged."""
    bsz, chunks = part.shape[:2]
    p = part.double()
    H = build_H(p.sum(1), n, lam)
    el = eliminate(H)
    a = alpha.double()
    if n == 1:
        check(key, f"{tag} alpha (n = 1)", a, torch.ones(bsz, 1, dtype=torch.float64), None, errs)
        return el
    if not bool(torch.isfinite(a).all()):
        errs.append(f"{tag}: {int((~torch.isfinite(a)).sum())} non-finite alpha")
        return el
    M = n + 1
    dH = torch.zeros_like(H)
    dH[:, 1:, 1:] = (chunks - 1) * E23 * build_H(p.abs().sum(1), n, 0.0)[:, 1:, 1:] + U32 * H[:, 1:, 1:].abs()
    if extra:
        dg = H[:, 1:, 1:].diagonal(dim1=1, dim2=2).clamp_min(0).sqrt()
        dH[:, 1:, 1:] += extra * dg[:, :, None] * dg[:, None, :]
    av = torch.cat([-(H[:, 1, 1:] * a).sum(1, keepdim=True), a], 1)
    LU = el["LU"]
    Lm = torch.tril(LU, -1).abs() + torch.eye(M, dtype=torch.float64)
    Um = torch.triu(LU).abs()
    piv_b = solve_gamma(n) * (Lm @ (Um @ av.abs()[:, :, None]))[:, :, 0]
    B = torch.zeros_like(piv_b).scatter(1, el["perm"], piv_b) + (dH @ av.abs()[:, :, None])[:, :, 0]
    r = (H @ av[:, :, None])[:, :, 0]
    r[:, 0] -= 1
    bnd = B.clone()
    bnd[:, 2:] += B[:, 1:2]
    keep = [0] + list(range(2, M))  # row 1 defines a_0
    check(key, f"{tag} |H a - e0|", r[:, keep], torch.zeros(bsz, len(keep), dtype=torch.float64), bnd[:, keep] + TINY, errs)
    return el


def solve_forward(part, n, lam):
    """The float64 solution of the same system (the forward-error reference of ``test_deq.py``)."""
    return eliminate(build_H(part.double().sum(1), n, lam))["x"][:, 1:]


# ------------------------------------------------------------------------------- mix

def mix_inputs(family, bsz, d, fdt, hdt, seed=0, m=M_ROWS):
    """(X, F [bsz, m, d], alpha [bsz, 8]) float32 values; alpha[:, :n] is the launch's alpha."""
    g = E._gen("anderson_mix", family, bsz, d, seed)
    if family == "exact":
        X = torch.randint(-2, 3, (bsz, m, d), generator=g).float()
        F = torch.randint(-2, 3, (bsz, m, d), generator=g).float()
        vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
        return X, F, vals[torch.randint(0, 7, (bsz, m), generator=g)]
    X, F = gram_inputs("converging" if family == "cancel" else family, bsz, d, fdt, hdt, seed, m)
    alpha = torch.randn(bsz, m, generator=g)
    if family == "cancel":  # a solve on nearly collinear rows: weights of about +-1000 that sum to 1
        alpha = 1000 * alpha
        alpha[:, 0] += 1 - alpha.sum(1)
    return X, F, alpha


def mix_ops(n, beta):
    return n + 2 if beta != 1.0 else n


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def mix_ref(X, F, alpha, n, beta):
    """(ref, B_o) [bsz, d] float64."""
    b32 = f32(beta)
    a = alpha[:, :n].double()[:, :, None]
    tf, tx = a * F[:, :n].double(), a * X[:, :n].double()
    if beta == 1.0:
        return tf.sum(1), mix_ops(n, beta) * E23 * tf.abs().sum(1) + TINY
    b, c = float(b32), float(f32(1.0) - b32)
    return b * tf.sum(1) + c * tx.sum(1), mix_ops(n, beta) * E23 * (abs(b) * tf.abs().sum(1) + abs(c) * tx.abs().sum(1)) + TINY


def mix_exact_asserts(X, F, alpha, n, beta, hdt, zdt):
    ref, _ = mix_ref(X, F, alpha, n, beta)
    for t in (hdt, zdt):
        if t is not None:
            assert bool((ref.to(t).double() == ref).all()), f"the exact mix does not survive {t}"
    assert float(ref.abs().max()) <= 64 and bool((ref != 0).any())
    return ref


def check_mix(key, tag, X, F, alpha, n, slot, beta, hdt, zdt, row, z, exact, errs):
    """The stored row ``row`` (hdt) and ``z`` (zdt or None) of one launch; the EQUAL relations between them."""
    ref, Bo = mix_ref(X, F, alpha, n, beta)
    if exact:
        ref = mix_exact_asserts(X, F, alpha, n, beta, hdt, zdt)
    rb = None if exact else (Bo if hdt == F32 else Bo + U8 * (ref.abs() + Bo))
    check(key + ("X",), f"{tag} X[:, slot]", row, ref, rb, errs)
    if z is None:
        return
    zb = None if exact else (Bo if zdt == F32 else Bo + rt(zdt, ref) + UT[zdt] * Bo)
    check(key + ("z",), f"{tag} z", z, ref, zb, errs)
    if hdt == F32:
        same_bits(f"{tag} z == X[:, slot].to(z)", z, row.to(zdt), errs)
    elif zdt == BF:
        same_bits(f"{tag} z == X[:, slot]", z, row, errs)
    elif zdt == F32:
        same_bits(f"{tag} X[:, slot] == bf16(z)", row, z.to(BF), errs)


def emu_mix(lay, Xb, Fb, alpha, n, slot, beta, zdt, defect=None):
    """mix_kernel on flat CPU buffers: (the X buffer after the launch, z [bsz, d] or None, the fp32 value o
    before either store)."""
    rs = lay.d if defect == "row_stride_d" else None
    hdt = Xb.dtype
    Xb = Xb.clone()
    X, F = lay.view(Xb, rs)[:, :n].float(), lay.view(Fb, rs)[:, :n].float()
    a = alpha[:, :n].float().contiguous()
    if defect == "alpha_n8":
        flat = torch.cat([a.flatten(), torch.zeros(lay.bsz * 8)])
        a = torch.stack([flat[b * 8:b * 8 + n] for b in range(lay.bsz)])
    sf, sx = torch.zeros(lay.bsz, lay.d), torch.zeros(lay.bsz, lay.d)
    for i in range(n):
        sf = sf + a[:, i, None] * F[:, i]
        sx = sx + a[:, i, None] * X[:, i]
    o = sf
    if beta != 1.0:
        b, c = f32(beta), f32(1.0) - f32(beta)
        if defect == "swap_beta":
            b, c = c, b
        o = b * sf + c * sx
    lay.view(Xb, rs)[:, slot] = o if hdt == F32 else (E.trunc_bf16(o) if defect == "trunc" else o.to(BF))
    return Xb, (None if zdt is None else o.to(zdt)), o


# ------------------------------------------------------------------------------- adjoint_step

def adjoint_blocks_ref(n):
    return max(1, min(1024, ceil_div(n // 8, KT * 4)))


def adjoint_K(n, blocks):
    return ceil_div(ceil_div(n // 8, KT), blocks)


def adjoint_L(n, blocks):
    return 1 + 8 * adjoint_K(n, blocks) + 6 + 4


def adjoint_inputs(family, n, dtype, seed=0):
    """(vjp, grad, u) flat tensors of ``dtype``. "int": integers, u_new - u in {-1, 0, 1}."""
    g = E._gen("adjoint_step", family, n, seed)
    if family == "int":
        v = torch.randint(-1, 2, (n,), generator=g)
        gr = torch.randint(-1, 2, (n,), generator=g)
        u = v + gr - torch.randint(-1, 2, (n,), generator=g)
        return v.to(dtype), gr.to(dtype), u.to(dtype)
    v, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    u = v + gr + (2.0 ** -6 if family == "converging" else 1.0) * torch.randn(n, generator=g)
    return v.to(dtype), gr.to(dtype), u.to(dtype)


def adjoint_ref(v, gr, u, blocks):
    """(u_new of T, partial refs [blocks] float64, their sums of squares): u_new = T(fl32(vjp + grad))."""
    un = (v.float() + gr.float()).to(v.dtype)
    d2 = (un.double() - u.double()) ** 2
    n8 = v.numel() // 8
    stride = blocks * KT
    K = max(1, ceil_div(n8, stride))
    pad = torch.zeros(K * stride * 8, dtype=torch.float64)
    pad[:d2.numel()] = d2
    return un, pad.view(K, blocks, KT * 8).sum((0, 2))


def check_adjoint(key, tag, v, gr, u, blocks, un, part, exact, errs):
    ref_un, ref_p = adjoint_ref(v, gr, u, blocks)
    same_bits(f"{tag} u_new", un, ref_un, errs)
    bnd = None if exact else (2 * U32 + adjoint_L(v.numel(), blocks) * E23) * ref_p
    if exact:
        assert float(ref_p.sum()) < 2 ** 24
        check(key, f"{tag} part", part, ref_p, None, errs)
    else:
        zero = ref_p == 0
        E.check(f"{tag} idle blocks", torch.where(zero, part.double(), torch.zeros_like(ref_p)), torch.zeros_like(ref_p), None, errs)
        check(key, f"{tag} part", part, ref_p, bnd + TINY + zero.double() * 1e300, errs)
    return ref_p


def ss_bound(ref_p, n, blocks):
    return (2 * U32 + (adjoint_L(n, blocks) + blocks) * E23) * float(ref_p.sum()) + TINY


def emu_adjoint(v, gr, u, blocks, defect=None):
    """adjoint_step_kernel in float32: (u_new, part [blocks])."""
    s = v.float() + gr.float()
    un = s.to(v.dtype)
    dl = (s if defect == "unrounded" else un.float()) - u.float()
    sq = dl * dl
    n8 = v.numel() // 8
    stride = blocks * KT
    K = max(1, ceil_div(n8, stride))
    pad = torch.zeros(K * stride * 8)
    pad[:sq.numel()] = sq
    lanes = seqsum(pad.view(K, blocks, KT, 8).permute(0, 3, 1, 2).reshape(K * 8, blocks, KT))
    return un, block_sum(lanes)


def emu_adjoint_total(part):
    """deq_adjoint_check_kernel's order: lane t adds part[t], part[t + 256], ...; the wave sums; (w0 + w1) + (w2 + w3)."""
    w = wave_tree(lane_acc(part.float()[None])[0].view(4, 64))
    return (w[0] + w[1]) + (w[2] + w[3])
