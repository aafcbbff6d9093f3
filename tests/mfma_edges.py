"""Inputs, float64 references, derived bounds and planted defects shared by
``test_mfma_edges_gpu.py`` (plain helper module: no fixtures, no tests).

Every operation of the MFMA GEMM / convolution family is brought to one form,
``C[i, j] = sum_k P[i, k] Q[j, k]`` (a 3x3 convolution through ``im2col``, plain slices of the
padded image), so that one reference, one bound and one checker serve all of them.
"""
import math

import torch
import torch.nn.functional as F

U8 = 2.0 ** -8     # bf16 unit roundoff (8 significand bits, round to nearest)
E23 = 2.0 ** -23   # assumed relative error of one fp32 addition (covers nearest and truncation)
TINY = 1e-30
FAMILIES = ("uniform", "cancel", "ternary", "gather")
EXACT = ("ternary", "gather")
BF16_SENTINEL = 0x5A5A        # 1.5e16 as bf16: finite, never produced by these inputs
F32_SENTINEL = 0x5A5A5A5A


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + (k if isinstance(k, int) else sum(map(ord, str(k))))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _uni(g, *shape):
    return torch.rand(*shape, generator=g) * 2 - 1


def mult(k):
    """The multiplier of pi(i) = (m i + 3) mod k: 7, or the next prime that does not divide k."""
    for m in (7, 11, 13, 17):
        if math.gcd(m, k) == 1:
            return m
    return 1


def perm(n, k):
    """pi(i) = (7 i + 3) mod k for i < n (a permutation of Z_k when n == k)."""
    return (mult(k) * torch.arange(n) + 3) % k


def patterns(*shape):
    """Distinct bf16 bit patterns (all 65024 finite normal ones, both signs, before any repeats; the
    order is scrambled by an odd stride coprime to 127 so neighbours differ in sign, exponent and
    significand). Subnormals and zero are left out: a zero hides a dropped term, and whether fp32
    subnormals survive a conversion is a property of the float mode, not of the index arithmetic."""
    n = math.prod(shape)
    i = (torch.arange(n, dtype=torch.int64) * 40503 + 12345) % 65024
    r = i // 2
    bits = ((i % 2) << 15) | ((1 + r // 128) << 7) | (r % 128)
    bits = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16)
    return bits.view(torch.bfloat16).reshape(shape)


def _sparse_ternary(g, rows, k, nnz):
    """[rows, k] in {-1, 0, 1}: every row has min(nnz, k) non-zeros at seeded positions drawn from the
    whole range (a random subset per row: every k-tile and tap is hit by some row)."""
    sign = torch.randint(0, 2, (rows, k), generator=g) * 2 - 1
    if nnz >= k:
        return sign.float()
    kth = torch.rand(rows, k, generator=g)
    thr = kth.kthvalue(nnz, dim=1, keepdim=True).values
    return torch.where(kth <= thr, sign, torch.zeros_like(sign)).float()


def gemm_inputs(family, m, n, k, seed=0, nnz=256):
    """bf16 ``P [m, k]`` and ``Q [n, k]`` (k the reduction) of one family, made on the CPU."""
    g = _gen(family, m, n, k, seed)
    if family == "uniform":
        p, q = _uni(g, m, k), _uni(g, n, k) * k ** -0.5
    elif family == "cancel":
        kp = k // 2
        u, v, w = _uni(g, m, kp), torch.rand(m, kp, generator=g), _uni(g, n, kp) * k ** -0.5
        p, q = torch.zeros(m, k), torch.zeros(n, k)
        p[:, 0:2 * kp:2], p[:, 1:2 * kp:2] = u, -u * (1 + 2.0 ** -6 * v)
        q[:, 0:2 * kp:2] = q[:, 1:2 * kp:2] = w  # an odd k leaves the last index zero on both sides
    elif family == "ternary":
        p = _sparse_ternary(g, m, k, nnz)
        q = (torch.randint(0, 3, (n, k), generator=g) - 1).float()
    elif family == "gather":
        p = torch.zeros(m, k)
        p[torch.arange(m), perm(m, k)] = 1.0
        return p.bfloat16(), patterns(n, k)
    else:
        raise ValueError(family)
    return p.bfloat16(), q.bfloat16()


def linbwd_inputs(family, m, n, k, seed=0):
    """bf16 ``dy [m, n], x [m, k], w [n, k]`` of a Linear backward (dx = dy w reduces over n, dw = dy^T x
    over m); dy serves both reductions. cancel: dy carries the sign pattern (+ -; - +) on 2 x 2 blocks
    over equal pairs of w rows and of x rows. ternary: dy is non-zero on the lattice (i + 7 j) % 4 == 0,
    at most n/4 per row and m/4 per column (<= 256 at the shapes used). gather: dy[i, pi(i)] = 1, so
    dx row i is w row pi(i) (distinct bit patterns) and dw row j is the sum of the x rows with
    pi(i) = j: one row of bit patterns when m == n, else a few signed powers of two (exact in fp32)."""
    g = _gen("linbwd", family, m, n, k, seed)
    if family == "uniform":
        return _uni(g, m, n).bfloat16(), _uni(g, m, k).bfloat16(), (_uni(g, n, k) * n ** -0.5).bfloat16()
    if family == "cancel":
        u = _uni(g, m // 2, n // 2)
        e1, e2 = (1 + 2.0 ** -6 * torch.rand(m // 2, n // 2, generator=g) for _ in range(2))
        dy = torch.zeros(m, n)
        dy[0::2, 0::2], dy[0::2, 1::2], dy[1::2, 0::2], dy[1::2, 1::2] = u, -u * e1, -u * e2, u * e1 * e2
        x, w = torch.zeros(m, k), torch.zeros(n, k)
        x[0::2] = x[1::2] = _uni(g, m // 2, k)
        w[0::2] = w[1::2] = _uni(g, n // 2, k) * n ** -0.5
        return dy.bfloat16(), x.bfloat16(), w.bfloat16()
    if family == "ternary":
        i, j = torch.arange(m).view(m, 1), torch.arange(n).view(1, n)
        sign = (torch.randint(0, 2, (m, n), generator=g) * 2 - 1).float()
        dy = torch.where((i + 7 * j) % 4 == 0, sign, torch.zeros(m, n))
        x = (torch.randint(0, 3, (m, k), generator=g) - 1).float()
        w = (torch.randint(0, 3, (n, k), generator=g) - 1).float()
        return dy.bfloat16(), x.bfloat16(), w.bfloat16()
    dy = torch.zeros(m, n)
    dy[torch.arange(m), perm(m, n)] = 1.0
    return dy.bfloat16(), patterns(m, k) if m == n else _pow2(g, m, k), patterns(n, k)


def _pow2(g, *shape):
    """Signed powers of two 2^0 .. 2^6: sums of up to m / n of them per column stay exact in fp32."""
    return ((torch.randint(0, 2, shape, generator=g) * 2 - 1) * 2.0 ** torch.randint(0, 7, shape, generator=g)).bfloat16()


def conv_inputs(family, n, c, h, w, co, seed=0, nnz=256, dgrad=False):
    """bf16 image ``[n, c_in, h, w]`` and filter ``[co, c, 3, 3]`` (NCHW / OIHW values; the tests lay them
    out). ``dgrad``: the image is dy ``[n, co, h, w]`` and the reduction runs over (co, tap) per input
    channel, so the sparse / one-hot structure is built per input channel instead of per output one."""
    g = _gen("conv", family, n, c, h, w, co, seed, int(dgrad))
    cin, cout = (co, c) if dgrad else (c, co)  # channels of the image operand / of the result
    kred = 9 * cin
    if family == "uniform":
        img, f = _uni(g, n, cin, h, w), _uni(g, cout, cin, 3, 3) * kred ** -0.5
    elif family == "cancel":  # adjacent channel pairs of the image cancel under equal weights
        u = _uni(g, n, cin // 2, h, w)
        img = torch.zeros(n, cin, h, w)
        img[:, 0::2], img[:, 1::2] = u, -u * (1 + 2.0 ** -6 * torch.rand(u.shape, generator=g))
        f = torch.zeros(cout, cin, 3, 3)
        f[:, 0::2] = f[:, 1::2] = _uni(g, cout, cin // 2, 3, 3) * kred ** -0.5
    elif family == "ternary":
        img = (torch.randint(0, 3, (n, cin, h, w), generator=g) - 1).float()
        f = _sparse_ternary(g, cout, 9 * cin, nnz).view(cout, 3, 3, cin).permute(0, 3, 1, 2)
    elif family == "gather":
        img = patterns(n, cin, h, w).float()
        f = torch.zeros(cout, cin, 3, 3)
        o = torch.arange(cout)
        f[o, perm(cout, cin), (o % 9) // 3, o % 3] = 1.0  # result channel o: tap o mod 9 of source channel pi(o)
    else:
        raise ValueError(family)
    if dgrad:  # f is indexed [result = ci][source = co][r][s]: as the filter W[co][ci] with the taps flipped back
        f = f.flip(2, 3).transpose(0, 1)
    return img.bfloat16(), f.contiguous().bfloat16()


# ------------------------------------------------------------------------------- references

def im2col(x, stride=1):
    """[n, c, h, w] -> [n * ho * wo, 9 * c], K ordered (tap r * 3 + s, channel): tap (r, s) of output
    pixel (i, j) is input pixel (stride i + r - 1, stride j + s - 1), zero outside."""
    n, c, h, w = x.shape
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    xp = F.pad(x, (1, 1, 1, 1))
    cols = [xp[:, :, r:r + stride * (ho - 1) + 1:stride, s:s + stride * (wo - 1) + 1:stride]
            for r in range(3) for s in range(3)]
    return torch.stack(cols, 1).permute(0, 3, 4, 1, 2).reshape(n * ho * wo, 9 * c)


def taps(wt):
    """[co, c, 3, 3] -> [co, 9 * c] (tap-major, channel fastest)."""
    return wt.permute(0, 2, 3, 1).reshape(wt.shape[0], -1)


def taps_t(wt):
    """The input gradient's filter: [ci, 9 * co] with WT[ci][r][s][co] = W[co][ci][2 - r][2 - s]."""
    return wt.flip(2, 3).permute(1, 2, 3, 0).reshape(wt.shape[1], -1)


def ref_gemm(p, q, dtype=torch.float64):
    """(R, A) = (P Q^T, |P| |Q|^T) in ``dtype`` (float64: exact for these inputs' purposes)."""
    p, q = p.to(dtype), q.to(dtype)
    return p @ q.t(), p.abs() @ q.abs().t()


def rn_bf16(x):
    return x.float().bfloat16()


def trunc_bf16(x):
    """fp32 -> bf16 by dropping the low 16 bits (a planted defect)."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()


# ------------------------------------------------------------------------------- bounds

def bound(r, a, kred, out, res=None):
    """The derived componentwise bounds (``out``: "f32", "bf16" or "res" for bf16(bf16(C) + r))."""
    acc = kred * E23 * a
    if out == "f32":
        return acc + 2.0 ** -24 * r.abs() + TINY
    if out == "bf16":
        return U8 * r.abs() + acc + TINY
    if out == "res":
        return U8 * r.abs() + U8 * (r + res.double()).abs() + acc + TINY
    raise ValueError(out)


def check(name, got, ref, bnd, errs):
    """Every element finite and |got - ref| <= bnd (``bnd = None``: equal as values, +-0 identified)."""
    got = got.double()
    if got.shape != ref.shape:
        errs.append(f"{name}: shape {tuple(got.shape)} != {tuple(ref.shape)}")
        return
    if not bool(torch.isfinite(got).all()):
        errs.append(f"{name}: {int((~torch.isfinite(got)).sum())} non-finite of {got.numel()}")
        return
    err = (got - ref).abs()
    if bnd is None:
        bad, score = err != 0, err
    else:
        bad, score = ~(err <= bnd), err / bnd
        print(f"{name}: worst |err| / bound {float(score.max()):.3f}")
    if bool(bad.any()):
        i = torch.argmax(torch.where(bad, score, torch.zeros_like(score)))
        idx = tuple(int(j) for j in torch.unravel_index(i, err.shape))
        what = "exact" if bnd is None else f"bound {float(bnd[idx]):.4g} exceeded {float(score[idx]):.3g}x"
        errs.append(f"{name}: {int(bad.sum())} of {got.numel()} wrong ({what}); worst at {idx}: got "
                    f"{float(got[idx]):.9g} ref {float(ref[idx]):.9g}")


def check_out(name, family, got, r, a, kred, out, errs, res=None):
    """One output against its family's criterion: the exact families equal, the others within the bound
    (``res``: the residual summand of a bf16(bf16(C) + r) epilogue; exact where |C + r| <= 256)."""
    ref = r if res is None else r + res.double()
    if family in EXACT:
        check(name, got, ref, None, errs)
    else:
        check(name, got, ref, bound(r, a, kred, "res" if res is not None else out, res), errs)


def check_colsums(name, family, shards, y, errs, squares=True):
    """Statistics shards ``[S, 2, N]`` (or ``[S, N]`` column partials with ``squares=False``) against
    float64 sums of the kernel's own stored output ``y [rows, N]``: rows 2^-23 sum|y| (and likewise
    for y^2); the ternary family, whose sums are integers below 2^24, must match exactly."""
    yd = y.double()
    rows = yd.shape[0]
    s = shards.double().sum(0)
    pairs = [("sum", s[0] if squares else s, yd.sum(0), yd.abs().sum(0))]
    if squares:
        pairs.append(("sumsq", s[1], (yd * yd).sum(0), (yd * yd).sum(0)))
    for what, got, ref, mag in pairs:
        if family == "ternary":
            assert float(mag.max()) < 2 ** 24, f"{name}: {what} magnitude {float(mag.max())} not below 2^24"
            check(f"{name} {what}", got, ref, None, errs)
        else:
            check(f"{name} {what}", got, ref, rows * E23 * mag + TINY, errs)


# ------------------------------------------------------------------------------- guard bands

_BITS16 = (torch.bfloat16, torch.float16)  # the 16-bit sentinel serves both (0x5A5A is 203.25 as fp16)


def guarded(rows, cols, ld, dtype, device, lead=1, fill=float("nan")):
    """A ``[rows, cols]`` view (row stride ``ld``) filled with NaN (``fill``) inside a buffer of sentinel bit
    patterns: ``lead`` whole rows before it, the columns ``cols .. ld`` of every row, one row after."""
    it = torch.int16 if dtype in _BITS16 else torch.int32
    sent = BF16_SENTINEL if dtype in _BITS16 else F32_SENTINEL
    buf = torch.full(((rows + lead + 1) * ld,), sent, dtype=it, device=device).view(dtype)
    view = buf[lead * ld:(lead + rows) * ld].view(rows, ld)[:, :cols]
    view.fill_(fill)
    return buf, view


def take_guarded(name, buf, view, errs):
    """The view's contents, after checking that every sentinel around it survived."""
    out = view.clone()
    it = torch.int16 if buf.dtype in _BITS16 else torch.int32
    sent = BF16_SENTINEL if buf.dtype in _BITS16 else F32_SENTINEL
    view.view(it).fill_(sent)
    broken = int((buf.view(it) != sent).sum())
    if broken:
        errs.append(f"{name}: {broken} guard elements overwritten")
    return out


# ------------------------------------------------------------------------------- planted defects

def defect(kind, acc, p, q, k0=32):
    """A float32 result ``acc = P Q^T`` with one planted defect, rounded to bf16 as a kernel would."""
    acc = acc.clone()
    if kind == "zero_row_segment":      # one output row of one 64-wide tile
        acc[5, 64:128] = 0
    elif kind == "missing_ktile":       # one 16x16 fragment without its last 32-deep k-tile
        acc[16:32, 32:48] -= p[16:32, -k0:].float() @ q[32:48, -k0:].float().t()
    elif kind == "transposed_fragment":
        acc[16:32, 32:48] = acc[16:32, 32:48].t().clone()
    elif kind == "truncation":
        return trunc_bf16(acc)
    elif kind == "duplicated_split":    # the first of 3 split-K pieces added twice in one tile
        kk = p.shape[1] // 3
        acc[0:64, 0:64] += p[0:64, :kk].float() @ q[0:64, :kk].float().t()
    else:
        raise ValueError(kind)
    return rn_bf16(acc)


def shifted_tap_conv(x, wt):
    """3x3 convolution whose tap (1, 2) reads one pixel too far on the image's right border (the
    wrap-around a missing column guard gives: the next row's first pixel instead of zero)."""
    n, c, h, w = x.shape
    p = im2col(x.float()).view(n, h, w, 9, c).clone()
    flat = x.float().permute(0, 2, 3, 1).reshape(n, h * w, c)
    nxt = torch.cat([flat[:, 1:], torch.zeros(n, 1, c)], 1).view(n, h, w, c)
    p[:, :, w - 1, 5] = nxt[:, :, w - 1]
    return p.view(n * h * w, 9 * c) @ taps(wt.float()).t()


# ------------------------------------------------------------------------------- the fast GELU

GELU_POLY_MAX = 3.0e38  # kGeluPolyMax of gelu_tanh.h: keeps 0 * (1 + 3 k1 x^2) finite once x^2 overflows


def _rcp(x):
    return 1.0 / x


def gelu_emulated(x, form, dtype=torch.bfloat16):
    """(gelu(x), gelu'(x)) as the EPI 1 epilogue of gemm_nt.hip / gelu_tanh.h evaluates and stores them
    (bf16), in float32 PyTorch (exp2 and the reciprocal are correctly rounded here, 1 ulp on the device).
    ``dtype``: the store's type (fp16: the fp16 instantiations of gelu.hip); ``None``: the unrounded
    float32 values (gelu.hip's backward multiplies the fp32 derivative and rounds only the product)."""
    def rn_bf16(v):  # the store
        return v if dtype is None else v.float().to(dtype)

    x = x.float()
    one, half = torch.tensor(1.0), torch.tensor(0.5)
    if form == "tanh":
        k0, k1, k3 = (torch.tensor(v, dtype=torch.float32) for v in (0.79788456080286536, 0.044715, 3 * 0.044715))
        u = k0 * x * (k1 * x * x + 1)
        t = one - 2 * _rcp(one + torch.exp2(torch.tensor(2.8853900817779268) * u))
        hx = half * x
        poly = torch.clamp(k3 * x * x + 1, max=GELU_POLY_MAX)
        return rn_bf16(hx * t + hx), rn_bf16(hx * (one - t * t) * (k0 * poly) + (half * t + half))
    a = [torch.tensor(v, dtype=torch.float32) for v in (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)]
    e = torch.exp2(torch.tensor(-0.72134752044448170) * x * x)
    t = _rcp(torch.tensor(0.3275911 * 0.70710678118654752, dtype=torch.float32) * x.abs() + 1)
    poly = t * (t * (t * (t * (t * a[4] + a[3]) + a[2]) + a[1]) + a[0])
    tail = half * poly * e
    cdf = torch.where(x >= 0, one - tail, tail)
    return rn_bf16(x * cdf), rn_bf16(x * torch.tensor(0.39894228040143268) * e + cdf)


def gelu_exact(x, form):
    """float64 gelu and gelu' of the selected form."""
    x = x.double()
    if form == "tanh":
        k0 = 0.7978845608028654
        t = torch.tanh(k0 * (x + 0.044715 * x ** 3))
        sech2 = 1 - t * t
        return 0.5 * x * (1 + t), 0.5 * (1 + t) + torch.where(sech2 == 0, torch.zeros_like(x),
                                                               0.5 * x * sech2 * k0 * (1 + 3 * 0.044715 * x * x))
    cdf = 0.5 * torch.erfc(-x * 0.7071067811865476)
    return x * cdf, cdf + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def all_finite_bf16():
    """All 65536 bf16 bit patterns as a [256, 256] matrix, the non-finite ones replaced by finite values
    (the pattern with the exponent field lowered by one)."""
    bits = torch.arange(65536, dtype=torch.int64)
    bits = torch.where((bits >> 7) & 0xFF == 0xFF, bits - 128, bits)
    bits = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16)
    return bits.view(torch.bfloat16).reshape(256, 256)


def gelu_bound(ref, c):
    return c * (U8 * ref.abs() + 2.0 ** -24)
