"""The K-group variants (variant bit 3: 8, 32-deep K-steps / 4 stages; 10, 64-deep / 2 stages) of
gemm_glds.hip's weight-gradient kernel, through the raw launcher (fp32 slabs) plus the split-K
reduce, in every B mode: plain, implicit 3x3, stride-2 1x1 gather, stride-2 3x3.

Reference: float64 from the same bf16 operands. Bound per element: (K + splits + 2) * 2^-24 *
sum_k |a_k b_k| — the first-order fp32 bound of a sum of K terms in any order (K - 1 additions of
relative error 2^-24 each; the products of two bf16 values are exact in fp32), with the splits' and
the K-groups' extra additions and the reduce's counted in. Integer operands in [-4, 4] keep every
partial sum below 2^24, hence exact: those cases require equality. Two launches must agree bit for
bit, and the variant stays within the sum of both bounds of variant 2 (the parent kernel).

Guards: operands are views inside NaN-filled buffers (row stride = lda / ldb; whole NaN rows or
images before and after; the never-read odd pixels of a stride-2 1x1 input are NaN too), the slabs
are NaN-prefilled between two canary slabs: an out-of-operand read that reaches an accumulator, a
slab element left unwritten or a slab count that differs from the Python helper's shows as a value,
not as a fault.
"""
import pytest
import torch

gpu = pytest.mark.gpu
VARIANTS = [8, 10]
PARENT = 2
U = 2.0 ** -24
CANARY = 7.0
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _values(shape, exact, seed):
    g = torch.Generator().manual_seed(seed)
    if exact:
        return torch.randint(-4, 5, shape, generator=g).to(torch.bfloat16)
    return (torch.rand(shape, generator=g) * 2 - 1).to(torch.bfloat16)


def _rows_view(vals):
    """[K, cols] values as a view inside a NaN buffer: one NaN row above and below, 8 NaN columns on
    both sides. Returns (buffer, view, row stride)."""
    k, cols = vals.shape
    buf = torch.full((k + 2, cols + 16), float("nan"), dtype=torch.bfloat16, device="cuda")
    view = buf[1:k + 1, 8:8 + cols]
    view.copy_(vals)
    return buf, view, cols + 16


def _image_view(vals):
    """[n, H, W, C] values (dense: the implicit im2col takes ldb = C) between two NaN images."""
    n = vals.shape[0]
    buf = torch.full((n + 2, *vals.shape[1:]), float("nan"), dtype=torch.bfloat16, device="cuda")
    view = buf[1:n + 1]
    view.copy_(vals)
    return buf, view


def _im2col(x, stride):
    """[n, H, W, C] -> [n * Ho * Wo, 9 * C] in float64 (column = tap * C + ci, zero padding 1)."""
    n, h, w, c = x.shape
    xp = torch.zeros(n, h + 2, w + 2, c, dtype=torch.float64, device=x.device)
    xp[:, 1:h + 1, 1:w + 1] = x.double()
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    taps = [xp[:, r:r + stride * (ho - 1) + 1:stride, s:s + stride * (wo - 1) + 1:stride] for r in range(3) for s in range(3)]
    return torch.stack(taps, dim=3).reshape(n * ho * wo, 9 * c)


def _launch(C, variant, a, lda, b, ldb, M, N, K, splits, conv=(0, 0, 0), b_sub=0):
    """gemm_wgrad into NaN slabs between canaries, then the reduce; returns dW [M, N] fp32."""
    from fluxmpi_amd.ops import gemm as G
    from fluxmpi_amd.ops.multi_tensor import DTYPE_CODE
    sp = G._actual_splits_v2(K, splits)
    ws = torch.full((sp + 2, M * N), float("nan"), dtype=torch.float32, device="cuda")
    ws[0] = CANARY
    ws[sp + 1] = CANARY
    s = torch.cuda.current_stream().cuda_stream
    C.gemm_wgrad(a.data_ptr(), b.data_ptr(), ws[1].data_ptr(), lda, ldb, M, N, K, sp, conv[0], conv[1], conv[2], s,
                 variant, b_sub)
    out = torch.empty(M, N, dtype=torch.float32, device="cuda")
    C.gemm_splitk_reduce(ws[1].data_ptr(), sp, M * N, out.data_ptr(), DTYPE_CODE[torch.float32], s)
    torch.cuda.synchronize()
    assert bool((ws[0] == CANARY).all()) and bool((ws[sp + 1] == CANARY).all()), "a store outside the slabs"
    return out


def _check(tag, C, variant, errs, a, lda, b, ldb, a64, b64, M, N, K, splits, exact, conv=(0, 0, 0), b_sub=0):
    """a64 [K, M], b64 [K, N]: the float64 operands the launch must multiply."""
    ref = a64.t() @ b64
    tag = f"v{variant} {tag}"
    out = _launch(C, variant, a, lda, b, ldb, M, N, K, splits, conv, b_sub)
    if not bool(torch.isfinite(out).all()):
        errs.append(f"{tag}: non-finite output (a guard value reached it, or a slab element was not written)")
        return
    if exact:
        if not torch.equal(out.double(), ref):
            errs.append(f"{tag}: exact case differs, max |d| = {float((out.double() - ref).abs().max())}")
        return
    bound = (K + splits + 2) * U * (a64.abs().t() @ b64.abs())
    over = ((out.double() - ref).abs() - bound).max()
    if float(over) > 0:
        errs.append(f"{tag}: error exceeds the bound by {float(over):.3e}")
    again = _launch(C, variant, a, lda, b, ldb, M, N, K, splits, conv, b_sub)
    if not torch.equal(out, again):
        errs.append(f"{tag}: two launches differ")
    parent = _launch(C, PARENT, a, lda, b, ldb, M, N, K, splits, conv, b_sub)
    over = ((out.double() - parent.double()).abs() - 2 * bound).max()
    if not float(over) <= 0:
        errs.append(f"{tag}: differs from variant 2 by more than both bounds ({float(over):.3e} over)")


def _done(errs):
    assert not errs, f"{len(errs)} failures:\n" + "\n".join(errs[:20])


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("splits", [1, 2, 3, 7])
def test_plain(gpu_ext, splits, exact, variant):
    """K < kBK (8), an empty second group (8, 40 at several splits), a ragged last step (40, 264,
    1000), edge tiles in M and N (72, 136), the 64-wide tile forms, and one to three N tiles."""
    errs = []
    for K in (8, 40, 264, 1000):
        for M in (64, 72, 128, 136):
            def make_a(K=K, M=M):
                return _rows_view(_values((K, M), exact, 1000 * K + M).cuda())
            abuf, a, lda = _cached(("a", K, M, exact), make_a)
            for N in (64, 72, 128, 136, 264):
                def make_b(K=K, N=N):
                    return _rows_view(_values((K, N), exact, 7 + 1000 * K + N).cuda())
                bbuf, b, ldb = _cached(("b", K, N, exact), make_b)
                _check(f"plain M{M} N{N} K{K} s{splits}", gpu_ext, variant, errs, a, lda, b, ldb, a.double(), b.double(),
                       M, N, K, splits, exact)
    _done(errs)


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (5, 7)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_conv3x3(gpu_ext, hw, exact, variant):
    """Implicit 3x3 / s1 / p1 B (C = 16, N = 144) over 2 and 3 distinct images; at 5x7 the split
    (k = 64) and K-group (k = 32, 64) boundaries fall inside an image."""
    h, w = hw
    c, N = 16, 144
    errs = []
    for n in (2, 3):
        K = n * h * w
        xbuf, x = _image_view(_values((n, h, w, c), exact, 31 * K + 1).cuda())
        b64 = _im2col(x, 1)
        for M in (64, 136):
            abuf, a, lda = _rows_view(_values((K, M), exact, 31 * K + M).cuda())
            for splits in (1, 2, 3):
                _check(f"3x3 {n}x{h}x{w} M{M} s{splits}", gpu_ext, variant, errs, a, lda, x, c, a.double(), b64, M, N, K, splits,
                       exact, conv=(h, w, c))
    _done(errs)


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("hw", [(5, 7), (6, 4)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_conv3x3_stride2(gpu_ext, hw, exact, variant):
    """Implicit 3x3 / s2 / p1 B over the output grid (odd and even H, W); 7 images put the split and
    K-group boundaries inside an image."""
    h, w = hw
    ho, wo = (h + 1) // 2, (w + 1) // 2
    c, N = 16, 144
    errs = []
    for n in (2, 7):
        K = n * ho * wo
        xbuf, x = _image_view(_values((n, h, w, c), exact, 37 * K + 1).cuda())
        b64 = _im2col(x, 2)
        for M in (64, 136):
            abuf, a, lda = _rows_view(_values((K, M), exact, 37 * K + M).cuda())
            for splits in (1, 2, 3):
                _check(f"3x3s2 {n}x{h}x{w} M{M} s{splits}", gpu_ext, variant, errs, a, lda, x, c, a.double(), b64, M, N, K, splits,
                       exact, conv=(h, w, c), b_sub=1)
    _done(errs)


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("hw", [(5, 7), (6, 4)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_conv1x1_stride2(gpu_ext, hw, exact, variant):
    """The stride-2 1x1 gather: B row (img, ho, wo) is input pixel (img, 2ho, 2wo); the pixels it
    skips and the columns past N are NaN."""
    h, w = hw
    ho, wo = (h + 1) // 2, (w + 1) // 2
    errs = []
    for n in (2, 7):
        K = n * ho * wo
        for N in (72, 128):
            ldb = N + 8
            vals = _values((n, ho, wo, N), exact, 41 * K + N).cuda()
            xbuf = torch.full((n + 2, h, w, ldb), float("nan"), dtype=torch.bfloat16, device="cuda")
            x = xbuf[1:n + 1]
            x[:, ::2, ::2, :N] = vals
            b64 = vals.double().reshape(K, N)
            for M in (64, 136):
                abuf, a, lda = _rows_view(_values((K, M), exact, 41 * K + M).cuda())
                for splits in (1, 2, 3):
                    _check(f"1x1s2 {n}x{h}x{w} M{M} N{N} s{splits}", gpu_ext, variant, errs, a, lda, x, ldb, a.double(), b64, M, N, K,
                           splits, exact, conv=(h, w, 0), b_sub=1)
    _done(errs)
