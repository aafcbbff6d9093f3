"""``mx6_quant.hip`` bit for bit against ``mx_quantize_reference`` for e2m3 and e3m2; ``mx6_gemm.hip`` exactly on operands
built on the fp6 grids (one nonzero per row at every K position under per-block scales: the operand and scale layout
of the scaled MFMA) and within ``tests.test_mx_gpu.mx_bound`` of float64 on the dequantised operands;
``Fp8Linear(scaling="mx", fwd="e2m3")`` against ``mx_linear_reference``."""
import pytest
import torch

from fluxmpi_amd.ops import fp8
from tests import mfma_edges as me
from tests.test_fp8_gpu import linear_data, step
from tests.test_mx4 import block_input
from tests.test_mx6 import FORMATS, ties
from tests.test_mx_gpu import gemm_family, mx_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIRS = [(fp8.E2M3, fp8.E2M3), (fp8.E3M2, fp8.E2M3)]
SHAPES = [(1, 8, 32), (16, 16, 128), (16, 16, 256), (144, 136, 160), (130, 72, 416)]
WRAP = (130, 72, fp8.MX6_STAGE_K * (2 * fp8.MX6_STAGES + 1))  # five stages of 128: the LDS ring wraps twice
ids = lambda s: "x".join(map(str, s))
pad16 = lambda n: -(-n // 16) * 16


@pytest.mark.parametrize("shape", [(32, 32), (128, 128), (160, 416), (32, 544)], ids=ids)
@pytest.mark.parametrize("fmt", FORMATS)
def test_mx6_quantize(gpu_ext, fmt, shape):
    """One launch, strided input, both images into sentinel-filled guarded buffers (rows of 3 C / 4 bytes in strides
    that are multiples of 16); the tie family, a zero block and a non-finite block of each image planted."""
    r, c = shape
    x = block_input(r, c, seed=r + c)
    x[2, :31], x[2, 31] = 4 * ties(fmt)[0], -4 * fp8.FMAX[fmt]   # row 2: every tie under the scale 1 / 4
    x[1, :32], x[:32, 9] = 0.0, 0.0                              # a zero block of each image (row 2 loses one tie)
    x[r - 1, c - 3], x[5, 17] = float("inf"), float("nan")
    xd = torch.zeros(r, c + 8, dtype=torch.bfloat16, device=DEV)[:, :c].copy_(x)
    sc, errs = fp8.mx_scale_cols, []
    qc, tc = 3 * c // 4, 3 * r // 4
    out = [me.guarded(*s, torch.uint8, DEV, fill=0x33) for s in
           ((r, qc, pad16(qc) + 16), (r, sc(c), sc(c) + 4), (c, tc, pad16(tc) + 16), (c, sc(r), sc(r) + 4))]
    fp8.mx_quantize_into(xd, fmt, *(v for _, v in out))
    q, s, q_t, s_t = (me.take_guarded(str(i), *o, errs).cpu() for i, o in enumerate(out))
    for src, gq, gs in ((x, q, s), (x.t().contiguous(), q_t, s_t)):
        want, by = fp8.mx_quantize_reference(src, fmt)
        assert torch.equal(gq, fp8.mx_pack_fp6(want, fmt)), f"{int((gq != fp8.mx_pack_fp6(want, fmt)).sum())} bytes differ"
        assert torch.equal(gs, fp8.mx_scale_image(by)), f"{int((gs != fp8.mx_scale_image(by)).sum())} scale bytes differ"
        assert int((by == 255).sum()) >= 2 and int((by == 127).sum()) >= 1
    assert not errs, "\n".join(errs)


def image(v, by, fmt):
    """Grid values ``v`` with block bytes ``by`` as a device operand (the scale rows' padding poisoned with 255, the
    rows' padding up to 16 bytes with 0xFF), and its float64 values."""
    q = fp8.mx_pack_fp6(v.to(DEV), fmt)
    q._base[:, q.shape[1]:] = 0xFF
    img = fp8.mx_scale_image(by)
    img[:, by.shape[1]:] = 255
    return fp8.MxTensor(q, img.to(DEV), None, None, fmt), fp8.mx_dequantize(v, by)


def operand(t, fmt):
    q, by = fp8.mx_quantize_reference(t, fmt)
    return image(q.float(), by, fmt)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("pair", PAIRS, ids=ids)
def test_mx6_gemm_exact(gpu_ext, pair, shape):
    """One-hot: row i of A and row j of B hold one value each, at K position (i + off) % K and (j + off) % K, every
    position below 256 in turn, with block kb of A at 2^kb and of B at 2^(2 kb): C is diagonal and C[i, i] names the
    position's value in each operand (the 31 nonzero magnitudes in turn) and its block in each scale image. Then the
    ternary families of the fp8 test, which both grids hold exactly."""
    m, n, k = shape
    kb = torch.arange(k // 32)
    errs = []
    for off in range(0, min(k, 256), min(m, n)):
        ops = []
        for rows, sign, by, fmt in ((m, 1, 127 + kb, pair[0]), (n, -1, 127 + 2 * kb, pair[1])):
            pos = (torch.arange(rows) + off) % k
            vals = sign * fp8.fp6_grid(fmt)[1:].float()[pos % 31 if sign > 0 else 30 - pos % 31]
            v = torch.zeros(rows, k).scatter_(1, pos.view(-1, 1), vals.view(-1, 1))
            ops.append(image(v, by.to(torch.uint8).expand(rows, -1).contiguous(), fmt))
        (a, ad), (b, bd) = ops
        ref = ad @ bd.t()
        assert int((ref != 0).sum()) >= min(m, n) and torch.equal(ref, ref.bfloat16().double())
        buf, view = me.guarded(m, n, n + 8, torch.bfloat16, DEV)
        fp8.mx_gemm_into(view, a, b)
        me.check(f"one-hot {off}", me.take_guarded("one-hot", buf, view, errs).cpu(), ref, None, errs)
    for family in ("one_block", "balanced"):
        p, q = gemm_family(family, m, n, k)
        (a, ad), (b, bd) = operand(p, pair[0]), operand(q, pair[1])
        assert torch.equal(ad, p.double()) and torch.equal(bd, q.double())
        buf, view = me.guarded(m, n, n + 8, torch.bfloat16, DEV)
        fp8.mx_gemm_into(view, a, b)
        me.check(family, me.take_guarded(family, buf, view, errs).cpu(), me.ref_gemm(ad, bd)[0], None, errs)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("shape", SHAPES + [WRAP], ids=ids)
@pytest.mark.parametrize("pair", PAIRS, ids=ids)
def test_mx6_gemm_bounded(gpu_ext, pair, shape):
    """Random operands through the reference quantiser against float64 of the DEQUANTISED operands (no quantisation
    error in the bound), no bias, a bf16 one and an fp32 one."""
    m, n, k = shape
    errs = []
    for family in ("uniform", "cancel"):
        p, q = gemm_family(family, m, n, k)
        (a, ad), (b, bd) = operand(p, pair[0]), operand(q, pair[1])
        r, mag = me.ref_gemm(ad, bd)
        bias = (torch.rand(n, generator=torch.Generator().manual_seed(m + n + k)) * 2 - 1).bfloat16()
        for bt in (None, bias, bias.float()):
            ref, amag = (r, mag) if bt is None else (r + bias.double(), mag + bias.double().abs())
            buf, view = me.guarded(m, n, n + 8, torch.bfloat16, DEV)
            fp8.mx_gemm_into(view, a, b, None if bt is None else bt.to(DEV))
            name = f"{family} bias={None if bt is None else bt.dtype}"
            me.check(name, me.take_guarded(name, buf, view, errs).cpu(), ref, mx_bound(ref, amag, k), errs)
    assert not errs, "\n".join(errs[:20])


def test_mx6_linear(gpu_ext):
    """y and dx within the GEMM's bound of the float64 reference on the same quantisation (dy in e3m2); dW and db are
    what fwd="e4m3" gives (the bf16 kernels either way); a width of 40 takes ``ops.linear.linear``."""
    from fluxmpi_amd.ops import linear as L
    x, w, b, dy = linear_data(64, 64, 96)
    lin = fp8.Fp8Linear(64, 96, scaling="mx", fwd="e2m3")
    assert fp8.mx_supported(x.to(DEV), w.to(DEV).requires_grad_())  # not the fallback
    y, dx, dw, db = step(lambda *a: fp8.fp8_linear(*a, state=lin.fp8), x, w, b, dy)
    _, _, dw8, db8 = step(lambda *a: fp8.fp8_linear(*a, state=fp8.Fp8State("mx")), x, w, b, dy)
    assert torch.equal(dw, dw8) and torch.equal(db, db8)
    yr, dxr, ya, dxa = fp8.mx_linear_reference(x, w, b, dy, fwd="e2m3")
    errs = []
    me.check("y", y.cpu(), yr, mx_bound(yr, ya, 64), errs)
    me.check("dx", dx.cpu(), dxr, mx_bound(dxr, dxa, 96), errs)
    assert not errs, "\n".join(errs)
    x, w, b, dy = linear_data(64, 40, 96)
    for got, want in zip(step(lambda *a: fp8.fp8_linear(*a, state=lin.fp8), x, w, b, dy), step(L.linear, x, w, b, dy)):
        assert torch.equal(got, want)
