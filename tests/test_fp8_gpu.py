"""``csrc/kernels/fp8_quant.hip`` bit for bit against torch's CPU float8 casts, ``gemm_fp8.hip`` against float64 of
the dequantised operands (exact families exact: the operand layout of the 128-deep MFMA, the swizzle, the edges),
``fp8_linear`` against ``fp8_linear_reference`` in both scaling modes, and the model switch."""
import pytest
import torch

from fluxmpi_amd.ops import fp8
from tests import mfma_edges as me

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIRS = [(fp8.E4M3, fp8.E4M3), (fp8.E5M2, fp8.E4M3)]
# v_mfma_f32_16x16x128_f8f6f4 sums its 128 products with less than fp32 precision. Measured on MI355X over
# test_gemm's cases, against float64 of the dequantised operands: worst |err| / ``bound(r, a, K, "bf16")`` 8.24
# (cancel) and 6.40 (uniform), both at K = 16. The error follows the largest product, not the number of terms
# (worst |err| / a: cancel 1.6e-4 at K = 16, 2.6e-5 at K = 400), so the K-proportional term K 2^-23 a is short
# only where K is small: once the output rounding 2^-8 |r| is charged it has to be multiplied by 21.2 at K = 16
# (uniform; cancel 9.6) and by 0.21 at K >= 128, one full instruction's depth. So the derived bound stands as it
# is from K = 128 on, and below that the accumulation term is widened to twice the measured multiplier (the
# cases sample the inputs). The exact families stay exact.
ACC_WIDEN, ACC_WIDEN_BELOW = 42.5, 128


def fp8_bound(r, a, k):
    widen = ACC_WIDEN if k < ACC_WIDEN_BELOW else 1.0
    return me.bound(r, a, k, "bf16") + (widen - 1) * k * me.E23 * a


def bits(t):
    return t.cpu().view(torch.uint8)


def words(block):
    return [int(v) & 0xFFFFFFFF for v in block.cpu().tolist()]


def f32_bits(v):
    return int(torch.tensor(v, dtype=torch.float32).view(torch.int32)) & 0xFFFFFFFF


def quant_input(kind, r, c, fmt):
    g = torch.Generator().manual_seed(r * 1000 + c)
    if kind == "zeros":
        return torch.zeros(r, c).bfloat16()
    if kind == "ties":  # every finite bf16 value of the binades the format spans below amax (ties, subnormals, zero)
        span = 22 if fmt == fp8.E4M3 else 36
        i = torch.arange(r * c, dtype=torch.int64) % (span * 256)
        b = ((i % 2) << 15) | ((128 - span + i // 256) << 7) | ((i // 2) % 128)
        return torch.where(b >= 32768, b - 65536, b).to(torch.int16).view(torch.bfloat16).view(r, c)
    x = (2.0 ** (torch.rand(r, c, generator=g) * 6 - 3)) * (torch.randint(0, 2, (r, c), generator=g) * 2 - 1)
    if kind == "pow2":  # amax is exactly 8: the binade's lower edge
        x = x.clamp(-7.5, 7.5)
        x[-1, -1] = -8.0
    return x.bfloat16()


@pytest.mark.parametrize("kind", ["binades", "pow2", "ties", "zeros"])
@pytest.mark.parametrize("shape", [(1, 16, 16), (17, 48, 48), (130, 144, 144), (300, 400, 400), (130, 144, 152),
                                   (130, 136, 136)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("transpose", [False, True], ids=["rows", "rows+t"])
@pytest.mark.parametrize("fmt", [fp8.E4M3, fp8.E5M2])
def test_quantize(gpu_ext, fmt, transpose, shape, kind):
    """Current scaling (amax pass, scale update, cast) into guarded outputs; ``shape`` = (R, C, input row stride).
    C = 136: the row-major image's rows are written up to 144 with zeros."""
    r, c, ld = shape
    x = quant_input(kind, r, c, fmt)
    xd = torch.zeros(r, ld, dtype=torch.bfloat16, device=DEV)[:, :c].copy_(x)
    want, s = fp8.quantize_reference(x, fmt)
    assert s == fp8.pow2_scale(float(x.float().abs().max()), fmt) and (s != 1.0 or kind == "zeros")
    errs = []
    blk = torch.zeros(8, dtype=torch.int32, device=DEV)
    fp8.quantize_into(xd, fmt, blk)
    assert words(blk)[2] == f32_bits(float(x.float().abs().max()))
    fp8.scale_update(blk, fmt)
    assert words(blk)[:4] == [f32_bits(s), f32_bits(1 / s), 0, f32_bits(float(x.float().abs().max()))]
    rp, cp = -(-r // 16) * 16, -(-c // 16) * 16
    qb, q = me.guarded(r, cp, cp + 16, torch.uint8, DEV, fill=0x33)
    tb, qt = me.guarded(c, rp, rp + 16, torch.uint8, DEV, fill=0x33) if transpose else (None, None)
    fp8.quantize_into(xd, fmt, blk, q, qt, amax=False)
    assert words(blk)[2] == 0
    got = me.take_guarded("q", qb, q, errs).cpu()
    assert torch.equal(got[:, :c], bits(want)), f"{int((got[:, :c] != bits(want)).sum())} of {r * c} bytes differ"
    assert not bool(got[:, c:].any())
    if transpose:
        got_t = me.take_guarded("q_t", tb, qt, errs).cpu()
        assert torch.equal(got_t[:, :r], bits(want).t()) and not bool(got_t[:, r:].any())
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("fmt", [fp8.E4M3, fp8.E5M2])
def test_quantize_stored_scale(gpu_ext, fmt):
    """With a block (delayed scaling): the cast uses the stored scale, an outgrown one saturates at +-FMAX, the amax
    is this tensor's; a NaN and an inf stay non-finite and make the amax non-finite (scale 1)."""
    x = quant_input("binades", 17, 48, fmt)
    blk = fp8.new_block(DEV, 2.0 ** 40)
    t = fp8.quantize(x.to(DEV), fmt, blk, transpose=True)
    want, _ = fp8.quantize_reference(x, fmt, 2.0 ** 40)
    assert torch.equal(bits(t.q), bits(want)) and torch.equal(bits(t.q_t)[:, :17], bits(want).t())
    assert float(want.float().abs().min()) == fp8.FMAX[fmt]
    assert words(blk)[2] == f32_bits(float(x.float().abs().max()))
    fp8.scale_update(blk, fmt)
    assert words(blk)[0] == f32_bits(fp8.pow2_scale(float(x.float().abs().max()), fmt))
    x[3, 5], x[7, 20] = float("nan"), float("-inf")
    t = fp8.quantize(x.to(DEV), fmt)
    got = t.q.cpu().view(fp8.TORCH_DTYPE[fmt]).float()
    want, s = fp8.quantize_reference(x, fmt)
    assert s == 1.0 and words(t.block)[0] == f32_bits(1.0) and words(t.block)[3] >= 0x7F800000
    assert not torch.isfinite(got[3, 5]) and not torch.isfinite(got[7, 20])
    fin = torch.isfinite(x.float())
    assert torch.equal(bits(t.q)[fin], bits(want)[fin])


def gather_q(n, k):
    """The gather family's other operand for fp8: ``patterns`` spans all of bf16's binades, of which one per-tensor
    scale keeps the top 17 and flushes the rest to zero (and a zero hides a dropped term). Instead every
    non-zero finite e4m3 bit pattern (126 magnitudes, both signs, subnormals included) in a scrambled order, an
    eighth as large so that the scale is not 1: each survives the cast and is exact in bf16."""
    i = (torch.arange(n * k, dtype=torch.int64) * 101 + 37) % 252
    byte = 1 + i % 126 + 128 * (i // 126)
    return (byte.to(torch.uint8).view(torch.float8_e4m3fn).float() * 0.125).bfloat16().view(n, k)


def operand(t, fmt):
    """The CPU reference quantiser's image of ``t`` on the device, and its float64 values."""
    q, s = fp8.quantize_reference(t, fmt)
    return fp8.Fp8Tensor(bits(q).to(DEV), None, fp8.new_block(DEV, s), fmt), q.double() / s


@pytest.mark.parametrize("shape", [(m, n, k) for m in (1, 127, 129, 300) for n in (8, 136) for k in (16, 128, 144, 400)]
                         + [(256, 256, 256)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "x".join(p))
def test_gemm(gpu_ext, pair, shape):
    """Every family, bias off and on, into a guarded output. ternary and gather are exact (integer sums <= 256;
    gather's bias is zero, a bit pattern plus a bias is not exact); uniform and cancel are held to
    ``bound(r, a, K, "bf16")``: fp8 products are exact in fp32, the bound charges the accumulation and the one
    rounding, with the accumulation term widened as measured (``ACC_WIDEN``)."""
    m, n, k = shape
    errs = []
    for family in me.FAMILIES:
        p, q = me.gemm_inputs(family, m, n, k)
        q = gather_q(n, k) if family == "gather" else q
        (a, ad), (b, bd) = operand(p, pair[0]), operand(q, pair[1])
        r, mag = me.ref_gemm(ad, bd)
        g = torch.Generator().manual_seed(m + n + k)
        bias = {"ternary": torch.randint(-2, 3, (n,), generator=g).float(), "gather": torch.zeros(n)}.get(
            family, torch.rand(n, generator=g) * 2 - 1).bfloat16()
        for with_bias in (False, True):
            ref, amag = (r + bias.double(), mag + bias.double().abs()) if with_bias else (r, mag)
            if family == "ternary":
                assert float(ref.abs().max()) <= 256
            buf, view = me.guarded(m, n, n + 8, torch.bfloat16, DEV)
            fp8.gemm_into(view, a, b, bias.to(DEV) if with_bias else None)
            name = f"{family} bias={with_bias}"
            me.check(name, me.take_guarded(name, buf, view, errs).cpu(), ref,
                     None if family in me.EXACT else fp8_bound(ref, amag, k), errs)
    assert not errs, "\n".join(errs)


def linear_data(rows, n_in, n_out, seed=0):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    return [t.bfloat16() for t in (u(rows, n_in), u(n_out, n_in) * n_in ** -0.5, u(n_out), u(rows, n_out))]


def step(fn, x, w, b, dy):
    """(y, dx, dW, db) of one forward + backward of ``fn(x, w, b)`` on fresh device leaves."""
    x, w, b = (t.to(DEV).requires_grad_() for t in (x, w, b))
    y = fn(x, w, b)
    y.backward(dy.to(DEV))
    return y.detach(), x.grad, w.grad, b.grad


def check_linear(name, y, dx, ref, n_in, n_out, errs):
    yr, dxr, ya, dxa = ref
    me.check(f"{name} y", y.cpu(), yr, fp8_bound(yr, ya, n_in), errs)
    me.check(f"{name} dx", dx.cpu(), dxr, fp8_bound(dxr, dxa, n_out), errs)


@pytest.mark.parametrize("shape", [(130, 144, 136), (1024, 256, 256)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("scaling", ["current", "delayed"])
def test_fp8_linear(gpu_ext, monkeypatch, scaling, shape):
    """y and dx within the GEMM's bound of the float64 reference on the same quantisation; dW and db are the bf16
    kernels' (``ops.linear.linear`` with its one-launch ``linbwd.hip`` backward off, i.e. its separate weight-gradient
    and column-sum calls, which are what the fp8 backward runs) bit for bit. Delayed: step 1 casts
    with scale 1, step 2 (other data) with step 1's amax. One inf in dy: a non-finite dx."""
    from fluxmpi_amd.ops import linear as L
    monkeypatch.setattr(L, "LINBWD", False)
    rows, n_in, n_out = shape
    x, w, b, dy = linear_data(rows, n_in, n_out)
    errs = []
    state = fp8.Fp8State(scaling)
    y, dx, dw, db = step(lambda *a: fp8.fp8_linear(*a, state=state), x, w, b, dy)
    _, _, dw_ref, db_ref = step(L.linear, x, w, b, dy)
    assert torch.equal(dw, dw_ref) and torch.equal(db, db_ref)
    check_linear("step 1", y, dx, fp8.fp8_linear_reference(x, w, b, dy, (1.0,) * 3 if scaling == "delayed" else None),
                 n_in, n_out, errs)
    if scaling == "delayed":
        x2, _, _, dy2 = linear_data(rows, n_in, n_out, seed=1)
        x2, dy2 = x2 * 4, dy2 * 0.125
        y, dx, _, _ = step(lambda *a: fp8.fp8_linear(*a, state=state), x2, w, b, dy2)
        scales = tuple(fp8.pow2_scale(float(t.float().abs().max()), f) for t, f in
                       ((x, fp8.E4M3), (w, fp8.E4M3), (dy, fp8.E5M2)))
        check_linear("step 2", y, dx, fp8.fp8_linear_reference(x2, w, b, dy2, scales), n_in, n_out, errs)
    dy[5, 7] = float("inf")
    assert not bool(torch.isfinite(step(fp8.fp8_linear, x, w, b, dy)[1]).all())
    assert not errs, "\n".join(errs)


def test_delayed_graph(gpu_ext):
    """Two delayed-scaling steps captured into one HIP graph (W is cast in each, with the amax before): every replay's
    step 2 equals the eager step 2 bit for bit (it depends on step 1's amax alone: history length 1)."""
    rows, n_in, n_out = 130, 144, 136
    data = [linear_data(rows, n_in, n_out, seed=s) for s in (0, 1)]
    data[1][0], data[1][3] = data[1][0] * 4, data[1][3] * 0.125

    def two_steps(lin, xs, dys):
        out = []
        for x, dy in zip(xs, dys):
            lin.weight.grad = lin.bias.grad = x.grad = None
            y = lin(x)
            y.backward(dy)
            out = [y.detach(), x.grad, lin.weight.grad, lin.bias.grad]
        return out

    def module():
        lin = fp8.Fp8Linear(n_in, n_out, scaling="delayed").to(DEV).bfloat16()
        with torch.no_grad():
            lin.weight.copy_(data[0][1]), lin.bias.copy_(data[0][2])
        return lin

    xs = [d[0].to(DEV).requires_grad_() for d in data]
    dys = [d[3].to(DEV) for d in data]
    eager = [t.clone() for t in two_steps(module(), xs, dys)]
    lin = module()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = two_steps(lin, xs, dys)
    for replay in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for name, a, e in zip(("y", "dx", "dW", "db"), got, eager):
            assert torch.equal(a, e), f"replay {replay}: {name} differs from the eager step"


@pytest.mark.parametrize("scaling", ["current", "delayed"])
def test_after_optimizer_step(gpu_ext, scaling):
    """The fused optimisers write the weight through raw pointers (``weight._version`` does not move): the step
    after a fused Adam update must run on the updated weight, forward and input gradient."""
    from fluxmpi_amd.ops import optim as fused
    rows, n_in, n_out = 130, 144, 136
    x, w, b, dy = linear_data(rows, n_in, n_out)
    lin = fp8.Fp8Linear(n_in, n_out, scaling=scaling).to(DEV).bfloat16()
    with torch.no_grad():
        lin.weight.copy_(w), lin.bias.copy_(b)
    xd, dyd = x.to(DEV).requires_grad_(), dy.to(DEV)
    lin(xd).backward(dyd)
    ps = [lin.weight, lin.bias]
    version = lin.weight._version
    fused.adam_([p.detach() for p in ps], [p.grad for p in ps], [torch.zeros_like(p) for p in ps],
                [torch.zeros_like(p) for p in ps], lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8, bc1=0.1, bc2=0.001)
    w2, b2 = lin.weight.detach().cpu(), lin.bias.detach().cpu()
    assert lin.weight._version == version and float((w2.float() - w.float()).abs().max()) > 0.02
    xd.grad = None
    y = lin(xd)
    y.backward(dyd)
    scales = None if scaling == "current" else tuple(
        fp8.pow2_scale(float(t.float().abs().max()), f) for t, f in ((x, fp8.E4M3), (w, fp8.E4M3), (dy, fp8.E5M2)))
    errs = []
    check_linear("after the update", y.detach(), xd.grad, fp8.fp8_linear_reference(x, w2, b2, dy, scales), n_in, n_out, errs)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("case", ["fp16", "n_in=100"])
def test_fallback(gpu_ext, case):
    x, w, b, dy = linear_data(130, 100 if case == "n_in=100" else 144, 136)
    if case == "fp16":
        x, w, b, dy = (t.half() for t in (x, w, b, dy))
    from fluxmpi_amd.ops.linear import linear
    assert not fp8.supported(x.to(DEV), w.to(DEV).requires_grad_())
    for got, want in zip(step(fp8.fp8_linear, x, w, b, dy), step(linear, x, w, b, dy)):
        assert torch.equal(got, want)


def test_vit(gpu_ext, monkeypatch):
    from fluxmpi_amd.models.vit import vit_tiny
    from fluxmpi_amd.ops.linear import Linear
    monkeypatch.delenv("FLUXMPI_FP8", raising=False)
    models = {}
    for name, kw in (("default", {}), ("off", {"fp8": False}), ("fp8", {"fp8": True})):
        torch.manual_seed(5)
        models[name] = vit_tiny(**kw).to(DEV).bfloat16()
    assert all(type(blk.qkv) is Linear for blk in models["default"].blocks)
    assert all(type(blk.qkv) is fp8.Fp8Linear for blk in models["fp8"].blocks)
    shapes = {k: v.shape for k, v in models["default"].state_dict().items()}
    assert {k: v.shape for k, v in models["fp8"].state_dict().items()} == shapes
    x = torch.randn(5, 3, 32, 32, generator=torch.Generator().manual_seed(6)).bfloat16().to(DEV)
    assert torch.equal(models["default"](x), models["off"](x))
    y = models["fp8"](x)
    y.float().square().sum().backward()
    assert bool(torch.isfinite(y).all())
    for k, p in models["fp8"].named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
