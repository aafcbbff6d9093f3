"""``csrc/kernels/mx_quant.hip`` bit for bit against ``mx_quantize_reference`` (bytes and scale images), ``mx_gemm.hip``
against float64 of the dequantised operands (exact families exact: which scale byte reaches which row, K group and
tile of the scaled MFMA), ``Fp8Linear(scaling="mx")`` against ``mx_linear_reference``, and the model switch."""
import pytest
import torch

from fluxmpi_amd.ops import fp8
from tests import mfma_edges as me
from tests.test_fp8_gpu import linear_data, step
from tests.test_mx import KINDS, quant_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
# v_mfma_scale_f32_16x16x128_f8f6f4 sums with less than fp32 precision, as its unscaled form does. Measured on MI355X
# over test_mx_gemm's uniform and cancel cases (each K block of both operands times its own 2^-6 .. 2^6, so one MFMA
# sums products of different scales), against float64 of the dequantised operands, worst |err| /
# ``bound(r, a, K, "bf16")``: 3.33 (cancel) and 2.75 (uniform) at K = 32; 0.99 / 0.99 / 0.97 / 0.96 (uniform) at
# K = 128 / 160 / 256 / 416. The accumulation term K 2^-23 a alone has to be multiplied by 3.79 at K = 32 (uniform;
# cancel 3.42) and by 0.79 or less from K = 128 on. So the derived bound stands from K = 128 on, and below that the
# accumulation term is widened to twice the measured multiplier (the cases sample the inputs). The exact families
# stay exact.
ACC_WIDEN, ACC_WIDEN_BELOW = 7.6, 128


def mx_bound(r, a, k):
    widen = ACC_WIDEN if k < ACC_WIDEN_BELOW else 1.0
    return me.bound(r, a, k, "bf16") + (widen - 1) * k * me.E23 * a


def bits(t):
    return t.cpu().view(torch.uint8)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape, transpose", [((1, 32, 32), False), ((17, 96, 96), False), ((130, 160, 168), False),
                                              ((300, 416, 416), False), ((32, 32, 32), True), ((160, 96, 104), True),
                                              ((288, 416, 416), True)], ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else ("rows", "rows+t")[s])
@pytest.mark.parametrize("fmt", [fp8.E4M3, fp8.E5M2])
def test_mx_quantize(gpu_ext, fmt, shape, transpose, kind):
    """One launch into guarded images and guarded scale images; ``shape`` = (R, C, input row stride). Finite elements
    bit-equal, non-finite ones non-finite (their blocks store 127), scale rows padded with 127."""
    r, c, ld = shape
    x = quant_input(kind, r, c, fmt)
    xd = torch.zeros(r, ld, dtype=torch.bfloat16, device=DEV)[:, :c].copy_(x)
    errs, sc = [], fp8.mx_scale_cols
    out = {"q": me.guarded(r, c, c + 16, torch.uint8, DEV, fill=0x33), "s": me.guarded(r, sc(c), sc(c) + 4, torch.uint8, DEV, fill=0x33)}
    if transpose:
        out["q_t"] = me.guarded(c, r, r + 16, torch.uint8, DEV, fill=0x33)
        out["s_t"] = me.guarded(c, sc(r), sc(r) + 4, torch.uint8, DEV, fill=0x33)
    fp8.mx_quantize_into(xd, fmt, *(out[k][1] if k in out else None for k in ("q", "s", "q_t", "s_t")))
    got = {k: me.take_guarded(k, *v, errs).cpu() for k, v in out.items()}
    for src, qk, sk in ((x, "q", "s"),) + (((x.t().contiguous(), "q_t", "s_t"),) if transpose else ()):
        want, by = fp8.mx_quantize_reference(src, fmt)
        fin = torch.isfinite(src.float())
        assert torch.equal(got[qk][fin], bits(want)[fin]), f"{qk}: {int((got[qk] != bits(want))[fin].sum())} bytes differ"
        assert not bool(torch.isfinite(got[qk].view(fp8.TORCH_DTYPE[fmt]).float()[~fin]).any())
        assert torch.equal(got[sk], fp8.mx_scale_image(by)), f"{sk}: {int((got[sk] != fp8.mx_scale_image(by)).sum())} scale bytes differ"
        if kind == "nonfinite":
            assert bool((by.repeat_interleave(32, 1)[~fin] == 127).all())
    assert not errs, "\n".join(errs)


def operand(t, fmt):
    """The CPU reference quantiser's image of ``t`` on the device (the scale rows' padding poisoned with 255: the
    GEMM must not let it in), and its float64 values."""
    q, by = fp8.mx_quantize_reference(t, fmt)
    img = fp8.mx_scale_image(by)
    img[:, by.shape[1]:] = 255
    return fp8.MxTensor(bits(q).to(DEV), img.to(DEV), None, None, fmt), fp8.mx_dequantize(q, by)


def block_pow2(e):
    """``2^e [rows, blocks]`` spread over the 32 elements of each block."""
    return (2.0 ** e.float()).repeat_interleave(32, 1)


def gemm_family(family, m, n, k):
    """bf16 ``A [m, k]``, ``B [n, k]`` (module docstring of the issue's families; built before quantisation, which
    keeps power-of-two multiples of ternary values exactly)."""
    nb = k // 32
    i, j, kb = torch.arange(m).view(m, 1), torch.arange(n).view(n, 1), torch.arange(nb).view(1, nb)
    if family == "one_block":  # row i of A lives in K block i % nb alone, at 2^ea[i]; B at 2^eb[j, kb], all different
        p, q = me.gemm_inputs("ternary", m, n, k, nnz=k)
        p = p.float() * block_pow2(torch.where(kb == i % nb, (5 * i) % 17 - 8, -1000))
        return p.bfloat16(), (q.float() * block_pow2((3 * j + 5 * kb) % 23 - 11)).bfloat16()
    u = (kb * 24) // max(nb - 1, 1) - 12
    if family == "balanced":  # every product is +-2^(r[i] + c[j]): u[kb] goes up in A and down in B
        p, q = me.gemm_inputs("ternary", m, n, k)
        return (p.float() * block_pow2(u + i % 5 - 2)).bfloat16(), (q.float() * block_pow2(j % 7 - 3 - u)).bfloat16()
    p, q = me.gemm_inputs(family, m, n, k)
    return ((p.float() * block_pow2((5 * kb) % 13 - 6 + 0 * i)).bfloat16(),
            (q.float() * block_pow2((3 * kb + 4) % 13 - 6 + 0 * j)).bfloat16())


@pytest.mark.parametrize("shape", [(m, n, k) for m in (1, 127, 129, 300) for n in (8, 136) for k in (32, 128, 160, 416)]
                         + [(256, 256, 256)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pair", [(fp8.E4M3, fp8.E4M3), (fp8.E5M2, fp8.E4M3)], ids=lambda p: "x".join(p))
def test_mx_gemm(gpu_ext, pair, shape):
    """Every family, bias off and on (zero for the exact families: a scaled integer plus a bias is not exact), into
    a guarded output. one_block and balanced are exact; uniform and cancel are held to ``mx_bound``."""
    m, n, k = shape
    errs = []
    for family in ("one_block", "balanced", "uniform", "cancel"):
        exact = family in ("one_block", "balanced")
        p, q = gemm_family(family, m, n, k)
        (a, ad), (b, bd) = operand(p, pair[0]), operand(q, pair[1])
        assert torch.equal(ad, p.double()) or not exact
        r, mag = me.ref_gemm(ad, bd)
        if family == "balanced":
            unit = 2.0 ** ((torch.arange(m) % 5 - 2).view(m, 1) + (torch.arange(n) % 7 - 3).view(1, n)).double()
            assert float((r / unit).abs().max()) <= 256 and torch.equal(r / unit, (r / unit).round())
        g = torch.Generator().manual_seed(m + n + k)
        bias = (torch.zeros(n) if exact else torch.rand(n, generator=g) * 2 - 1).bfloat16()
        for with_bias in (False, True):
            ref, amag = (r + bias.double(), mag + bias.double().abs()) if with_bias else (r, mag)
            buf, view = me.guarded(m, n, n + 8, torch.bfloat16, DEV)
            fp8.mx_gemm_into(view, a, b, bias.to(DEV) if with_bias else None)
            name = f"{family} bias={with_bias}"
            me.check(name, me.take_guarded(name, buf, view, errs).cpu(), ref, None if exact else mx_bound(ref, amag, k), errs)
    assert not errs, "\n".join(errs)


def check_linear(name, y, dx, ref, n_in, n_out, errs):
    yr, dxr, ya, dxa = ref
    me.check(f"{name} y", y.cpu(), yr, mx_bound(yr, ya, n_in), errs)
    me.check(f"{name} dx", dx.cpu(), dxr, mx_bound(dxr, dxa, n_out), errs)


def mx_linear(x, w, b):
    assert fp8.mx_supported(x, w)  # not the fallback
    return fp8.fp8_linear(x, w, b, state=fp8.Fp8State("mx"))


@pytest.mark.parametrize("shape", [(130, 160, 96), (1024, 256, 256)], ids=lambda s: "x".join(map(str, s)))
def test_mx_linear(gpu_ext, monkeypatch, shape):
    """y and dx within the GEMM's bound of the float64 reference on the same quantisation; dW and db are the bf16
    kernels' (``ops.linear.linear`` with its one-launch backward off) bit for bit. One inf in dy: a non-finite dx."""
    from fluxmpi_amd.ops import linear as L
    monkeypatch.setattr(L, "LINBWD", False)
    rows, n_in, n_out = shape
    x, w, b, dy = linear_data(rows, n_in, n_out)
    errs = []
    y, dx, dw, db = step(mx_linear, x, w, b, dy)
    _, _, dw_ref, db_ref = step(L.linear, x, w, b, dy)
    assert torch.equal(dw, dw_ref) and torch.equal(db, db_ref)
    check_linear("step", y, dx, fp8.mx_linear_reference(x, w, b, dy), n_in, n_out, errs)
    dy[5, 7] = float("inf")
    assert not bool(torch.isfinite(step(mx_linear, x, w, b, dy)[1]).all())
    assert not errs, "\n".join(errs)


def mx_module(w, b):
    lin = fp8.Fp8Linear(w.shape[1], w.shape[0], scaling="mx").to(DEV).bfloat16()
    with torch.no_grad():
        lin.weight.copy_(w), lin.bias.copy_(b)
    return lin


def module_step(lin, x, dy):
    lin.weight.grad = lin.bias.grad = x.grad = None
    y = lin(x)
    y.backward(dy)
    return [y.detach(), x.grad, lin.weight.grad, lin.bias.grad]


def test_mx_graph(gpu_ext):
    """One forward + backward captured in a HIP graph: three replays are bit-equal to the eager step."""
    x, w, b, dy = linear_data(130, 160, 96)
    xd, dyd = x.to(DEV).requires_grad_(), dy.to(DEV)
    assert fp8.mx_supported(xd, mx_module(w, b).weight)
    eager = [t.clone() for t in module_step(mx_module(w, b), xd, dyd)]
    lin = mx_module(w, b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = module_step(lin, xd, dyd)
    for replay in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for name, a, e in zip(("y", "dx", "dW", "db"), got, eager):
            assert torch.equal(a, e), f"replay {replay}: {name} differs from the eager step"


def test_after_optimizer_step(gpu_ext):
    """The step after a fused Adam update through raw pointers (``weight._version`` does not move) runs on the
    updated weight, forward and input gradient."""
    from fluxmpi_amd.ops import optim as fused
    rows, n_in, n_out = 130, 160, 96
    x, w, b, dy = linear_data(rows, n_in, n_out)
    lin = mx_module(w, b)
    xd, dyd = x.to(DEV).requires_grad_(), dy.to(DEV)
    assert fp8.mx_supported(xd, lin.weight)
    lin(xd).backward(dyd)
    ps = [lin.weight, lin.bias]
    version = lin.weight._version
    fused.adam_([p.detach() for p in ps], [p.grad for p in ps], [torch.zeros_like(p) for p in ps],
                [torch.zeros_like(p) for p in ps], lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8, bc1=0.1, bc2=0.001)
    w2, b2 = lin.weight.detach().cpu(), lin.bias.detach().cpu()
    assert lin.weight._version == version and float((w2.float() - w.float()).abs().max()) > 0.02
    y, dx, _, _ = module_step(lin, xd, dyd)
    errs = []
    check_linear("after the update", y, dx, fp8.mx_linear_reference(x, w2, b2, dy), n_in, n_out, errs)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("case", ["fp16", "n_in=48"])
def test_fallback(gpu_ext, case):
    from fluxmpi_amd.ops.linear import linear
    x, w, b, dy = linear_data(130, 48 if case == "n_in=48" else 160, 96)
    if case == "fp16":
        x, w, b, dy = (t.half() for t in (x, w, b, dy))
    assert not fp8.mx_supported(x.to(DEV), w.to(DEV).requires_grad_())
    mx = lambda *a: fp8.fp8_linear(*a, state=fp8.Fp8State("mx"))
    for got, want in zip(step(mx, x, w, b, dy), step(linear, x, w, b, dy)):
        assert torch.equal(got, want)


def test_vit(gpu_ext, monkeypatch):
    from fluxmpi_amd.models.vit import vit_tiny
    monkeypatch.delenv("FLUXMPI_FP8", raising=False)
    models = {}
    for name, kw in (("default", {}), ("off", {"fp8": False}), ("mx", {"fp8": "mx"})):
        torch.manual_seed(5)
        models[name] = vit_tiny(**kw).to(DEV).bfloat16()
    x = torch.randn(5, 3, 32, 32, generator=torch.Generator().manual_seed(6)).bfloat16().to(DEV)
    assert torch.equal(models["default"](x), models["off"](x))
    tokens = torch.zeros(5, 17, 64, dtype=torch.bfloat16, device=DEV)
    assert all(blk.qkv.fp8.scaling == "mx" and fp8.mx_supported(tokens, blk.qkv.weight) for blk in models["mx"].blocks)
    y = models["mx"](x)
    y.float().square().sum().backward()
    assert bool(torch.isfinite(y).all())
    for k, p in models["mx"].named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
