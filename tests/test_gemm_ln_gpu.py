"""The Linear + residual add + LayerNorm forward as one full-row GEMM (csrc/kernels/gemm_ln.hip): the raw entry
per element against float64, the autograd node on that route, and the fall-back for shapes it does not take."""
import pytest
import torch
import torch.nn.functional as F

from . import mfma_edges as E
from . import norm_edges as NE

pytestmark = pytest.mark.gpu

# (M, N, K, max_blocks): one row / a unit with one live row / partial tiles, three k-tiles / the ring wraps many
# times / two workgroups walk several tiles each, the last partial / one workgroup, every tile boundary
CASES = [(1, 384, 64, 0), (65, 384, 128, 0), (200, 768, 192, 0), (77, 768, 1536, 0), (333, 768, 128, 2),
         (333, 384, 64, 1)]
L_CHAIN = 24 + 4 + 8  # see test_gemm_ln_kernel
CODE = {torch.float32: 7, torch.bfloat16: 9}


def _rel(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


@pytest.mark.parametrize("M,N,K,max_blocks", CASES)
@pytest.mark.parametrize("family", E.FAMILIES)
def test_gemm_ln_kernel(gpu_ext, family, M, N, K, max_blocks):
    """h = bf16(a W^T + bias + x) against float64 (exact for the exact families, else mfma_edges.bound over K + 2
    terms and one bf16 rounding), then mean / rstd / y against float64 of the kernel's OWN stored h with
    norm_edges' two-pass bounds at the kernel's longest summation chain
        L = 24 (a lane's values of a row) + 4 (lane steps; the kernel takes 2) + 8 (waves; 4 at N = 384) = 36,
    which over-counts as ln_L does. Every output sits in a NaN-filled guarded buffer. bias and x: uniform for
    uniform / cancel, {-1, 0, 1} for ternary (nnz 64, so |h| <= 66 is an exact bf16 integer) and 0 for gather,
    whose h is then the W bit pattern itself; its rows of full-range bf16 patterns overflow an fp32 variance, so
    the gather family checks h and the guards only. N = 768 takes a bf16 bias and an fp32 affine, N = 384 the
    other way round."""
    from fluxmpi_amd.ops import _ext
    dev, eps = "cuda", 1e-5
    a, W = E.gemm_inputs(family, M, N, K, nnz=64)
    g = E._gen("gemm_ln", family, M, N, K)
    if family in E.EXACT:
        lim = 2 if family == "ternary" else 1  # randint's exclusive end: {-1, 0, 1} or {0}
        bias, x = (torch.randint(1 - lim, lim, s, generator=g).float() for s in ((N,), (M, N)))
    else:
        bias, x = E._uni(g, N), E._uni(g, M, N)
    lw, lb = NE.affine(g, N)
    bdt, adt = (torch.bfloat16, torch.float32) if N == 768 else (torch.float32, torch.bfloat16)
    bias, x, lw, lb = bias.to(bdt), x.bfloat16(), lw.to(adt), lb.to(adt)
    bufs = {k: E.guarded(M, N, N, torch.bfloat16, dev) for k in ("h", "y")}
    bufs.update({k: E.guarded(1, M, M, torch.float32, dev) for k in ("mean", "rstd")})
    d = [t.to(dev) for t in (a, W, bias, x, lw, lb)]
    _ext.ln().linear_add_ln_fwd(*(t.data_ptr() for t in d[:4]), bufs["h"][1].data_ptr(), bufs["y"][1].data_ptr(),
                                d[4].data_ptr(), d[5].data_ptr(), bufs["mean"][1].data_ptr(), bufs["rstd"][1].data_ptr(),
                                M, N, K, eps, CODE[bdt], CODE[adt], torch.cuda.current_stream().cuda_stream, max_blocks)
    torch.cuda.synchronize()
    errs = []
    out = {k: E.take_guarded(k, *bufs[k], errs).cpu() for k in bufs}
    r, ab = E.ref_gemm(a, W)
    r, ab = r + bias.double() + x.double(), ab + bias.double().abs() + x.double().abs()
    if family in E.EXACT:
        assert float(r.abs().max()) <= 256 or family == "gather"
    E.check_out("h", family, out["h"], r, ab, K + 2, "bf16", errs)
    if family != "gather" and not errs:
        h = out["h"]
        mean, var, a1, _ = NE.stats_ref(h, 1)
        rstd, dmean, drstd = NE.two_pass_bounds(L_CHAIN, mean, var, a1, eps)
        c, wd, bd = h.double() - mean[:, None], lw.double(), lb.double()
        y = c * rstd[:, None] * wd + bd
        dy = (wd.abs() * (c.abs() * drstd[:, None] + (rstd * dmean)[:, None] + (drstd * dmean)[:, None])
              + 3 * NE.U32 * (c * rstd[:, None] * wd).abs() + 2 * NE.U32 * (y.abs() + bd.abs())
              + NE.rt(torch.bfloat16, y))  # ln_refs' y bound
        E.check("mean", out["mean"][0], mean, dmean + E.TINY, errs)
        E.check("rstd", out["rstd"][0], rstd, drstd + E.TINY, errs)
        E.check("y", out["y"], y, dy + E.TINY, errs)
    assert not errs, "\n".join(errs)


def _node_inputs(d, k, shape=(2, 100)):
    torch.manual_seed(3)
    mk = lambda *s, scale=1.0: (torch.randn(*s, device="cuda") * scale).bfloat16()
    return [mk(*shape, k, scale=0.5), mk(d, k, scale=0.05), mk(d, scale=0.1), mk(*shape, d),
            (torch.rand(d, device="cuda") + 0.5).bfloat16(), mk(d, scale=0.1)]


def test_gemm_ln_node(gpu_ext, monkeypatch):
    """linear_add_layer_norm(fused_fwd=True): forward and all six gradients against the fp32 composition by
    test_layernorm.py::test_linear_add_layer_norm's criterion, with ops.linear.fwd made to raise during the forward
    (the fused route has no use for it); fused_fwd=False is bit-identical to leaving the argument out."""
    from fluxmpi_amd.ops import linear
    from fluxmpi_amd.ops.layernorm import linear_add_layer_norm
    d = 384
    base = _node_inputs(d, 128)
    ins = [t.clone().requires_grad_() for t in base]
    ref = [t.float().clone().requires_grad_() for t in base]

    def boom(*a, **k):
        raise AssertionError("the composition's Linear forward ran")

    with monkeypatch.context() as mp:
        mp.setattr(linear, "fwd", boom)
        h, y = linear_add_layer_norm(*ins, 1e-6, fused_fwd=True)
    hr = ref[3] + F.linear(ref[0], ref[1], ref[2])
    yr = F.layer_norm(hr, (d,), ref[4], ref[5], 1e-6)
    gh, gy = torch.randn_like(hr), torch.randn_like(yr)
    ((h.float() * gh).sum() + (y.float() * gy).sum()).backward()
    ((hr * gh).sum() + (yr * gy).sum()).backward()
    assert _rel(h, hr) < 2e-2 and _rel(y, yr) < 2e-2
    for t, r in zip(ins, ref):
        assert t.grad is not None and t.grad.dtype == t.dtype
        assert _rel(t.grad, r.grad) < 3e-2
    off = linear_add_layer_norm(*[t.clone().requires_grad_() for t in base], 1e-6, fused_fwd=False)
    plain = linear_add_layer_norm(*[t.clone().requires_grad_() for t in base], 1e-6)
    assert all(torch.equal(u, v) for u, v in zip(off, plain))


def test_gemm_ln_unsupported_falls_back(gpu_ext):
    """N = 1032, K = 96 is no shape of the kernel: fused_fwd=True gives the composition's result."""
    from fluxmpi_amd.ops import _ext
    from fluxmpi_amd.ops.layernorm import linear_add_layer_norm
    base = _node_inputs(1032, 96)
    assert not _ext.ln().linear_add_ln_supported(200, 1032, 96)
    on = linear_add_layer_norm(*[t.clone().requires_grad_() for t in base], 1e-6, fused_fwd=True)
    plain = linear_add_layer_norm(*[t.clone().requires_grad_() for t in base], 1e-6)
    assert all(torch.equal(u, v) for u, v in zip(on, plain))
