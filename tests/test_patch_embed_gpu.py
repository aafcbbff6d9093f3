"""``csrc/kernels/patch_embed.hip`` against float64: every element of the forward within the derived bound
(exact for ternary inputs), the weight gradient through the autograd node, and the model switch."""
import copy

import pytest
import torch

from fluxmpi_amd.ops import patch_embed as pe
from tests import mfma_edges as me

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = {3: "M = 18, one partial tile", 43: "M = 258, whole tiles plus a rest"}  # B -> (B, 2p, 3p)


def image_of(a, b, p, c):
    """The inverse unfold: A [B * 6, p p C] in (i, j, c) order -> the channels_last batch [B, C, 2p, 3p];
    channel 3 (C = 4) is filled with 1.0."""
    nhwc = a.view(b, 2, 3, p, p, c).permute(0, 1, 3, 2, 4, 5).reshape(b, 2 * p, 3 * p, c).clone()
    if c == 4:
        nhwc[..., 3] = 1.0
    return nhwc.to(DEV).permute(0, 3, 1, 2)


MIXED = (torch.float32, torch.bfloat16, torch.bfloat16)  # each of bias / cls / pos carries its own type


def params_of(family, d, n, dtype, seed):
    """bias [D], cls [1, 1, D], pos [1, n + 1, D]: small integers for the exact family."""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,) * 3
    g = torch.Generator().manual_seed(seed)
    if family == "ternary":
        vals = [torch.randint(-2, 3, s, generator=g).float() for s in ((d,), (1, 1, d), (1, n + 1, d))]
    else:
        vals = [torch.rand(s, generator=g) * 2 - 1 for s in ((d,), (1, 1, d), (1, n + 1, d))]
    return [v.to(t) for v, t in zip(vals, dtypes)]


def filter_of(wp, p, c):
    """The parameter [D, 3 p p] in (c, i, j) order whose pack is ``wp`` (its channel-3 columns dropped)."""
    d = wp.shape[0]
    return wp.view(d, p, p, c)[..., :3].permute(0, 3, 1, 2).reshape(d, 3 * p * p).contiguous()


def drop_c3(a, p, c):
    a = a.clone().view(-1, p, p, c)
    if c == 4:
        a[..., 3] = 0
    return a.view(-1, p * p * c)


@pytest.mark.parametrize("pdtype", [torch.bfloat16, torch.float32, MIXED], ids=["pbf16", "pf32", "pmixed"])
@pytest.mark.parametrize("family", ["uniform", "ternary"])
@pytest.mark.parametrize("b", list(SHAPES))
@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("p", [16, 8])
@pytest.mark.parametrize("c", [3, 4])
def test_forward(gpu_ext, c, p, d, b, family, pdtype):
    n, m, kp = 6, b * 6, p * p * c
    a, wp = me.gemm_inputs(family, m, d, kp)
    wp = drop_c3(wp, p, c)
    bias, cls, pos = params_of(family, d, n, pdtype, seed=m + d)
    x = image_of(a, b, p, c)
    r, mag = me.ref_gemm(drop_c3(a, p, c), wp)
    add = (bias.double() + pos.double()[0, 1:]).repeat(b, 1, 1).view(m, d)
    mag = mag + (bias.double().abs() + pos.double()[0, 1:].abs()).repeat(b, 1, 1).view(m, d)
    ref = r + add
    errs = []
    buf, view = me.guarded(b * (n + 1), d, d + 8, torch.bfloat16, DEV)
    pe.forward_into(view, x, filter_of(wp, p, c).to(DEV), bias.to(DEV), cls.to(DEV), pos.to(DEV), p)
    got = me.take_guarded("out", buf, view, errs).cpu().view(b, n + 1, d)
    if family == "ternary":
        assert float(ref.abs().max()) < 256
    me.check("tokens", got[:, 1:].reshape(m, d), ref, None if family == "ternary" else me.bound(ref, mag, kp, "bf16"), errs)
    row0 = (cls.float() + pos.float()[:, :1]).bfloat16().expand(b, 1, d)
    me.check("cls row", got[:, :1], row0.double(), None, errs)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("splits", [None, 1, 2], ids=["auto", "s1", "s2"])
@pytest.mark.parametrize("family", ["uniform", "ternary"])
@pytest.mark.parametrize("b", list(SHAPES))
@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("p", [16, 8])
@pytest.mark.parametrize("c", [3, 4])
def test_weight_gradient(gpu_ext, monkeypatch, c, p, d, b, family, splits):
    """``splits``: the node's own choice (64-token ranges, one step each at these shapes), or 1 / 2 ranges: at
    M = 258 a workgroup then walks 5 / 3 steps of 64 tokens through both LDS stages, across sample wraps
    (n = 6), with a partial last step."""
    from fluxmpi_amd.ops import graddst
    monkeypatch.setattr(pe, "WGRAD_SPLITS", splits)
    n, m, kp = 6, b * 6, p * p * c
    dyt, at = me.gemm_inputs(family, d, kp, m)  # dY[:, 1:]^T [D, M] and A^T [K', M]: the reduction runs over M
    x = image_of(at.t().contiguous(), b, p, c)
    dy = torch.full((b, n + 1, d), 1e4, dtype=torch.bfloat16)
    dy[:, 1:] = dyt.t().reshape(b, n, d)
    w, bias, cls, pos = (t.to(DEV).requires_grad_() for t in
                         (torch.zeros(d, 3 * p * p, dtype=torch.bfloat16), *params_of("uniform", d, n, torch.bfloat16, 1)))
    with graddst.into(None):
        pe.patch_embed(x, w, bias, cls, pos, p).backward(dy.to(DEV))
    r, mag = me.ref_gemm(dyt, at)  # dW' [D, K'] in (i, j, c) order
    r, mag = (filter_of(t, p, c) for t in (r, mag))
    errs = []
    if family == "ternary":
        assert float(r.abs().max()) < 256
    me.check("dW", w.grad.cpu(), r, None if family == "ternary" else me.bound(r, mag, m, "bf16"), errs)
    dyd = dy.double()
    for name, got, ref, mg in (("dpos", pos.grad[0], dyd.sum(0), dyd.abs().sum(0)),
                               ("dcls", cls.grad[0, 0], dyd[:, 0].sum(0), dyd[:, 0].abs().sum(0)),
                               ("dbias", bias.grad, dyd[:, 1:].sum((0, 1)), dyd[:, 1:].abs().sum((0, 1)))):
        me.check(name, got.cpu(), ref, m * me.E23 * mg + me.U8 * ref.abs() + me.TINY, errs)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("c", [3, 4])
def test_model(gpu_ext, monkeypatch, c):
    """``vit_tiny(embed="fused")`` against ``vit_tiny()`` and a float64 CPU copy on a channels_last bf16 batch
    of 5: the fused path's worst error (max |err| / max |ref| over the logits and the four front-end
    gradients) is at most twice the unfold path's. Measured on MI355X (unfold / fused): 3 channels 0.00726 /
    0.00620, 4 channels 0.00906 / 0.00652."""
    from fluxmpi_amd.models.vit import vit_tiny
    torch.manual_seed(11)
    unfold = vit_tiny()
    with torch.no_grad():
        unfold.cls.normal_(0, 0.5)
        unfold.embed.proj.bias.normal_(0, 0.5)
    fused = vit_tiny(embed="fused")
    fused.load_state_dict(unfold.state_dict())
    ref = copy.deepcopy(unfold).double()
    assert {k: v.shape for k, v in fused.state_dict().items()} == {k: v.shape for k, v in unfold.state_dict().items()}
    x = torch.randn(5, c, 32, 32).bfloat16().to(DEV).contiguous(memory_format=torch.channels_last)
    calls = []
    real = pe.patch_embed
    monkeypatch.setattr(pe, "patch_embed", lambda *a: (calls.append(1), real(*a))[1])

    def run(model, inp):
        model.zero_grad()
        y = model(inp)
        y.double().square().sum().backward()
        f = model.embed.proj
        return [t.detach().double().cpu() for t in (y, f.weight.grad, f.bias.grad, model.cls.grad, model.pos.grad)]

    want = run(ref, x[:, :3].cpu().double())
    worst = {}
    for name, model in (("unfold", unfold), ("fused", fused)):
        got = run(model.to(DEV).bfloat16(), x if name == "fused" else x[:, :3])
        worst[name] = max(float((g - r).abs().max() / r.abs().max()) for g, r in zip(got, want))
    print(f"worst error: unfold {worst['unfold']:.4g}, fused {worst['fused']:.4g}")
    assert len(calls) == 1
    assert worst["fused"] <= 2 * worst["unfold"], worst
    xg = x.clone().requires_grad_()  # an image that wants a gradient takes the unfold path and gets one
    fused(xg).float().sum().backward()
    assert len(calls) == 1 and xg.grad is not None
