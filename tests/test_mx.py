"""The CPU side of MX block scaling in ``fluxmpi_amd.ops.fp8``: the reference quantiser against the scalar scale rule
block by block, the CPU fallback, the model switch. ``quant_input`` also feeds ``test_mx_gpu.py``."""
import math

import pytest
import torch

from fluxmpi_amd.ops import fp8

KINDS = ("binades", "edges", "ties", "zeros", "nonfinite")


def quant_input(kind, r, c, fmt):
    """bf16 ``[r, c]``. binades: block (i, b) has magnitude 2^u, u spread over -20 .. 20 so that neighbouring scales
    differ, and block (0, 0) has amax 2^-124 (the exponent clamp). edges: block amax exactly 2^e, 1.75 2^e, and the
    next bf16 above. ties: the per-tensor test's generator. nonfinite: binades with a NaN and an inf."""
    from tests.test_fp8_gpu import quant_input as per_tensor_input
    g = torch.Generator().manual_seed(r * 1000 + c)
    nb = c // 32
    if kind == "zeros":
        return torch.zeros(r, c).bfloat16()
    if kind == "ties":
        return per_tensor_input("ties", r, c, fmt)
    i, b = torch.arange(r).view(r, 1, 1), torch.arange(nb).view(1, nb, 1)
    x = (torch.rand(r, nb, 32, generator=g) * 0.98 + 0.01) * (torch.randint(0, 2, (r, nb, 32), generator=g) * 2 - 1)
    if kind == "edges":
        top = torch.tensor([1.0, 1.75, 1.7578125])[(i + b) % 3].expand(r, nb, 1)
        x = x * 0.99
        x.scatter_(2, ((3 * i + 5 * b) % 32).expand(r, nb, 1), top * (1 - 2 * ((i + b) % 2)))
        return (x * 2.0 ** ((7 * i + 3 * b) % 25 - 12)).view(r, c).bfloat16()
    x = x * 2.0 ** ((17 * i + 11 * b) % 41 - 20)
    x[0, 0] = x[0, 0].sign() * 2.0 ** -124 * torch.where(torch.arange(32) % 2 == 0, 1.0, 0.5)
    x = x.view(r, c).bfloat16()
    if kind == "nonfinite":
        x[0, 5], x[r - 1, c - 7] = float("nan"), float("-inf")
    return x


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", [fp8.E4M3, fp8.E5M2])
def test_reference_rule(fmt, kind):
    """Every block's byte is 127 - log2(pow2_scale(block amax)) of the scalar function; the block's amax lands in
    (FMAX / 2, FMAX] after scaling unless the exponent was clamped; nothing finite saturates or turns non-finite."""
    r, c = 17, 96
    x = quant_input(kind, r, c, fmt)
    q, by = fp8.mx_quantize_reference(x, fmt)
    assert q.shape == (r, c) and by.shape == (r, c // 32) and by.dtype == torch.uint8
    xf, qf = x.float().view(r, -1, 32), q.float().view(r, -1, 32)
    for i in range(r):
        for b in range(c // 32):
            amax = float(xf[i, b].abs().max())
            s = fp8.pow2_scale(amax, fmt)
            assert int(by[i, b]) == 127 - int(math.log2(s)) and 1 <= int(by[i, b]) <= 253
            fin = torch.isfinite(xf[i, b])
            assert bool(torch.isfinite(qf[i, b][fin]).all()) and not bool(torch.isfinite(qf[i, b][~fin]).any())
            if math.isfinite(amax) and amax > 0 and s < 2.0 ** 126:
                assert fp8.FMAX[fmt] / 2 < amax * s <= fp8.FMAX[fmt]  # so the clamp never acts on a finite value
                assert fp8.FMAX[fmt] / 2 <= float(qf[i, b].abs().max()) <= fp8.FMAX[fmt]
    assert bool((by == 127).all()) == (kind == "zeros")


@pytest.mark.parametrize("fmt", [fp8.E4M3, fp8.E5M2])
def test_reference_round_trip(fmt):
    """Signed powers of two within 8 binades of their block's amax come back exactly from q 2^(byte - 127)."""
    g = torch.Generator().manual_seed(3)
    x = ((torch.randint(0, 2, (9, 4, 32), generator=g) * 2 - 1)
         * 2.0 ** (torch.randint(-7, 1, (9, 4, 32), generator=g) + torch.randint(-30, 30, (9, 4, 1), generator=g)))
    x = x.view(9, 128).bfloat16()
    assert torch.equal(fp8.mx_dequantize(*fp8.mx_quantize_reference(x, fmt)), x.double())


def test_cpu_is_linear():
    from fluxmpi_amd.ops.linear import linear
    torch.manual_seed(0)
    lin = fp8.Fp8Linear(32, 64, scaling="mx").bfloat16()
    assert list(lin.state_dict()) == ["weight", "bias"] and lin.fp8.scaling == "mx"
    x = torch.randn(5, 32).bfloat16().requires_grad_()
    assert not fp8.mx_supported(x, lin.weight)
    assert torch.equal(lin(x), linear(x, lin.weight, lin.bias))
    with pytest.raises(ValueError, match="fp8.mx_quantize"):
        fp8.mx_quantize(x.detach(), fp8.E4M3)
    with pytest.raises(ValueError, match="fp8.mx"):
        fp8.MxTensor(None, None, None, None, fp8.E4M3).t()


def test_model_switch(monkeypatch):
    from fluxmpi_amd.models.vit import vit_tiny
    monkeypatch.delenv("FLUXMPI_FP8", raising=False)
    default = vit_tiny()
    shapes = {k: v.shape for k, v in default.state_dict().items()}
    for kw, env, want in (({"fp8": "mx"}, None, "mx"), ({}, "mx", "mx"), ({"fp8": True}, None, "current"),
                          ({}, "1", "current"), ({"fp8": True}, "mx", "current")):
        if env is not None:
            monkeypatch.setenv("FLUXMPI_FP8", env)
        model = vit_tiny(**kw)
        monkeypatch.delenv("FLUXMPI_FP8", raising=False)
        assert all(type(blk.qkv) is fp8.Fp8Linear and blk.qkv.fp8.scaling == want for blk in model.blocks), (kw, env)
        assert {k: v.shape for k, v in model.state_dict().items()} == shapes
    assert not any(isinstance(blk.qkv, fp8.Fp8Linear) for blk in default.blocks)
