"""The torch reference of the patch embedding (``ops/patch_embed.py``) against the unfold composition, the
model switch on CPU tensors, and what ``supported`` refuses."""
import pytest
import torch

from fluxmpi_amd.models.vit import PatchEmbed, ViT, vit_tiny
from fluxmpi_amd.ops import patch_embed as pe


@pytest.mark.parametrize("p", [16, 8])
@pytest.mark.parametrize("c", [3, 4])
def test_reference_is_the_unfold_composition(c, p):
    """Pins the K order, the pack and the [CLS] row offset: float64, 1e-12 relative."""
    g = torch.Generator().manual_seed(c * 100 + p)
    b, d, n = 3, 64, 6
    x = torch.randn(b, c, 2 * p, 3 * p, generator=g, dtype=torch.float64)
    emb = PatchEmbed(img=2 * p, patch=p, cin=3, dim=d).double()
    with torch.no_grad():
        emb.proj.bias.normal_(generator=g)
    cls, pos = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((1, 1, d), (1, n + 1, d)))
    want = torch.cat([cls.expand(b, -1, -1), emb(x[:, :3])], 1) + pos
    got = pe.patch_embed_reference(x, emb.proj.weight, emb.proj.bias, cls, pos, p)
    assert got.shape == want.shape
    assert float((got - want).detach().abs().max()) <= 1e-12 * float(want.detach().abs().max())


def test_fused_model_on_cpu_is_the_default_bit_for_bit():
    torch.manual_seed(5)
    a = vit_tiny()
    b = vit_tiny(embed="fused")
    b.load_state_dict(a.state_dict())
    assert list(a.state_dict()) == list(b.state_dict())
    x = torch.randn(4, 3, 32, 32)
    assert torch.equal(a(x), b(x))
    x4 = torch.cat([x, torch.ones(4, 1, 32, 32)], 1).contiguous(memory_format=torch.channels_last)
    assert torch.equal(a(x), b(x4))  # an unsupported 4-channel batch: its first three channels
    xg = x.clone().requires_grad_()  # an image that wants a gradient gets one, whatever the switch
    b(xg).sum().backward()
    assert xg.grad is not None and bool(xg.grad.abs().sum() > 0)
    with pytest.raises(ValueError):
        ViT(embed="im2col")


def test_supported_refuses():
    good = torch.zeros(2, 3, 32, 48, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert pe.layout_ok(good, 16, 64) and pe.layout_ok(good, 8, 192)
    assert not pe.supported(good, 16, 64)  # a CPU tensor
    assert not pe.layout_ok(good.contiguous(), 16, 64)  # NCHW-contiguous
    assert not pe.layout_ok(good.to(torch.float16), 16, 64)
    assert not pe.layout_ok(torch.zeros(2, 28, 42, 3, dtype=torch.bfloat16).permute(0, 3, 1, 2), 14, 64)  # p C % 8
    assert not pe.layout_ok(good, 16, 96) and not pe.layout_ok(good, 5, 64)
    flat = torch.zeros(2 * 3 * 32 * 48 + 8, dtype=torch.bfloat16)
    off = flat[1:1 + 2 * 3 * 32 * 48].view(2, 32, 48, 3).permute(0, 3, 1, 2)  # the same layout, base + 2 bytes
    assert off.data_ptr() % 16 != 0 and not pe.layout_ok(off, 16, 64)
