"""The CPU side of ``fluxmpi_amd.ops.fp8``: the scale rule, the reference quantiser, the errors, the CPU fallback."""
import pytest
import torch

from fluxmpi_amd.ops import fp8


@pytest.mark.parametrize("fmt, top", [(fp8.E4M3, 8), (fp8.E5M2, 15)])
def test_pow2_scale(fmt, top):
    """FMAX = 1.75 * 2^top: the scale steps down where amax's significand passes 1.75, and amax * scale is the
    largest power-of-two multiple of amax that does not exceed FMAX."""
    for e in (-20, -1, 0, 3, 30):
        for m, step in ((1.0, 0), (1.75, 0), (1.7578125, 1), (1.9921875, 1)):
            s = fp8.pow2_scale(m * 2.0 ** e, fmt)
            assert s == 2.0 ** (top - e - step)
            assert m * 2.0 ** e * s <= fp8.FMAX[fmt] < 2 * m * 2.0 ** e * s
    assert fp8.pow2_scale(fp8.FMAX[fmt], fmt) == 1.0
    for amax in (0.0, float("inf"), float("nan")):
        assert fp8.pow2_scale(amax, fmt) == 1.0
    assert fp8.pow2_scale(2.0 ** -140, fmt) == 2.0 ** 126 and fp8.pow2_scale(2.0 ** 127, fp8.E4M3) == 2.0 ** -119


@pytest.mark.parametrize("fmt", [fp8.E4M3, fp8.E5M2])
def test_quantize_reference(fmt):
    """Values the format holds survive the round trip at any scale; the largest input lands in (FMAX / 2, FMAX];
    an outgrown scale saturates; NaN and inf stay non-finite."""
    bits = 3 if fmt == fp8.E4M3 else 2
    x = (torch.arange(-2 ** bits, 2 ** bits + 1).float() / 2 ** bits * 2.0).bfloat16()  # bits + 1 significant bits
    q, s = fp8.quantize_reference(x, fmt)
    assert s == fp8.pow2_scale(2.0, fmt) and torch.equal(q.float() / s, x.float())
    assert fp8.FMAX[fmt] / 2 < float(q.float().abs().max()) <= fp8.FMAX[fmt]
    q, _ = fp8.quantize_reference(x, fmt, 2.0 ** 30)
    assert set(q.float().abs().tolist()) == {0.0, fp8.FMAX[fmt]}
    q, s = fp8.quantize_reference(torch.tensor([1.0, float("nan"), float("-inf")]), fmt)
    assert s == 1.0 and q.float().isfinite().tolist() == [True, False, False]


def test_errors_name_the_op():
    x = torch.zeros(4, 16, dtype=torch.bfloat16)
    t = fp8.Fp8Tensor(torch.zeros(4, 16, dtype=torch.uint8), None, fp8.new_block("cpu"), fp8.E4M3)
    for match, call in (("fp8", lambda: fp8.pow2_scale(1.0, "e3m4")),
                        ("fp8.quantize", lambda: fp8.quantize(x, fp8.E4M3)),
                        ("fp8.quantize", lambda: fp8.quantize_into(x, fp8.E4M3, fp8.new_block("cpu"))),
                        ("fp8.gemm", lambda: fp8.gemm_into(torch.zeros(4, 4, dtype=torch.bfloat16), t, t)),
                        ("fp8", lambda: t.t()),
                        ("fp8_linear", lambda: fp8.Fp8Linear(16, 16, scaling="history"))):
        with pytest.raises(ValueError, match=match):
            call()


def test_cpu_is_linear():
    torch.manual_seed(0)
    lin = fp8.Fp8Linear(16, 32, scaling="delayed")
    assert list(lin.state_dict()) == ["weight", "bias"] and lin.bfloat16().fp8_blocks.dtype == torch.int32
    x = torch.randn(5, 16).bfloat16().requires_grad_()
    assert not fp8.supported(x, lin.weight)
    y = lin(x)
    assert torch.equal(y, torch.nn.functional.linear(x, lin.weight, lin.bias))
    y.sum().backward()
    assert lin.weight.grad is not None and x.grad is not None
