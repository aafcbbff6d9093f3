"""CPU side of the MX weight gradient: the float64 reference and the switch's argument checks."""
import pytest
import torch

from fluxmpi_amd.ops import fp8


@pytest.mark.parametrize("fmt", [fp8.E4M3, fp8.E5M2])
def test_reference_exact(fmt):
    """Ternary values times a power of two per 32 tokens survive the cast, so the reference is ``dy^T x`` itself."""
    g = torch.Generator().manual_seed(3)
    tern = lambda *s: torch.randint(-1, 2, s, generator=g).float()
    pow2 = lambda lo, hi, cols: (2.0 ** torch.randint(lo, hi, (3, cols), generator=g).float()).repeat_interleave(32, 0)
    dy, x = (tern(96, 40) * pow2(-9, 10, 40)).bfloat16(), (tern(96, 24) * pow2(-6, 7, 24)).bfloat16()
    ref, mag = fp8.mx_wgrad_reference(dy, x, fmt)
    assert torch.equal(ref, dy.double().t() @ x.double()) and torch.equal(mag, dy.double().abs().t() @ x.double().abs())
    assert ref.shape == (40, 24) and ref.dtype == torch.float64 and float(ref.abs().max()) > 0


@pytest.mark.parametrize("kw, word", [({"scaling": "mx", "wgrad": "fp8"}, "wgrad"), ({"scaling": "mx", "wgrad": None}, "wgrad"),
                                      ({"scaling": "current", "wgrad": "mx"}, "scaling='mx'"),
                                      ({"scaling": "delayed", "wgrad": "mx"}, "scaling='mx'")])
def test_switch_errors(kw, word):
    with pytest.raises(ValueError, match=word):
        fp8.Fp8State(**kw)
    with pytest.raises(ValueError, match=word):
        fp8.Fp8Linear(32, 32, **kw)
    assert fp8.Fp8State("mx").wgrad == "bf16" and fp8.Fp8Linear(32, 32, scaling="mx", wgrad="mx").fp8.wgrad == "mx"
