"""The e2m1 (fp4) side of ``ops.fp8`` on the CPU: the reference quantiser's grid, scale rule, rounding and non-finite
blocks, and the nibble packing."""
import pytest
import torch

from fluxmpi_amd.ops import fp8

TIES = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0}


def block_input(r, c, seed=0):
    """bf16 ``[r, c]``, every 32-block of a row with a magnitude of its own, 2^-6 .. 2^6."""
    g = torch.Generator().manual_seed(seed)
    mag = 2.0 ** torch.randint(-6, 7, (r, c // 32), generator=g).float()
    return ((torch.rand(r, c, generator=g) * 2 - 1) * mag.repeat_interleave(32, 1)).bfloat16()


@pytest.mark.parametrize("shape", [(3, 32), (17, 416)], ids=lambda s: "x".join(map(str, s)))
def test_grid_and_scale(shape):
    """Every value is on the grid and no finite block is clamped: the rounded amax is in [amax / 2, 6]."""
    x = block_input(*shape)
    q, by = fp8.mx_quantize_reference(x, fp8.E2M1)
    assert q.dtype == torch.float32 and q.shape == x.shape and by.shape == (shape[0], shape[1] // 32)
    assert set(q.abs().unique().tolist()) <= set(fp8.FP4_GRID)
    qmax = q.view(*by.shape, 32).abs().amax(-1).double()
    amax = x.double().view(*by.shape, 32).abs().amax(-1)
    assert bool((qmax <= 6).all()) and bool((qmax * 2.0 ** (by.double() - 127) >= amax / 2).all())
    assert bool((qmax >= 3).all())  # the scale is the largest that does not clamp


def test_pack_roundtrip():
    """All 16 codes in both nibbles; element 2 i is the low nibble of byte i."""
    codes = torch.arange(256, dtype=torch.uint8).view(4, 64)
    v = fp8.mx_unpack_fp4(codes)
    assert torch.equal(fp8.mx_pack_fp4(v), codes)
    assert v[0, :6].tolist() == [0.0, 0.0, 0.5, 0.0, 1.0, 0.0] and v[0, 16 * 2 + 1] == 0.5 and v[3, 63 * 2 + 1] == -6.0


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -9, 2.0 ** 20])
def test_ties(scale, sign):
    """Round to nearest, a midpoint to the neighbour with the even mantissa bit (the block's amax 6 keeps the scale)."""
    x = torch.zeros(1, 32)
    x[0, :7], x[0, 7] = torch.tensor(list(TIES)), 6.0
    q, by = fp8.mx_quantize_reference((sign * scale * x).bfloat16(), fp8.E2M1)
    assert q[0, :8].tolist() == [sign * v for v in TIES.values()] + [sign * 6.0]
    assert 2.0 ** (int(by[0, 0]) - 127) == scale


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_nonfinite_and_zero_blocks(bad):
    """A block with an inf or NaN: zeros under the byte 255, its neighbours untouched; an all-zero block: byte 127."""
    x = block_input(2, 96)
    x[0, 40], x[1, :32] = bad, 0.0
    q, by = fp8.mx_quantize_reference(x, fp8.E2M1)
    assert by[0].tolist()[1] == 255 and not bool(q[0, 32:64].any()) and by[1, 0] == 127 and not bool(q[1, :32].any())
    clean, cby = fp8.mx_quantize_reference(block_input(2, 96), fp8.E2M1)
    assert torch.equal(q[0, :32], clean[0, :32]) and torch.equal(q[0, 64:], clean[0, 64:]) and by[0, 0] == cby[0, 0]
    assert bool(torch.isfinite(fp8.mx_dequantize(q, by)[1]).all())


def test_arguments():
    """e2m1 is an MX format only, and the fp4 forward has no fp8 weight gradient."""
    assert fp8.FMT_CODE[fp8.E2M1] == 2 and fp8.FMAX[fp8.E2M1] == 6.0 and fp8.pow2_scale(6.0, fp8.E2M1) == 1.0
    assert fp8.pow2_scale(6.5, fp8.E2M1) == 0.5 and fp8.pow2_scale(0.75, fp8.E2M1) == 8.0
    assert fp8.Fp8State("mx", fwd="e2m1").fwd == fp8.E2M1
    for make in (lambda: fp8.Fp8State("mx", fwd="e2m1", wgrad="mx"), lambda: fp8.Fp8State("current", fwd="e2m1"),
                 lambda: fp8.Fp8Linear(64, 96, scaling="mx", fwd="e2m1", wgrad="mx"),
                 lambda: fp8.quantize_reference(torch.ones(2, 8), fp8.E2M1)):
        with pytest.raises(ValueError):
            make()
