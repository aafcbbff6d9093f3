"""The fp6 (e2m3 / e3m2) side of ``ops.fp8`` on the CPU: the reference quantiser's grid, scale rule, rounding and
non-finite blocks, the 4-in-3-bytes packing and the argument checks."""
import pytest
import torch

from fluxmpi_amd.ops import fp8
from tests.test_mx4 import block_input

FORMATS = [fp8.E2M3, fp8.E3M2]


def ties(fmt):
    """The 31 midpoints of neighbouring codes (bf16 values: at most 5 significant bits) and where each goes: the
    neighbour whose code is even. Codes 7 | 8 (e2m3) and 3 | 4 (e3m2) straddle the subnormal / normal border."""
    g = fp8.fp6_grid(fmt)
    return (g[:-1] + g[1:]) / 2, torch.stack([g[c + c % 2] for c in range(31)])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", [(3, 32), (17, 416)], ids=lambda s: "x".join(map(str, s)))
def test_grid_and_scale(fmt, shape):
    """Every value is on the grid, no finite block is clamped, and the scale is the largest such: the rounded amax lies
    in [FMAX / 2, FMAX] and dequantises to within a factor 2 of the block's amax."""
    x = block_input(*shape)
    q, by = fp8.mx_quantize_reference(x, fmt)
    assert q.dtype == torch.float32 and q.shape == x.shape and by.shape == (shape[0], shape[1] // 32)
    assert set(q.abs().unique().tolist()) <= set(fp8.fp6_grid(fmt).tolist())
    qmax = q.view(*by.shape, 32).abs().amax(-1).double()
    amax = x.double().view(*by.shape, 32).abs().amax(-1)
    assert bool((qmax <= fp8.FMAX[fmt]).all()) and bool((qmax >= fp8.FMAX[fmt] / 2).all())
    assert bool((qmax * 2.0 ** (by.double() - 127) >= amax / 2).all())
    assert bool((fp8.mx_dequantize(q, by) - x.double()).abs().le(amax.repeat_interleave(32, 1) / 2 ** fp8.FP6_BITS[fmt][0]).all())


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -9, 2.0 ** 20])
def test_ties(fmt, scale, sign):
    """Round to nearest, every midpoint (subnormal ones included) to the even code; the block's amax FMAX keeps the scale."""
    mid, want = ties(fmt)
    x = torch.cat([mid, torch.tensor([fp8.FMAX[fmt]], dtype=torch.float64)]).view(1, 32) * sign * scale
    assert torch.equal(x.bfloat16().double(), x)
    q, by = fp8.mx_quantize_reference(x.bfloat16(), fmt)
    assert q[0, :31].tolist() == (sign * want).tolist() and q[0, 31] == sign * fp8.FMAX[fmt]
    assert 2.0 ** (int(by[0, 0]) - 127) == scale


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_nonfinite_and_zero_blocks(fmt, bad):
    """A block with an inf or NaN: zeros under the byte 255, its neighbours untouched; an all-zero block: byte 127."""
    x = block_input(2, 96)
    x[0, 40], x[1, :32] = bad, 0.0
    q, by = fp8.mx_quantize_reference(x, fmt)
    assert by[0].tolist()[1] == 255 and not bool(q[0, 32:64].any()) and by[1, 0] == 127 and not bool(q[1, :32].any())
    clean, cby = fp8.mx_quantize_reference(block_input(2, 96), fmt)
    assert torch.equal(q[0, :32], clean[0, :32]) and torch.equal(q[0, 64:], clean[0, 64:]) and by[0, 0] == cby[0, 0]
    assert bool(torch.isfinite(fp8.mx_dequantize(q, by)[1]).all())


@pytest.mark.parametrize("fmt", FORMATS)
def test_pack_roundtrip(fmt):
    """All 64 codes in each of the four positions of a 3-byte group (the other three hold the complement code): value i
    sits at bits 6 i .. 6 i + 5 of the little-endian group, rows are padded to 16 bytes behind the view."""
    code = (63 - torch.arange(64)).view(1, 64, 1).repeat(4, 1, 4)
    for pos in range(4):
        code[pos, :, pos] = torch.arange(64)
    code = code.view(256, 4)
    w = code[:, 0] | code[:, 1] << 6 | code[:, 2] << 12 | code[:, 3] << 18
    raw = torch.stack([w & 255, (w >> 8) & 255, w >> 16], 1).to(torch.uint8)
    v = fp8.mx_unpack_fp6(raw, fmt)
    grid = fp8.fp6_grid(fmt).float()
    assert torch.equal(v.abs(), grid[code & 31]) and torch.equal(torch.signbit(v), code >= 32)
    packed = fp8.mx_pack_fp6(v, fmt)
    assert torch.equal(packed, raw) and packed.stride(0) == 16
    assert fp8.mx_pack_fp6(torch.zeros(2, 160), fmt).shape == (2, 120)


def test_arguments():
    """The fp6 formats are MX formats only, built as e2m3 x e2m3 and e3m2 x e2m3, without an fp8 weight gradient."""
    assert fp8.FMT_CODE[fp8.E2M3] == 3 and fp8.FMT_CODE[fp8.E3M2] == 4
    assert fp8.pow2_scale(7.5, fp8.E2M3) == 1.0 and fp8.pow2_scale(7.75, fp8.E2M3) == 0.5
    assert fp8.pow2_scale(28.0, fp8.E3M2) == 1.0 and fp8.pow2_scale(0.5, fp8.E3M2) == 32.0
    assert fp8.Fp8State("mx", fwd="e2m3").fwd == fp8.E2M3
    img = lambda fmt: fp8.MxTensor(torch.zeros(8, 24, dtype=torch.uint8), torch.zeros(8, 4, dtype=torch.uint8), None, None, fmt)
    out = torch.zeros(8, 8, dtype=torch.bfloat16)
    for make in (lambda: fp8.Fp8State("mx", fwd="e2m3", wgrad="mx"), lambda: fp8.Fp8State("current", fwd="e2m3"),
                 lambda: fp8.Fp8State("mx", fwd="e3m2"),
                 lambda: fp8.Fp8Linear(64, 96, scaling="mx", fwd="e2m3", wgrad="mx"),
                 lambda: fp8.quantize_reference(torch.ones(2, 8), fp8.E3M2),
                 lambda: fp8.mx_gemm_into(out, img(fp8.E2M3), img(fp8.E3M2)),
                 lambda: fp8.mx_gemm_into(out, img(fp8.E4M3), img(fp8.E2M3))):
        with pytest.raises(ValueError):
            make()
