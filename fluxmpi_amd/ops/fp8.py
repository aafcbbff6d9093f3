"""fp8 Linear on the gfx950 matrix core: quantise kernels, an fp8 NT GEMM, ``Fp8Linear`` (opt-in).

Scaling is per tensor and a power of two, ``s = 2^floor(log2(FMAX / amax))`` (:func:`pow2_scale`), so scaling
and unscaling are exact and the cast to fp8 is the only rounding. A tensor's scale lives in an 8-word device
block ``{scale, 1 / scale, amax bits, consumed amax, ...}`` (int32 storage, so that ``module.bfloat16()``
leaves it alone); nothing is read back to the host and every launch is HIP-graph capturable.

* :func:`quantize` -> :class:`Fp8Tensor` (``csrc/kernels/fp8_quant.hip``): ``block=None`` is *current*
  scaling (an amax launch, ``fp8_scale_update``, the cast); with a block it casts with the block's stored scale
  while accumulating the tensor's amax, and :func:`scale_update` turns that into the next scale (*delayed*).
* :func:`gemm` (``csrc/kernels/gemm_fp8.hip``): ``a [M, K] x b [N, K]^T`` in fp32 on
  ``v_mfma_f32_16x16x128_f8f6f4``, unscaled and rounded once to bf16, bias in the epilogue.
* :func:`fp8_linear` / :class:`Fp8Linear`: forward ``x`` and ``W`` in e4m3, input gradient ``dy`` in e5m2 against
  ``W``'s transposed image; ``dW`` and ``db`` come from the bf16 kernels of ``ops.linear`` (``wgrad_bgrad``: its
  separate weight-gradient and column-sum calls, not the one-launch ``linbwd.hip`` node, whose input gradient
  this path replaces) on the saved bf16 ``x`` and the bf16 ``dy``, delivered into their bucket slices. Parameters and ``state_dict()`` are ``nn.Linear``'s.
  Whatever :func:`supported` refuses takes ``ops.linear.linear`` unchanged.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from . import _ext
from . import graddst
from .linear import linear, wgrad_bgrad
from .multi_tensor import DTYPE_CODE

E4M3, E5M2 = "e4m3", "e5m2"
E2M1 = "e2m1"  # fp4, the MX entries only (the MX section below)
E2M3, E3M2 = "e2m3", "e3m2"  # fp6, the MX entries only
FMT_CODE = {E4M3: 0, E5M2: 1, E2M1: 2, E2M3: 3, E3M2: 4}
FMAX = {E4M3: 448.0, E5M2: 57344.0, E2M1: 6.0, E2M3: 7.5, E3M2: 28.0}
TOP = {E4M3: 1.75, E5M2: 1.75, E2M1: 1.5, E2M3: 1.875, E3M2: 1.75}  # the significand of FMAX
MX_ONLY = (E2M1, E2M3, E3M2)
TORCH_DTYPE = {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}
BLOCK_WORDS = 8


def _fmt(fmt: str, mx: bool = False) -> str:
    """The format's name checked: ``'e2m1'``, ``'e2m3'`` and ``'e3m2'`` where ``mx`` (the block-scaled entries that
    have fp4 and fp6 kernels) only."""
    if fmt not in FMT_CODE or (fmt in MX_ONLY and not mx):
        names = "'e4m3', 'e5m2', 'e2m1', 'e2m3' or 'e3m2'" if mx else "'e4m3' or 'e5m2'"
        raise ValueError(f"fp8: the format is {names}, got {fmt!r}")
    return fmt


def pow2_scale(amax: float, fmt: str) -> float:
    """``2^floor(log2(FMAX / amax))`` with the exponent kept in -126 .. 126; 1 for an ``amax`` of 0, inf or NaN."""
    amax = float(amax)
    if amax == 0.0 or not math.isfinite(amax):
        return 1.0
    m, e = math.frexp(abs(amax))  # amax = (2 m) 2^(e - 1), 2 m in [1, 2); FMAX = TOP * 2^E
    top = TOP[_fmt(fmt, mx=True)]
    p = int(math.log2(FMAX[fmt] / top)) - (e - 1) - (1 if 2 * m > top else 0)
    return 2.0 ** max(-126, min(126, p))


def quantize_reference(x: torch.Tensor, fmt: str, scale: float | None = None):
    """``(q, scale)`` on the CPU with torch's round-to-nearest-even casts: ``q = cast(clamp(x * scale, +-FMAX))``
    as a float8 tensor, non-finite inputs kept non-finite; ``scale=None``: :func:`pow2_scale` of ``x``'s amax."""
    xf = x.detach().float().cpu()
    if scale is None:
        scale = pow2_scale(float(xf.abs().max()) if xf.numel() else 0.0, fmt)
    y = (xf * scale).clamp(-FMAX[_fmt(fmt)], FMAX[fmt])
    return torch.where(torch.isfinite(xf), y, xf).to(TORCH_DTYPE[fmt]), scale


def new_block(device, scale: float = 1.0) -> torch.Tensor:
    """A scale block (int32 ``[8]``) holding ``scale`` (a power of two) and an empty amax."""
    f = torch.tensor([scale, 1.0 / scale], dtype=torch.float32).view(torch.int32)
    return torch.cat([f, torch.zeros(BLOCK_WORDS - 2, dtype=torch.int32)]).to(device)


@dataclass
class Fp8Tensor:
    """An fp8 image of a bf16 matrix: ``q [R, C]`` and, when asked for, ``q_t [C, R']`` (``R'`` = ``R`` rounded up
    to 16, zero padding), both uint8 bit patterns of ``fmt``, and the device scale block they were cast with.
    Where ``C % 16 != 0``, ``q`` is a view of rows that are zero up to ``C`` rounded up to 16: :func:`gemm` reads
    that padding of both operands."""
    q: torch.Tensor
    q_t: torch.Tensor | None
    block: torch.Tensor
    fmt: str

    def t(self) -> "Fp8Tensor":
        """The transposed image as a GEMM operand."""
        if self.q_t is None:
            raise ValueError("fp8: this tensor was quantised without its transposed image")
        return Fp8Tensor(self.q_t, None, self.block, self.fmt)


def _pad16(n: int) -> int:
    return -(-n // 16) * 16


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def layout_ok(x: torch.Tensor) -> bool:
    """What ``fp8_quantize`` takes: a bf16 matrix with unit column stride, ``C % 8 == 0``, a row stride that is a
    multiple of 8 elements, a 16-byte aligned base."""
    return (x.dim() == 2 and x.dtype == torch.bfloat16 and x.shape[0] >= 1 and x.shape[1] >= 8
            and x.shape[1] % 8 == 0 and x.stride(1) == 1 and x.stride(0) >= x.shape[1] and x.stride(0) % 8 == 0
            and x.data_ptr() % 16 == 0)


def scale_update(block: torch.Tensor, fmt: str) -> None:
    """``fp8_scale_update``: the block's amax becomes its scale (and exact inverse) and is cleared."""
    _ext.get(required=True).fp8_scale_update(block.data_ptr(), FMT_CODE[_fmt(fmt)], _stream(block))


def quantize_into(x, fmt, block, q=None, q_t=None, amax=True) -> None:
    """One ``fp8_quantize`` launch on ``x`` with ``block``'s stored scale into the uint8 views ``q [R, C']`` and
    ``q_t [C, R']`` (``C'``, ``R'``: rounded up to 16, the padding written as zero; each may be None; both None:
    the amax pass alone)."""
    if not (x.is_cuda and layout_ok(x)):
        raise ValueError("fp8.quantize: the input must be a bf16 CUDA matrix with C % 8 == 0, a row stride "
                         "that is a multiple of 8 and a 16-byte aligned base")
    if block.dtype != torch.int32 or block.numel() < BLOCK_WORDS or not block.is_contiguous() or block.device != x.device:
        raise ValueError("fp8.quantize: the scale block is a contiguous int32 tensor of 8 words on the input's device")
    r, c = x.shape
    for o, shape in ((q, (r, _pad16(c))), (q_t, (c, _pad16(r)))):
        if o is not None and (o.dtype != torch.uint8 or tuple(o.shape) != shape or o.stride(1) != 1):
            raise ValueError(f"fp8.quantize: an output must be a uint8 view of shape {shape}")
    _ext.get(required=True).fp8_quantize(
        x.data_ptr(), r, c, x.stride(0), block.data_ptr(), FMT_CODE[_fmt(fmt)],
        q.data_ptr() if q is not None else 0, q.stride(0) if q is not None else 0,
        q_t.data_ptr() if q_t is not None else 0, q_t.stride(0) if q_t is not None else 0, int(amax), _stream(x))


def quantize(x: torch.Tensor, fmt: str, block: torch.Tensor | None = None, transpose: bool = False) -> Fp8Tensor:
    """The fp8 image of the bf16 matrix ``x``. ``block=None``: current scaling in a fresh block (amax pass, scale
    update, cast). With a block: the cast uses its stored scale and accumulates ``x``'s amax into it (delayed
    scaling; :func:`scale_update` then prepares the next scale); values the scale has outgrown saturate."""
    _fmt(fmt)
    if not x.is_cuda or x.dim() != 2:
        raise ValueError("fp8.quantize: the input is a bf16 matrix on the GPU (CPU tensors take quantize_reference)")
    current = block is None
    if current:
        block = torch.zeros(BLOCK_WORDS, dtype=torch.int32, device=x.device)
        quantize_into(x, fmt, block)
        scale_update(block, fmt)
    r, c = x.shape
    q = torch.empty(r, _pad16(c), dtype=torch.uint8, device=x.device)
    q_t = torch.empty(c, _pad16(r), dtype=torch.uint8, device=x.device) if transpose else None
    quantize_into(x, fmt, block, q, q_t, amax=not current)
    return Fp8Tensor(q[:, :c], q_t, block, fmt)


def gemm_into(out: torch.Tensor, a: Fp8Tensor, b: Fp8Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`gemm` into the bf16 view ``out [M, N]`` (any row stride that is a multiple of 8)."""
    m, k = a.q.shape
    n = b.q.shape[0]
    if (a.fmt, b.fmt) not in ((E4M3, E4M3), (E5M2, E4M3)):
        raise ValueError("fp8.gemm: the operands are e4m3 x e4m3 or e5m2 x e4m3")
    # K is walked up to the next multiple of 16: the rows' zero padding (Fp8Tensor; b's columns k .. kp are that of
    # a transposed image; more columns than that is another K)
    kp = _pad16(k)
    if not a.q.is_cuda or not k <= b.q.shape[1] <= kp or min(a.q.stride(0), b.q.stride(0)) < kp or n % 8:
        raise ValueError(f"fp8.gemm: a [M, K] and b [N, K] need N % 8 == 0 and rows padded to K rounded up to 16 on "
                         f"the GPU, got {tuple(a.q.shape)} and {tuple(b.q.shape)}")
    if out.dtype != torch.bfloat16 or tuple(out.shape) != (m, n) or out.stride(1) != 1:
        raise ValueError(f"fp8.gemm: the output must be a bf16 view of shape {(m, n)}")
    if bias is not None:
        bias = bias.detach()
        if bias.dtype not in (torch.bfloat16, torch.float32):
            bias = bias.float()
        bias = bias.contiguous()
        if bias.numel() != n:
            raise ValueError(f"fp8.gemm: the bias must have {n} elements")
    _ext.get(required=True).fp8_gemm(
        a.q.data_ptr(), b.q.data_ptr(), out.data_ptr(), bias.data_ptr() if bias is not None else 0,
        DTYPE_CODE[bias.dtype] if bias is not None else 0, a.block.data_ptr(), b.block.data_ptr(),
        m, n, kp, a.q.stride(0), b.q.stride(0), out.stride(0), FMT_CODE[a.fmt], FMT_CODE[b.fmt], _stream(a.q))
    return out


def gemm(a: Fp8Tensor, b: Fp8Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """``bf16(a b^T / (sa sb) + bias)``: ``a [M, K]`` e4m3 or e5m2, ``b [N, K]`` e4m3, fp32 accumulation."""
    out = torch.empty(a.q.shape[0], b.q.shape[0], dtype=torch.bfloat16, device=a.q.device)
    return gemm_into(out, a, b, bias)


def supported(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """True when :func:`fp8_linear` runs ``x @ weight.T`` in fp8: bf16 on the GPU, both widths multiples of 8
    (each is the N of one GEMM and the K of the other, which the images pad to 16), aligned contiguous storage,
    and a gradient wanted."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and weight.dim() == 2):
        return False
    n_out, n_in = weight.shape
    if x.dim() < 1 or x.shape[-1] != n_in or n_in % 8 or n_out % 8 or x.numel() == 0:
        return False
    if not (torch.is_grad_enabled() and weight.requires_grad):
        return False
    return x.is_contiguous() and weight.is_contiguous() and x.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0


class Fp8State:
    """What an fp8 Linear keeps between calls: the scaling mode, under ``"delayed"`` the three scale blocks
    (``blocks [3, 8]`` int32: x, W, dy; made on first use, scale 1); ``"mx"`` (block scaling, the MX section
    below) keeps nothing and uses no scale block, and ``wgrad="mx"`` runs its weight gradient in fp8 as well
    (:func:`mx_wgrad`; the default ``"bf16"`` is the bf16 kernels). ``W``'s images are NOT kept from one forward
    to the next: the fused optimisers write the parameters through raw pointers and leave ``weight._version``
    alone, so nothing the module can see says that a cached image is still the weight's. A forward casts ``W``
    (two small launches beside the activation's) and hands the images to its own backward."""

    def __init__(self, scaling: str = "current", blocks: torch.Tensor | None = None, wgrad: str = "bf16",
                 fwd: str = E4M3):
        if scaling not in ("current", "delayed", "mx"):
            raise ValueError(f"fp8_linear: scaling must be 'current', 'delayed' or 'mx', got {scaling!r}")
        if wgrad not in ("bf16", "mx"):
            raise ValueError(f"fp8_linear: wgrad must be 'bf16' or 'mx', got {wgrad!r}")
        if wgrad == "mx" and scaling != "mx":
            raise ValueError(f"fp8_linear: wgrad='mx' needs scaling='mx', got scaling={scaling!r}")
        if fwd not in (E4M3, E2M1, E2M3) or (fwd != E4M3 and scaling != "mx"):
            raise ValueError(f"fp8_linear: fwd is 'e4m3', or 'e2m1' or 'e2m3' with scaling='mx', got {fwd!r} with "
                             f"{scaling!r}")
        if fwd != E4M3 and wgrad == "mx":
            raise ValueError(f"fp8_linear: fwd={fwd!r} has no fp8 weight gradient (wgrad='mx' wants an e4m3 token-blocked "
                             "image of x, which this mode does not produce)")
        self.scaling = scaling
        # "e2m1" (MX only): x and W in fp4 for the forward, dy e4m3 against W's packed transposed image; "e2m3" (MX only):
        # x and W in fp6 e2m3, dy in fp6 e3m2 against W's packed transposed image
        self.fwd = fwd
        self.blocks = blocks
        self.wgrad = wgrad  # "mx": the weight gradient in block-scaled fp8 too (mx_wgrad.hip), T % 32 == 0

    def block(self, i: int, device):
        if self.scaling == "current":
            return None
        if self.blocks is None or self.blocks.device != device:
            self.blocks = torch.stack([new_block(device) for _ in range(3)])
        return self.blocks[i]

    def image(self, x2: torch.Tensor, fmt: str, i: int, transpose: bool = False) -> Fp8Tensor:
        """Delayed scaling prepares this step's scale from the previous step's amax, then casts with it."""
        blk = self.block(i, x2.device)
        if blk is not None:
            scale_update(blk, fmt)
        return quantize(x2, fmt, blk, transpose)



class _Fp8LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, state):
        n_out, n_in = weight.shape
        wq = state.image(weight.detach(), E4M3, 1, transpose=True)
        xq = state.image(x.view(-1, n_in), E4M3, 0)
        ctx.save_for_backward(x, weight)
        ctx.state, ctx.wq, ctx.bias = state, wq, bias  # the bias leaf itself: its bucket slice
        return gemm(xq, wq, bias).view(*x.shape[:-1], n_out)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        n_out, n_in = w.shape
        dy2 = dy.reshape(-1, n_out)
        if dy2.dtype != torch.bfloat16 or not dy2.is_contiguous() or dy2.data_ptr() % 16:
            dy2 = dy2.to(torch.bfloat16).contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = gemm(ctx.state.image(dy2, E5M2, 2), ctx.wq.t()).view(x.shape)
        # dW and db: the bf16 kernels on the bf16 x and dy, as _LinearFn's separate calls
        need_b = ctx.bias is not None and ctx.needs_input_grad[2]
        dw, db = wgrad_bgrad(x.reshape(-1, n_in), w, ctx.bias, dy2, ctx.needs_input_grad[1], need_b)
        return dx, dw, db, None


def fp8_linear(x, weight, bias=None, state: Fp8State | None = None) -> torch.Tensor:
    """``F.linear`` with the forward and the input gradient in fp8 (see the module); ``state=None`` is stateless
    current scaling. Unsupported input (:func:`supported`) takes ``ops.linear.linear``."""
    state = state if state is not None else Fp8State()
    if state.scaling == "mx":
        if not mx_supported(x, weight):
            return linear(x, weight, bias)
        return _MxLinearFn.apply(x, weight, bias,
                                 state.wgrad == "mx" and (x.numel() // weight.shape[1]) % MX_BLOCK == 0, state.fwd)
    if not supported(x, weight):
        return linear(x, weight, bias)
    return _Fp8LinearFn.apply(x, weight, bias, state)


class Fp8Linear(torch.nn.Linear):
    """Drop-in for ``ops.linear.Linear``: same parameters and ``state_dict()``; the weight stays bf16 and the
    fp8 images are per-step scratch. ``scaling="delayed"`` keeps its three scale blocks in a non-persistent
    buffer; ``scaling="mx"`` is block scaling (``mx_quant.hip``, ``mx_gemm.hip``) where :func:`mx_supported`, and
    with ``wgrad="mx"`` the weight gradient runs in fp8 too (``mx_wgrad.hip``) where the token count is a multiple
    of 32; ``fwd="e2m1"`` (with ``scaling="mx"``) runs the forward on fp4 images of ``x`` and ``W`` and the input
    gradient on e4m3 ``dy`` against ``W``'s fp4 transposed image (``mx4_quant.hip``, ``mx4_gemm.hip``); ``fwd="e2m3"``
    runs both on fp6: ``x`` and both images of ``W`` in e2m3, ``dy`` in e3m2 (``mx6_quant.hip``, ``mx6_gemm.hip``)."""

    def __init__(self, in_features, out_features, bias=True, scaling="current", wgrad="bf16", fwd=E4M3, **kw):
        super().__init__(in_features, out_features, bias=bias, **kw)
        self.fp8 = Fp8State(scaling, wgrad=wgrad, fwd=fwd)
        self.register_buffer("fp8_blocks", torch.stack([new_block("cpu") for _ in range(3)]), persistent=False)

    def forward(self, x):
        if self.fp8.scaling == "mx":
            return fp8_linear(x, self.weight, self.bias, self.fp8)
        if not supported(x, self.weight):
            return linear(x, self.weight, self.bias)
        self.fp8.blocks = self.fp8_blocks  # follows .to(device)
        return _Fp8LinearFn.apply(x, self.weight, self.bias, self.fp8)


def fp8_linear_reference(x, w, b, dy, scales=None):
    """``(y, dx, |y|, |dx|)`` in float64 on the CPU of the same quantisation: x, w in e4m3 and dy in e5m2 with
    :func:`pow2_scale` of each tensor (or ``scales = (sx, sw, sdy)``), then float64 products of the dequantised
    values; the last two are the same products of absolute values (what an error bound scales with)."""
    sx, sw, sdy = scales if scales is not None else (None, None, None)
    n_in = w.shape[1]
    deq = []
    for t, fmt, s in ((x.reshape(-1, n_in), E4M3, sx), (w, E4M3, sw), (dy.reshape(-1, w.shape[0]), E5M2, sdy)):
        q, s = quantize_reference(t, fmt, s)
        deq.append(q.double() / s)
    xd, wd, dyd = deq
    bd = b.detach().double().cpu() if b is not None else torch.zeros(w.shape[0], dtype=torch.float64)
    y, ya = xd @ wd.t() + bd, xd.abs() @ wd.abs().t() + bd.abs()
    return y, dyd @ wd, ya, dyd.abs() @ wd.abs()


# ---------------------------------------------------------------------------------------------------- MX
# Block scaling (OCP MX): one :func:`pow2_scale` per MX_BLOCK consecutive elements along the reduction axis of
# the GEMM that reads the image, stored as the E8M0 byte of its inverse, ``127 - log2(s)`` (1 .. 253; 127 for an
# all-zero or non-finite block). ``csrc/kernels/mx_quant.hip`` casts in ONE launch with no amax pass, no scale
# block and no state; ``mx_gemm.hip`` applies the scales inside ``v_mfma_scale_f32_16x16x128_f8f6f4``.
#
# ``'e2m1'`` (fp4: +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, no inf or NaN) is packed two values per byte, element ``2 i`` in the
# low nibble of byte ``i``: ``q`` is ``[R, C / 2]``, the scale images are the same. Its scale follows the same
# non-saturating rule with the format's top significand 1.5 (a valid MX scale, not the OCP document's floor rule); a
# block with an inf or NaN is zeros under the byte 255. ``mx4_quant.hip`` / ``mx4_gemm.hip``; pairs e2m1 x e2m1 and
# e4m3 x e2m1.
MX_BLOCK = 32
MX_ONE = 127
MX_NAN = 255  # E8M0's NaN: an e2m1 block that held a non-finite value
MX4_STAGES = 2  # LDS stages of mx4_gemm.hip, each 256 values of K deep
MX6_STAGES = 2  # LDS stages of mx6_gemm.hip, each MX6_STAGE_K values of K deep
MX6_STAGE_K = 128
MX_PAIRS = ((E4M3, E4M3), (E5M2, E4M3), (E2M1, E2M1), (E4M3, E2M1), (E2M3, E2M3), (E3M2, E2M3))  # what mx_gemm builds, a x b
FP4_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # code = sign << 3 | index
# ``'e2m3'`` / ``'e3m2'`` (OCP FP6, no inf or NaN; code = sign << 5 | exponent << MB | mantissa) are packed four values in
# three bytes: value ``i`` of a 32-value block at bits ``6 i .. 6 i + 5`` of the block's 24 bytes read as one little-endian
# bit string, the order the scaled MFMA reads (``mx6_gemm.hip``). ``q`` is ``[R, 3 C / 4]``, a view of rows rounded up to
# 16 bytes (the kernels' row strides are multiples of 16). Scale rule and the byte 255 as e2m1. ``mx6_quant.hip`` /
# ``mx6_gemm.hip``; pairs e2m3 x e2m3 and e3m2 x e2m3.
FP6_BITS = {E2M3: (3, 1), E3M2: (2, 3)}  # mantissa bits, exponent bias


def fp6_grid(fmt: str) -> torch.Tensor:
    """The 32 magnitudes of ``fmt`` by code (float64, increasing)."""
    mb, bias = FP6_BITS[fmt]
    c = torch.arange(32, dtype=torch.float64)
    e, m = torch.div(c, 2 ** mb, rounding_mode="floor"), c % 2 ** mb
    return torch.where(e == 0, m * 2.0 ** (1 - bias - mb), (1 + m / 2 ** mb) * 2.0 ** (e - bias))


def _cols(fmt: str, k: int) -> int:
    """Bytes of ``k`` values of ``fmt``."""
    return k // 2 if fmt == E2M1 else (k // 4 * 3 if fmt in FP6_BITS else k)


def _values(fmt: str, cols: int) -> int:
    """:func:`_cols` inverted."""
    return cols * 2 if fmt == E2M1 else (cols // 3 * 4 if fmt in FP6_BITS else cols)


def _rows16(r: int, cols: int, device=None) -> torch.Tensor:
    """uint8 zeros ``[r, cols]`` as a view of rows rounded up to 16 bytes."""
    return torch.zeros(r, _pad16(cols), dtype=torch.uint8, device=device)[:, :cols]


def mx_pack_fp6(values: torch.Tensor, fmt: str) -> torch.Tensor:
    """Grid values ``[R, C]`` (float, ``C % 4 == 0``) of ``fmt`` as packed codes uint8 ``[R, 3 C / 4]`` (a view of rows
    rounded up to 16 bytes): codes ``c0 .. c3`` of four values are the 24-bit little-endian string ``c0 | c1 << 6 |
    c2 << 12 | c3 << 18``."""
    v = values.detach().double()
    code = torch.bucketize(v.abs(), fp6_grid(fmt).to(v.device)) | (torch.signbit(v).long() << 5)
    w = code[:, 0::4] | (code[:, 1::4] << 6) | (code[:, 2::4] << 12) | (code[:, 3::4] << 18)
    out = _rows16(v.shape[0], _cols(fmt, v.shape[1]), v.device)
    out.copy_(torch.stack([w & 255, (w >> 8) & 255, w >> 16], -1).reshape(v.shape[0], -1))
    return out


def mx_unpack_fp6(q: torch.Tensor, fmt: str) -> torch.Tensor:
    """Packed codes uint8 ``[R, 3 C / 4]`` as their float32 values ``[R, C]``."""
    b = q.long().reshape(q.shape[0], -1, 3)
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    code = torch.stack([(w >> s) & 63 for s in (0, 6, 12, 18)], -1).reshape(q.shape[0], -1)
    v = fp6_grid(fmt).float().to(q.device)[code & 31]
    return torch.where((code & 32) != 0, -v, v)


def _round_fp6(y: torch.Tensor, fmt: str) -> torch.Tensor:
    """``y`` (float32, ``|y| <= FMAX``) to the grid of ``fmt``: the spacing at ``|y|``'s exponent (the subnormal step
    below the smallest normal), then ``torch.round``, which takes a midpoint to the even multiple."""
    mb, bias = FP6_BITS[fmt]
    _, ex = torch.frexp(y.abs())  # |y| = m 2^ex, m in [0.5, 1): the exponent is ex - 1
    step = torch.ldexp(torch.ones_like(y), (ex - 1).clamp(min=1 - bias) - mb)
    return torch.copysign(torch.round(y.abs() / step) * step, y)


def mx_pack_fp4(values: torch.Tensor) -> torch.Tensor:
    """Grid values ``[R, C]`` (float) as packed codes uint8 ``[R, C / 2]``, element ``2 i`` in the low nibble."""
    v = values.detach().double()
    code = torch.bucketize(v.abs(), torch.tensor(FP4_GRID, dtype=torch.float64)) | (torch.signbit(v).long() << 3)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8)


def mx_unpack_fp4(q: torch.Tensor) -> torch.Tensor:
    """Packed codes uint8 ``[R, C / 2]`` as their float32 values ``[R, C]``."""
    code = torch.stack([q & 15, q >> 4], -1).reshape(q.shape[0], -1).long()
    v = torch.tensor(FP4_GRID, dtype=torch.float32, device=q.device)[code & 7]
    return torch.where((code & 8) != 0, -v, v)


def _round_fp4(y: torch.Tensor) -> torch.Tensor:
    """``y`` (float32, ``|y| <= 6``) to the e2m1 grid: nearest, a midpoint to the neighbour with the even code."""
    a = y.abs()
    mids = ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False))
    idx = sum(((a >= m) if up else (a > m)).long() for m, up in mids)
    return torch.copysign(torch.tensor(FP4_GRID, dtype=torch.float32)[idx], y)


def mx_scale_cols(k: int) -> int:
    """Bytes of a scale-image row for a reduction length ``k``: a dword per 128 elements."""
    return 4 * (-(-k // 128))


@dataclass
class MxTensor:
    """An MX image of a bf16 matrix ``[R, C]``: ``q [R, C]`` uint8 bit patterns of ``fmt`` with ``scales
    [R, 4 ceil(C / 128)]`` (the ``C / 32`` block bytes of a row, then 127), blocks along ``C``; and, when asked for,
    ``q_t [C, R]`` with ``scales_t [C, 4 ceil(R / 128)]``, blocks along ``R``: an image of its own, not ``q``'s
    transpose."""
    q: torch.Tensor
    scales: torch.Tensor
    q_t: torch.Tensor | None
    scales_t: torch.Tensor | None
    fmt: str  # 'e2m1': q and q_t are packed, [R, C / 2] and [C, R / 2]; 'e2m3' / 'e3m2': [R, 3 C / 4] and [C, 3 R / 4]

    def t(self) -> "MxTensor":
        """The transposed image as a GEMM operand."""
        if self.q_t is None:
            raise ValueError("fp8.mx: this tensor was quantised without its transposed image")
        return MxTensor(self.q_t, self.scales_t, None, None, self.fmt)


def mx_quantize_reference(x: torch.Tensor, fmt: str):
    """``(q, bytes)`` on the CPU: ``q`` float8 ``[R, C]`` and the blocks' E8M0 bytes uint8 ``[R, C / 32]``, blocks
    along the last axis; :func:`pow2_scale` of every block's amax (vectorised with ``torch.frexp``), torch's
    round-to-nearest-even cast, non-finite inputs kept non-finite in a block of scale 1. ``'e2m1'``: ``q`` is float32
    values on the fp4 grid (:func:`mx_pack_fp4` packs them), and a block with a non-finite input is zeros under the
    byte 255; ``'e2m3'`` / ``'e3m2'`` likewise on the fp6 grids (:func:`mx_pack_fp6`)."""
    xf = x.detach().float().cpu()
    r, c = xf.shape
    if c % MX_BLOCK:
        raise ValueError(f"fp8.mx: the blocked axis must be a multiple of {MX_BLOCK}, got {c}")
    blk = xf.view(r, c // MX_BLOCK, MX_BLOCK)
    amax = blk.abs().amax(-1)
    ok = torch.isfinite(amax) & (amax > 0)
    m, e = torch.frexp(torch.where(ok, amax, torch.ones_like(amax)))  # amax = (2 m) 2^(e - 1), 2 m in [1, 2)
    top = TOP[_fmt(fmt, mx=True)]
    p = int(math.log2(FMAX[fmt] / top)) - (e - 1) - (2 * m > top).int()
    p = torch.where(ok, p.clamp(-126, 126), torch.zeros_like(p))
    y = (blk * torch.ldexp(torch.ones_like(amax), p).unsqueeze(-1)).clamp(-FMAX[fmt], FMAX[fmt])
    if fmt in MX_ONLY:
        bad = ~torch.isfinite(amax)
        y = torch.where(bad.unsqueeze(-1), torch.zeros_like(y), _round_fp4(y) if fmt == E2M1 else _round_fp6(y, fmt))
        return y.view(r, c), torch.where(bad, torch.full_like(p, MX_NAN), MX_ONE - p).to(torch.uint8)
    return torch.where(torch.isfinite(blk), y, blk).view(r, c).to(TORCH_DTYPE[fmt]), (MX_ONE - p).to(torch.uint8)


def mx_dequantize(q: torch.Tensor, block_bytes: torch.Tensor) -> torch.Tensor:
    """float64 values of a reference image: ``q 2^(byte - 127)`` block by block (exact)."""
    return q.double() * torch.ldexp(torch.ones(1, dtype=torch.float64),
                                    block_bytes.int() - MX_ONE).repeat_interleave(MX_BLOCK, 1)


def mx_scale_image(block_bytes: torch.Tensor) -> torch.Tensor:
    """Block bytes ``[R, C / 32]`` as a scale image ``[R, 4 ceil(C / 128)]``, padded with 127."""
    r, nb = block_bytes.shape
    out = torch.full((r, mx_scale_cols(nb * MX_BLOCK)), MX_ONE, dtype=torch.uint8, device=block_bytes.device)
    out[:, :nb] = block_bytes
    return out


def mx_layout_ok(x: torch.Tensor) -> bool:
    """What ``mx_quantize`` takes: a bf16 matrix with unit column stride, ``C % 32 == 0``, a row stride that is a
    multiple of 8 elements, a 16-byte aligned base."""
    return (x.dim() == 2 and x.dtype == torch.bfloat16 and x.shape[0] >= 1 and x.shape[1] >= MX_BLOCK
            and x.shape[1] % MX_BLOCK == 0 and x.stride(1) == 1 and x.stride(0) >= x.shape[1]
            and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0)


def mx_quantize_into(x, fmt, q=None, scales=None, q_t=None, scales_t=None) -> None:
    """One ``mx_quantize`` launch on ``x [R, C]`` into the uint8 views ``q [R, C]`` with ``scales`` and / or
    ``q_t [C, R]`` with ``scales_t`` (each pair may be None; shapes as :class:`MxTensor`)."""
    if not (x.is_cuda and mx_layout_ok(x)):
        raise ValueError("fp8.mx_quantize: the input must be a bf16 CUDA matrix with C % 32 == 0, a row stride "
                         "that is a multiple of 8 and a 16-byte aligned base")
    r, c = x.shape
    if q_t is not None and r % MX_BLOCK:
        raise ValueError(f"fp8.mx_quantize: the transposed image needs R % {MX_BLOCK} == 0, got R = {r}")
    _fmt(fmt, mx=True)
    for o, shape in ((q, (r, _cols(fmt, c))), (scales, (r, mx_scale_cols(c))), (q_t, (c, _cols(fmt, r))),
                     (scales_t, (c, mx_scale_cols(r)))):
        if o is not None and (o.dtype != torch.uint8 or tuple(o.shape) != shape or o.stride(1) != 1):
            raise ValueError(f"fp8.mx_quantize: an output must be a uint8 view of shape {shape}")
    if (q is None) != (scales is None) or (q_t is None) != (scales_t is None) or (q is None and q_t is None):
        raise ValueError("fp8.mx_quantize: an image and its scales come together, and one pair is needed")
    arg = lambda o: (o.data_ptr(), o.stride(0)) if o is not None else (0, 0)
    _ext.mx().mx_quantize(x.data_ptr(), r, c, x.stride(0), FMT_CODE[fmt], *arg(q), *arg(scales), *arg(q_t),
                          *arg(scales_t), _stream(x))


def mx_quantize(x: torch.Tensor, fmt: str, transpose: bool = False) -> MxTensor:
    """The MX image of the bf16 matrix ``x`` in one launch; ``transpose``: the image blocked along ``R`` too. fp6 images
    are views of rows rounded up to 16 bytes (``3 C / 4`` is not always a multiple of 16, the row stride must be)."""
    _fmt(fmt, mx=True)
    if not x.is_cuda or x.dim() != 2:
        raise ValueError("fp8.mx_quantize: the input is a bf16 matrix on the GPU (CPU tensors take "
                         "mx_quantize_reference)")
    r, c = x.shape
    new = lambda *s: torch.empty(*s, dtype=torch.uint8, device=x.device)
    img = lambda rows, cols: new(rows, _pad16(cols))[:, :cols] if cols % 16 else new(rows, cols)
    t = MxTensor(img(r, _cols(fmt, c)), new(r, mx_scale_cols(c)), img(c, _cols(fmt, r)) if transpose else None,
                 new(c, mx_scale_cols(r)) if transpose else None, fmt)
    mx_quantize_into(x, fmt, t.q, t.scales, t.q_t, t.scales_t)
    return t


def mx_gemm_into(out: torch.Tensor, a: MxTensor, b: MxTensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`mx_gemm` into the bf16 view ``out [M, N]`` (any row stride that is a multiple of 8)."""
    if (a.fmt, b.fmt) not in MX_PAIRS:
        raise ValueError("fp8.mx_gemm: the operands are e4m3 x e4m3, e5m2 x e4m3, e2m1 x e2m1, e4m3 x e2m1, e2m3 x e2m3 "
                         "or e3m2 x e2m3")
    m, n = a.q.shape[0], b.q.shape[0]
    k = _values(a.fmt, a.q.shape[1])  # values: an e2m1 or fp6 image is packed
    if not a.q.is_cuda or a.q.shape[1] != _cols(a.fmt, k) or b.q.shape[1] != _cols(b.fmt, k) or k % MX_BLOCK or n % 8:
        raise ValueError(f"fp8.mx_gemm: a [M, K] and b [N, K] on the GPU need K % 32 == 0 and N % 8 == 0 (an e2m1 image "
                         f"has K / 2 columns, an fp6 one 3 K / 4), got {tuple(a.q.shape)} and {tuple(b.q.shape)}")
    for t, rows in ((a, m), (b, n)):
        if t.scales.dtype != torch.uint8 or t.scales.shape[0] != rows or t.scales.shape[1] < mx_scale_cols(k):
            raise ValueError(f"fp8.mx_gemm: a scale image must be uint8 [{rows}, >= {mx_scale_cols(k)}]")
    if out.dtype != torch.bfloat16 or tuple(out.shape) != (m, n) or out.stride(1) != 1:
        raise ValueError(f"fp8.mx_gemm: the output must be a bf16 view of shape {(m, n)}")
    if bias is not None:
        bias = bias.detach()
        if bias.dtype not in (torch.bfloat16, torch.float32):
            bias = bias.float()
        bias = bias.contiguous()
        if bias.numel() != n:
            raise ValueError(f"fp8.mx_gemm: the bias must have {n} elements")
    _ext.mx().mx_gemm(
        a.q.data_ptr(), b.q.data_ptr(), out.data_ptr(), bias.data_ptr() if bias is not None else 0,
        DTYPE_CODE[bias.dtype] if bias is not None else 0, a.scales.data_ptr(), b.scales.data_ptr(), m, n, k,
        a.q.stride(0), b.q.stride(0), out.stride(0), a.scales.stride(0), b.scales.stride(0), FMT_CODE[a.fmt],
        FMT_CODE[b.fmt], _stream(a.q))
    return out


def mx_gemm(a: MxTensor, b: MxTensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """``bf16(sum over K blocks of the dequantised a_blk . b_blk + bias)``: ``a [M, K]`` e4m3 or e5m2 with ``b [N, K]``
    e4m3, or ``a`` e2m1 or e4m3 with ``b`` e2m1 (``mx4_gemm.hip``), or ``a`` e2m3 or e3m2 with ``b`` e2m3
    (``mx6_gemm.hip``); the block scales applied inside the MFMA, fp32
    accumulation."""
    out = torch.empty(a.q.shape[0], b.q.shape[0], dtype=torch.bfloat16, device=a.q.device)
    return mx_gemm_into(out, a, b, bias)


def mx_supported(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """:func:`supported` with both widths multiples of 32 (each is the blocked axis of one GEMM)."""
    return supported(x, weight) and weight.shape[0] % MX_BLOCK == 0 and weight.shape[1] % MX_BLOCK == 0


def mx_wgrad_splits(m: int, n: int, k: int, cus: int) -> int:
    """The default split count, ``wgrad256``'s rule: one round of resident workgroups, floor and not ceil (a second,
    partial round costs a whole one), at most one split per 128-byte K tile."""
    C = _ext.mx()
    tile = C.MX_WGRAD_TILE
    tiles = -(-m // tile) * (-(-n // tile))
    return max(1, min(cus * C.MX_WGRAD_PER_CU // tiles, -(-k // 128)))


def mx_wgrad(a_t: MxTensor, b_t: MxTensor, out_dtype: torch.dtype = torch.float32,
             splits: int | None = None) -> torch.Tensor:
    """``[M, N]``: the sum over K blocks of the dequantised ``a_t [M, K]`` (e4m3 or e5m2) times ``b_t [N, K]`` (e4m3)
    blocks, i.e. a Linear's ``dW`` from the transposed images of ``dy`` and ``x`` (``K`` = tokens). ``mx_wgrad.hip``
    writes fp32 partials of ``splits`` token ranges (default :func:`mx_wgrad_splits`; the kernel clamps it to the
    number of K tiles) and ``gemm_splitk_reduce`` sums them in order into ``graddst.empty``: under
    ``graddst.into(weight)`` the gradient lands in the bucket slice; bit-identical run to run."""
    m, k = a_t.q.shape
    n = b_t.q.shape[0]
    if (a_t.fmt, b_t.fmt) not in ((E4M3, E4M3), (E5M2, E4M3)):
        raise ValueError("fp8.mx_wgrad: the operands are e4m3 x e4m3 or e5m2 x e4m3")
    if not a_t.q.is_cuda or b_t.q.shape[1] != k or k % MX_BLOCK or n % 8:
        raise ValueError(f"fp8.mx_wgrad: a_t [M, K] and b_t [N, K] on the GPU need K % 32 == 0 and N % 8 == 0, got "
                         f"{tuple(a_t.q.shape)} and {tuple(b_t.q.shape)}")
    for t, rows in ((a_t, m), (b_t, n)):
        if t.scales.dtype != torch.uint8 or t.scales.shape[0] != rows or t.scales.shape[1] < mx_scale_cols(k):
            raise ValueError(f"fp8.mx_wgrad: a scale image must be uint8 [{rows}, >= {mx_scale_cols(k)}]")
    C, dev = _ext.mx(), a_t.q.device
    if splits is None:
        splits = mx_wgrad_splits(m, n, k, torch.cuda.get_device_properties(dev).multi_processor_count)
    s = C.mx_wgrad_splits(k, splits)
    ws = torch.empty(s, m, n, device=dev, dtype=torch.float32)
    stream = _stream(a_t.q)
    C.mx_wgrad(a_t.q.data_ptr(), b_t.q.data_ptr(), ws.data_ptr(), a_t.scales.data_ptr(), b_t.scales.data_ptr(), m, n, k,
               a_t.q.stride(0), b_t.q.stride(0), a_t.scales.stride(0), b_t.scales.stride(0), FMT_CODE[a_t.fmt],
               FMT_CODE[b_t.fmt], s, stream)
    odt = out_dtype if out_dtype in (torch.float32, torch.bfloat16) else torch.float32
    dw = graddst.empty((m, n), odt, dev)
    _ext.get(required=True).gemm_splitk_reduce(ws.data_ptr(), s, dw.numel(), dw.data_ptr(), DTYPE_CODE[odt], stream)
    return dw.to(out_dtype)


def mx_wgrad_reference(dy, x, fmt: str = E4M3):
    """``(dW, |dW|)`` in float64 on the CPU of the same quantisation: ``dy.t()`` (``fmt``) and ``x.t()`` (e4m3) blocked
    along the tokens, dequantised, then multiplied; the second is the product of absolute values."""
    dyd = mx_dequantize(*mx_quantize_reference(dy.detach().reshape(-1, dy.shape[-1]).t().contiguous(), fmt))
    xd = mx_dequantize(*mx_quantize_reference(x.detach().reshape(-1, x.shape[-1]).t().contiguous(), E4M3))
    return dyd @ xd.t(), dyd.abs() @ xd.abs().t()


class _MxLinearFn(torch.autograd.Function):
    """x, W and dy all in e4m3 (the OCP / Transformer Engine recipe: with a scale per 32 values e5m2's range is
    not needed); W's two images come from one launch in every forward (:class:`Fp8State` says why). ``fp8_wgrad``
    (``wgrad="mx"`` and a token count that is a multiple of 32): x and dy are cast with their token-blocked images in
    the same launches, the backward keeps x's instead of the bf16 x, and dW is :func:`mx_wgrad` of the two.
    ``fwd="e2m1"``: x and W are cast to fp4 instead (W's transposed image packed along ``n_out``), dy stays e4m3.
    ``fwd="e2m3"``: x and W are cast to fp6 e2m3 and dy to e3m2, a homogeneous fp6 pair in both GEMMs."""

    @staticmethod
    def forward(ctx, x, weight, bias, fp8_wgrad=False, fwd=E4M3):
        n_out, n_in = weight.shape
        wq = mx_quantize(weight.detach(), fwd, transpose=True)
        xq = mx_quantize(x.view(-1, n_in), fwd, transpose=fp8_wgrad)
        if fp8_wgrad:
            ctx.save_for_backward(weight, xq.q_t, xq.scales_t)
        else:
            ctx.save_for_backward(x, weight)
        ctx.wq, ctx.bias, ctx.fp8_wgrad, ctx.x_shape = wq, bias, fp8_wgrad, x.shape
        ctx.dy_fmt = E3M2 if fwd == E2M3 else E4M3
        return mx_gemm(xq, wq, bias).view(*x.shape[:-1], n_out)

    @staticmethod
    def backward(ctx, dy):
        w = ctx.saved_tensors[0] if ctx.fp8_wgrad else ctx.saved_tensors[1]
        n_out, n_in = w.shape
        dy2 = dy.reshape(-1, n_out)
        if dy2.dtype != torch.bfloat16 or not dy2.is_contiguous() or dy2.data_ptr() % 16:
            dy2 = dy2.to(torch.bfloat16).contiguous()
        need_b = ctx.bias is not None and ctx.needs_input_grad[2]
        dx = None
        if not ctx.fp8_wgrad:
            if ctx.needs_input_grad[0]:
                dx = mx_gemm(mx_quantize(dy2, ctx.dy_fmt), ctx.wq.t()).view(ctx.x_shape)
            dw, db = wgrad_bgrad(ctx.saved_tensors[0].reshape(-1, n_in), w, ctx.bias, dy2, ctx.needs_input_grad[1], need_b)
            return dx, dw, db, None, None
        # one cast of dy: the row-wise image feeds dx, the token-blocked one dW
        dyq = mx_quantize(dy2, E4M3, transpose=ctx.needs_input_grad[1])
        if ctx.needs_input_grad[0]:
            dx = mx_gemm(dyq, ctx.wq.t()).view(ctx.x_shape)
        dw = db = None
        if ctx.needs_input_grad[1]:
            _, xq_t, xs_t = ctx.saved_tensors
            with graddst.into(w):
                dw = mx_wgrad(dyq.t(), MxTensor(xq_t, xs_t, None, None, E4M3), w.dtype)
        # db as the default path takes it (bias_grad where ops.linear.native_ok): the bf16 x is gone, and dy2 has
        # its rows and layout, which is all that wgrad_bgrad asks of it when no dW is wanted
        _, db = wgrad_bgrad(dy2, w, ctx.bias, dy2, False, need_b)
        return dx, dw, db, None, None


def mx_linear_reference(x, w, b, dy, fwd: str = E4M3):
    """``(y, dx, |y|, |dx|)`` in float64 on the CPU of the same quantisation, as :func:`fp8_linear_reference`: x and
    w blocked along ``n_in`` for y, dy and w blocked along ``n_out`` for dx; x and both images of w in ``fwd``, dy in
    e4m3 (e3m2 with ``fwd="e2m3"``)."""
    n_out, n_in = w.shape
    xd, wd, dyd, wtd = (mx_dequantize(*mx_quantize_reference(t, f)) for t, f in
                        ((x.reshape(-1, n_in), fwd), (w, fwd), (dy.reshape(-1, n_out), E3M2 if fwd == E2M3 else E4M3),
                         (w.detach().t().contiguous(), fwd)))
    bd = b.detach().double().cpu() if b is not None else torch.zeros(n_out, dtype=torch.float64)
    y, ya = xd @ wd.t() + bd, xd.abs() @ wd.abs().t() + bd.abs()
    return y, dyd @ wtd.t(), ya, dyd.abs() @ wtd.abs().t()


__all__ = ["E4M3", "E5M2", "E2M1", "E2M3", "E3M2", "FMAX", "mx_pack_fp4", "mx_unpack_fp4", "mx_pack_fp6", "mx_unpack_fp6", "Fp8Tensor", "Fp8State", "Fp8Linear", "fp8_linear", "fp8_linear_reference",
           "quantize", "quantize_into", "quantize_reference", "pow2_scale", "scale_update", "new_block", "gemm",
           "gemm_into", "supported", "layout_ok", "MX_BLOCK", "MxTensor", "mx_quantize", "mx_quantize_into",
           "mx_quantize_reference", "mx_dequantize", "mx_scale_image", "mx_gemm", "mx_gemm_into", "mx_supported",
           "mx_linear_reference", "mx_wgrad", "mx_wgrad_splits", "mx_wgrad_reference"]
