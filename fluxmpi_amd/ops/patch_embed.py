"""ViT patch embedding as one implicit GEMM on the input pipeline's NHWC batch.

``patch_embed(x, weight, bias, cls, pos, patch)`` is ``cat([cls, unfold(x) @ weight.T + bias], 1) + pos``
for a ``channels_last`` bf16 batch ``x [B, C, H, W]`` with 3 or 4 channels (the fourth, the input
pipeline's pad channel, does not reach the output): ``csrc/kernels/patch_embed.hip`` reads the patches
straight from the image, writes the token buffer ``[B, n + 1, D]`` once (bias, position embedding and the
``[CLS]`` row in the epilogue) and takes the filter gradient from the same image and from ``dy`` in place.
No patch matrix exists in either direction. The filter stays the parameter ``[D, 3 p p]`` in ``(c, i, j)``
order; it is re-packed to the kernel's ``(i, j, c)`` order by a streaming kernel every forward.

The backward's three small reductions (``dpos``, ``dcls``, ``dbias``) come from ONE fp32 batch sum of
``dy`` in PyTorch; every gradient is delivered into its DDP bucket slice where ``ops/graddst`` has one.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _ext
from . import graddst
from .multi_tensor import DTYPE_CODE

# workgroups the weight gradient's split-K aims at (64 x 64 tiles, several per compute unit)
WGRAD_TARGET = 1024
# the split count the node asks for instead (None: from WGRAD_TARGET); the tests walk several 64-token
# steps per workgroup at small shapes with it
WGRAD_SPLITS: int | None = None


def layout_ok(x: torch.Tensor, patch: int, dim: int) -> bool:
    """The limits of ``patch_embed.hip`` that do not depend on the device: a bf16 ``[B, C, H, W]`` batch
    with NHWC (``channels_last``) memory, 3 or 4 channels, 16-byte-aligned base, whole 16-byte chunks
    per patch row, sides that are multiples of the patch, a sample below 2^31 bytes, ``dim % 64 == 0``."""
    if x.dim() != 4 or x.dtype != torch.bfloat16 or x.shape[0] < 1:
        return False
    b, c, h, w = x.shape
    if c not in (3, 4) or patch < 1 or patch > 512 or (patch * c) % 8 or (patch * patch * c) % 64:
        return False
    if h < patch or w < patch or h % patch or w % patch or h * w * c * 2 >= 2 ** 31:
        return False
    if dim < 64 or dim % 64 or b * ((h // patch) * (w // patch) + 1) >= 2 ** 31 - 1024:
        return False
    return x.permute(0, 2, 3, 1).is_contiguous() and x.data_ptr() % 16 == 0


def supported(x: torch.Tensor, patch: int, dim: int) -> bool:
    """True when :func:`patch_embed` takes ``x`` as it is (on the GPU, see :func:`layout_ok`)."""
    return x.is_cuda and layout_ok(x, patch, dim)


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def pack_weight(weight: torch.Tensor, patch: int, channels: int) -> torch.Tensor:
    """``[D, 3 p p]`` in ``(c, i, j)`` order -> ``[D, p p C]`` in ``(i, j, c)`` order (``patch_weight_pack``)."""
    d = weight.shape[0]
    if weight.dtype != torch.bfloat16 or tuple(weight.shape) != (d, 3 * patch * patch) or not weight.is_contiguous():
        raise ValueError("patch_embed: the filter must be a contiguous bf16 [D, 3 p p] matrix")
    wp = torch.empty(d, patch * patch * channels, device=weight.device, dtype=torch.bfloat16)
    _ext.get(required=True).patch_weight_pack(weight.data_ptr(), wp.data_ptr(), d, patch, channels, _stream(weight))
    return wp


def _param(p: torch.Tensor) -> torch.Tensor:
    """bias / cls / pos as the kernel reads them: bf16 or fp32 as stored, each with its own dtype code
    (no copy unless the tensor is another type or not contiguous)."""
    p = p.detach()
    if p.dtype not in (torch.bfloat16, torch.float32):
        p = p.float()
    return p.contiguous()


def forward_into(out: torch.Tensor, x, weight, bias, cls, pos, patch: int) -> torch.Tensor:
    """The forward into ``out``: ``[B (n + 1), D]`` rows with stride ``out.stride(0)`` (pack + ``patch_embed_fwd``)."""
    b, c, h, w = x.shape
    d = weight.shape[0]
    n = (h // patch) * (w // patch)
    if not supported(x, patch, d):
        raise ValueError("patch_embed: unsupported input (see ops.patch_embed.supported)")
    if bias.numel() != d or cls.numel() != d or pos.numel() != (n + 1) * d:
        raise ValueError("patch_embed: bias [D], cls [1, 1, D] and pos [1, n + 1, D] do not fit the image")
    wp = pack_weight(weight.detach(), patch, c)
    bias_, cls_, pos_ = _param(bias), _param(cls), _param(pos)
    _ext.get(required=True).patch_embed_fwd(
        x.data_ptr(), wp.data_ptr(), bias_.data_ptr(), cls_.data_ptr(), pos_.data_ptr(), out.data_ptr(), b, h, w, c,
        patch, d, out.stride(0), DTYPE_CODE[bias_.dtype], DTYPE_CODE[cls_.dtype], DTYPE_CODE[pos_.dtype], _stream(x))
    return out


def weight_grad(x: torch.Tensor, dy: torch.Tensor, weight: torch.Tensor, patch: int, splits: int | None = None):
    """``dy[:, 1:]^T unfold(x)`` in the filter's ``[D, 3 p p]`` layout: ``patch_embed_wgrad`` + ``gemm_splitk_reduce``
    (into the filter's bucket slice when the caller bound it with ``graddst.into``)."""
    b, c, h, w = x.shape
    d = weight.shape[0]
    m = b * (h // patch) * (w // patch)
    P = _ext.get(required=True)
    tiles = (d // 64) * (patch * patch * c // 64)
    s = P.patch_embed_wgrad_splits(m, splits or max(1, -(-WGRAD_TARGET // tiles)))
    ws = torch.empty(s, d, 3 * patch * patch, device=x.device, dtype=torch.float32)
    P.patch_embed_wgrad(x.data_ptr(), dy.data_ptr(), ws.data_ptr(), b, h, w, c, patch, d, s, _stream(x))
    odt = weight.dtype if weight.dtype in (torch.float32, torch.bfloat16) else torch.float32
    dw = graddst.empty(tuple(weight.shape), odt, x.device)
    _ext.get(required=True).gemm_splitk_reduce(ws.data_ptr(), s, dw.numel(), dw.data_ptr(), DTYPE_CODE[odt], _stream(x))
    return dw.to(weight.dtype)


class _PatchEmbed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, cls, pos, patch):
        b, _, h, w = x.shape
        d = weight.shape[0]
        n = (h // patch) * (w // patch)
        out = torch.empty(b, n + 1, d, device=x.device, dtype=torch.bfloat16)
        forward_into(out.view(b * (n + 1), d), x, weight, bias, cls, pos, patch)
        ctx.save_for_backward(x)
        ctx.params = (weight, bias, cls, pos)  # the leaves themselves: their bucket slices
        ctx.patch = patch
        return out

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        weight, bias, cls, pos = ctx.params
        need = ctx.needs_input_grad
        if dy.dtype != torch.bfloat16 or not dy.is_contiguous() or dy.data_ptr() % 16:
            dy = dy.to(torch.bfloat16).contiguous()
        dw = db = dcls = dpos = None
        if need[1]:
            with graddst.into(weight):
                dw = weight_grad(x, dy, weight, ctx.patch, WGRAD_SPLITS)
        if need[2] or need[3] or need[4]:
            s = torch.sum(dy, 0, dtype=torch.float32)  # [n + 1, D]: the one batch sum
            if need[4]:
                dpos = graddst.deliver(pos, s.view(pos.shape))
            if need[3]:
                dcls = graddst.deliver(cls, s[0].view(cls.shape))
            if need[2]:
                db = graddst.deliver(bias, s[1:].sum(0))
        return None, dw, db, dcls, dpos, None


def patch_embed(x, weight, bias, cls, pos, patch: int) -> torch.Tensor:
    """``[B, n + 1, D]`` bf16 tokens of a ``channels_last`` bf16 batch (see the module); differentiable in
    ``weight``, ``bias``, ``cls`` and ``pos`` (the image has no gradient). CPU tensors: the torch reference."""
    if not x.is_cuda:
        return patch_embed_reference(x, weight, bias, cls, pos, patch, dtype=x.dtype)
    if x.requires_grad and torch.is_grad_enabled():
        raise ValueError("patch_embed: the image has no gradient on this path; use the unfold path "
                         "(ViT(embed=\"fused\") takes it by itself) or detach the image")
    return _PatchEmbed.apply(x, weight, bias, cls, pos, patch)


def patches_reference(x: torch.Tensor, patch: int, dtype=torch.float64) -> torch.Tensor:
    """``A [B, n, p p C]`` in the kernel's K order ``(i, j, c)``, over all C channels of ``x [B, C, H, W]``."""
    b, c, h, w = x.shape
    a = x.permute(0, 2, 3, 1).to(dtype).reshape(b, h // patch, patch, w // patch, patch, c)
    return a.permute(0, 1, 3, 2, 4, 5).reshape(b, (h // patch) * (w // patch), patch * patch * c)


def pack_reference(weight: torch.Tensor, patch: int, channels: int, dtype=torch.float64) -> torch.Tensor:
    """``Wp [D, p p C]`` as ``patch_weight_pack`` lays it out (channel 3 zero)."""
    d = weight.shape[0]
    wp = weight.to(dtype).view(d, 3, patch, patch).permute(0, 2, 3, 1)
    if channels == 4:
        wp = F.pad(wp, (0, 1))
    return wp.reshape(d, patch * patch * channels)


def patch_embed_reference(x, weight, bias, cls, pos, patch: int, dtype=torch.float64) -> torch.Tensor:
    """:func:`patch_embed` in torch at ``dtype``, in the kernel's K order (any device, differentiable)."""
    b, c = x.shape[:2]
    d = weight.shape[0]
    tok = patches_reference(x, patch, dtype) @ pack_reference(weight, patch, c, dtype).t() + bias.to(dtype)
    pos = pos.to(dtype).view(1, -1, d)
    head = (cls.to(dtype).view(1, 1, d) + pos[:, :1]).expand(b, 1, d)
    return torch.cat([head, tok + pos[:, 1:]], 1)


__all__ = ["patch_embed", "patch_embed_reference", "supported", "layout_ok", "pack_weight", "forward_into",
           "weight_grad", "patches_reference", "pack_reference"]
