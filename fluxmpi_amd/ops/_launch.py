"""What every launch of the extension needs from a tensor, said once: its channels_last form, its
device pointer (0 for ``None``) and its stream's handle; and the vendor's convolution backward with
the argument list ``aten.convolution_backward`` wants. Imports nothing of the package (no cycles)."""
from __future__ import annotations

import torch


def nhwc(x: torch.Tensor) -> torch.Tensor:
    """``x`` in NHWC memory: itself when it already is channels_last (4-D) / contiguous (else), a copy otherwise."""
    if x.dim() == 4:
        return x if x.is_contiguous(memory_format=torch.channels_last) else x.contiguous(
            memory_format=torch.channels_last)
    return x.contiguous()


def ptr(t) -> int:
    return t.data_ptr() if t is not None else 0


def stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def conv_backward(dy, x, w, stride: int, pad: int, want_x: bool, want_w: bool):
    """``(dx, dw)`` of the bias-free, undilated, ungrouped ``conv2d(x, w, None, stride, pad)`` on the
    vendor library (MIOpen); the one not wanted is ``None``."""
    return torch.ops.aten.convolution_backward(dy, x, w, None, [stride, stride], [pad, pad], [1, 1], False, [0, 0], 1,
                                               [want_x, want_w, False])[:2]
