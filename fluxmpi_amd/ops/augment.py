"""Device input pipeline: random crop, flip, normalise, NHWC cast, channel pad and mixup / cutmix of
a uint8 image batch in one pass (``csrc/kernels/augment.hip``), deterministic from ``(seed, step,
sample)``.

``augment_batch(u8, size=(h, w), ...)`` takes the dense ``uint8 [B, H, W, 3]`` batch (any byte
alignment: a slice of a dataset) and returns the logical ``[B, C, h, w]`` view (channels_last strides)
of the NHWC bf16 / fp16 buffer it wrote, ``C`` in {3, 4} with channel 3 zero: the format the ResNet
stem, the ViT patch embedding and the small-channel convolutions take. GPU tensors run the kernel,
CPU tensors :func:`augment_reference` (numpy on :func:`..philox.philox4x32`), which agrees with the
kernel bit for bit.

Semantics, per output pixel ``(b, i, j)``:

* draws of sample ``b``: one Philox4x32-10 call, key ``(seed lo, seed hi)``, counter ``(s lo, s hi,
  stream, step)``, ``s = sample_offset + b``; ``ox = (w0 * rx) >> 32``, ``oy = (w1 * ry) >> 32``,
  ``flip = w2 & 1`` with ``rx = W + 2 pad - w + 1`` and ``ry`` likewise. ``crop="center"`` sets
  ``ox = (rx - 1) // 2``, ``oy = (ry - 1) // 2`` and draws nothing (so it does not flip either);
  ``flip=False`` forces 0;
* source pixel: row ``i + oy - pad``, column ``(w - 1 - j if flip else j) + ox - pad``; outside the
  image it is the byte ``fill`` in every channel, normalised like any pixel (torchvision's
  ``RandomCrop(padding)`` before ``Normalize``);
* ``y = float(u) * a_c + b_c`` in fp32, the product and the sum rounded separately, ``a_c = fp32(1 /
  (255 std_c))``, ``b_c = fp32(-mean_c / std_c)`` formed in double;
* mix with the partner ``B - 1 - b`` (timm's ``x.flip(0)``), whose pixel is its own crop and flip at
  the same ``(i, j)``: mixup ``z = y_p + lam * (y - y_p)`` (three rounded operations), cutmix ``z =
  y_p`` inside the box ``y0 <= i < y1, x0 <= j < x1``; the store is the round-to-nearest cast.

:class:`DeviceAugment` is the public class on top: the step counter, the host draw of the batch's
mixing (:func:`draw_mix`, timm's rules), the soft targets (:func:`mix_targets`) and the device block
that makes a call HIP-graph capturable.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _ext
from ._launch import ptr as _ptr
from ._launch import stream as _stream
from .multi_tensor import DTYPE_CODE
from .philox import philox4x32
from .xent import MixedLabels

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

MODE_NONE, MODE_MIXUP, MODE_CUTMIX = 0, 1, 2
# words of the device block (csrc/api.h: aug_block_set)
BLOCK_WORDS = 8
_BLOCK_LAM = 6


class MixDraw(NamedTuple):
    """A batch's mixing: ``mode`` 0 none / 1 mixup / 2 cutmix, ``lam`` the weight of a sample's own label
    (and, for mixup, of its own pixels), ``box = (y0, x0, y1, x1)`` the cutmix box in the output."""
    mode: int = MODE_NONE
    lam: float = 1.0
    box: tuple = (0, 0, 0, 0)


def _check_ids(op: str, seed, stream, step, sample_offset=0) -> None:
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"{op}: seed must be in [0, 2^64), got {seed}")
    if not 0 <= int(stream) < 1 << 30:
        raise ValueError(f"{op}: stream must be in [0, 2^30), got {stream}")
    if not 0 <= int(step) < 1 << 32:
        raise ValueError(f"{op}: step must be a uint32, got {step}")
    if not 0 <= int(sample_offset) < 1 << 62:
        raise ValueError(f"{op}: sample_offset must be in [0, 2^62), got {sample_offset}")


def sample_draws(n: int, seed: int, stream: int, step: int, sample_offset: int, rx: int, ry: int):
    """``(ox, oy, flip)`` (int64 arrays of ``n``) of samples ``sample_offset .. sample_offset + n``: the
    crop offsets in ``[0, rx)`` / ``[0, ry)`` and the flip bit."""
    _check_ids("sample_draws", seed, stream, step, sample_offset)
    if not (1 <= int(rx) < 1 << 32 and 1 <= int(ry) < 1 << 32):
        raise ValueError(f"sample_draws: the ranges must be in [1, 2^32), got {rx}, {ry}")
    s = np.arange(int(sample_offset), int(sample_offset) + int(n), dtype=np.uint64)
    ctr = np.stack([s & np.uint64(0xFFFFFFFF), s >> np.uint64(32), np.full_like(s, int(stream)),
                    np.full_like(s, int(step))], axis=-1)
    key = np.array([int(seed) & 0xFFFFFFFF, int(seed) >> 32], dtype=np.uint64)
    w = philox4x32(ctr, key).astype(np.uint64).reshape(-1, 4)
    ox = (w[:, 0] * np.uint64(rx)) >> np.uint64(32)  # 32 x 32 -> 64: no overflow
    oy = (w[:, 1] * np.uint64(ry)) >> np.uint64(32)
    flip = w[:, 2] & np.uint64(1)
    return ox.astype(np.int64), oy.astype(np.int64), flip.astype(np.int64)


def norm_constants(mean, std):
    """``(a, b)``, fp32 arrays of 3: ``y = u * a + b`` is ``(u / 255 - mean) / std``; formed in double."""
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    std = np.asarray(std, dtype=np.float64).reshape(-1)
    if mean.shape != (3,) or std.shape != (3,):
        raise ValueError("augment_batch: mean and std have 3 entries")
    if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std != 0)):
        raise ValueError("augment_batch: mean and std must be finite, std non-zero")
    return (1.0 / (255.0 * std)).astype(np.float32), (-mean / std).astype(np.float32)


class _Call(NamedTuple):
    B: int
    H: int
    W: int
    h: int
    w: int
    rx: int
    ry: int
    mix: MixDraw
    a: np.ndarray
    b: np.ndarray


def _check_input(op: str, u8, size):
    """``(B, H, W, h, w)`` of a checked input and ``size``."""
    if not isinstance(u8, torch.Tensor):
        raise TypeError(f"{op}: the input is a torch tensor, got {type(u8).__name__}")
    if u8.dtype != torch.uint8:
        raise TypeError(f"{op}: the input is uint8, got {u8.dtype}")
    if u8.dim() != 4 or u8.shape[-1] != 3:
        raise ValueError(f"{op}: the input is [B, H, W, 3], got {tuple(u8.shape)}")
    if not u8.is_contiguous():
        raise ValueError(f"{op}: the input must be dense")
    B, H, W, _ = u8.shape
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise TypeError(f"{op}: size is (h, w), got {size!r}") from None
    return B, H, W, h, w


def _check_output(op: str, u8, B, h, w, channels, dtype, mix, dev_block, out, uncast_ok) -> MixDraw:
    """The checks of what is written and mixed; returns the normalised :class:`MixDraw`."""
    if channels not in (3, 4):
        raise ValueError(f"{op}: channels must be 3 or 4, got {channels}")
    if dtype not in (torch.bfloat16, torch.float16) and not (uncast_ok and dtype == torch.float32):
        raise TypeError(f"{op}: dtype must be torch.bfloat16 or torch.float16, got {dtype}")
    mix = MixDraw() if mix is None else MixDraw(*mix)
    if mix.mode not in (MODE_NONE, MODE_MIXUP, MODE_CUTMIX):
        raise ValueError(f"{op}: the mix mode must be 0, 1 or 2, got {mix.mode}")
    if not math.isfinite(float(mix.lam)):
        raise ValueError(f"{op}: lam must be finite, got {mix.lam}")
    y0, x0, y1, x1 = (int(v) for v in mix.box)
    if mix.mode == MODE_CUTMIX and not (0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w):
        raise ValueError(f"{op}: the box {(y0, x0, y1, x1)} must lie inside the output {(h, w)}")
    mix = MixDraw(int(mix.mode), float(mix.lam), (y0, x0, y1, x1))
    if dev_block is not None:
        if not (isinstance(dev_block, torch.Tensor) and dev_block.dtype == torch.int32
                and dev_block.numel() >= BLOCK_WORDS and dev_block.is_contiguous() and dev_block.device == u8.device
                and u8.is_cuda):
            raise ValueError(f"{op}: dev_block is a dense int32 tensor of {BLOCK_WORDS} words on the input's GPU")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != dtype:
            raise TypeError(f"{op}: out must be a {dtype} tensor")
        if out.device != u8.device:
            raise ValueError(f"{op}: out must live on {u8.device}")
        if tuple(out.shape) == (B, channels, h, w):
            dense = out.permute(0, 2, 3, 1).is_contiguous()
        else:
            dense = tuple(out.shape) == (B, h, w, channels) and out.is_contiguous()
        if not dense:
            raise ValueError(f"{op}: out must be the dense NHWC buffer [{B}, {h}, {w}, {channels}] (or its "
                             f"[B, C, h, w] view), got shape {tuple(out.shape)} strides {tuple(out.stride())}")
        if out.data_ptr() % 16 != 0:
            raise ValueError(f"{op}: out must be 16-byte aligned")
    return mix


def _validate(u8, size, pad, fill, crop, flip, mean, std, channels, dtype, seed, stream, step, sample_offset, mix,
              dev_block, out, uncast_ok=False) -> _Call:
    op = "augment_batch"
    B, H, W, h, w = _check_input(op, u8, size)
    pad, fill = int(pad), int(fill)
    if pad < 0 or pad > 1 << 20:
        raise ValueError(f"{op}: pad must be in [0, 2^20], got {pad}")
    if not 0 <= fill <= 255:
        raise ValueError(f"{op}: fill is a byte, got {fill}")
    if H < 1 or W < 1 or max(H, W) > 1 << 24:
        raise ValueError(f"{op}: the image sides must be in [1, 2^24], got {H} x {W}")
    if h < 1 or w < 1 or h > H + 2 * pad or w > W + 2 * pad:
        raise ValueError(f"{op}: size {(h, w)} must be positive and at most the padded image "
                         f"{(H + 2 * pad, W + 2 * pad)}")
    if crop not in ("random", "center"):
        raise ValueError(f"{op}: crop is 'random' or 'center', got {crop!r}")
    if channels not in (3, 4):
        raise ValueError(f"{op}: channels must be 3 or 4, got {channels}")
    if dtype not in (torch.bfloat16, torch.float16) and not (uncast_ok and dtype == torch.float32):
        raise TypeError(f"{op}: dtype must be torch.bfloat16 or torch.float16, got {dtype}")
    _check_ids(op, seed, stream, step, sample_offset)
    mix = _check_output(op, u8, B, h, w, channels, dtype, mix, dev_block, out, uncast_ok)
    a, b = norm_constants(mean, std)
    return _Call(B, H, W, h, w, W + 2 * pad - w + 1, H + 2 * pad - h + 1, mix, a, b)


def _draws(c: _Call, crop, flip, seed, stream, step, sample_offset):
    if crop == "center":
        return (np.full(c.B, (c.rx - 1) // 2, dtype=np.int64), np.full(c.B, (c.ry - 1) // 2, dtype=np.int64),
                np.zeros(c.B, dtype=np.int64))
    ox, oy, fl = sample_draws(c.B, seed, stream, step, sample_offset, c.rx, c.ry)
    return ox, oy, fl if flip else np.zeros_like(fl)


def _reference(u8: torch.Tensor, c: _Call, pad, fill, crop, flip, channels, dtype, seed, stream, step,
               sample_offset) -> torch.Tensor:
    """The NHWC ``[B, h, w, channels]`` result on the CPU."""
    img = u8.detach().cpu().numpy()
    ox, oy, fl = _draws(c, crop, flip, seed, stream, step, sample_offset)
    padded = np.full((c.B, c.H + 2 * pad, c.W + 2 * pad, 3), fill, dtype=np.uint8)
    padded[:, pad:pad + c.H, pad:pad + c.W] = img
    rows = np.arange(c.h)[None, :] + oy[:, None]  # [B, h] in padded coordinates
    j = np.arange(c.w)[None, :]
    cols = np.where(fl[:, None] == 1, c.w - 1 - j, j) + ox[:, None]  # [B, w]
    u = padded[np.arange(c.B)[:, None, None], rows[:, :, None], cols[:, None, :]]  # [B, h, w, 3]
    y = u.astype(np.float32) * c.a.reshape(1, 1, 1, 3)  # the product rounded to fp32 ...
    y = y + c.b.reshape(1, 1, 1, 3)  # ... then the sum
    mode, lam, (y0, x0, y1, x1) = c.mix
    if mode == MODE_MIXUP:
        yp = y[::-1]
        d = y - yp
        t = np.float32(lam) * d
        y = yp + t
    elif mode == MODE_CUTMIX:
        y = y.copy()
        y[:, y0:y1, x0:x1] = y[::-1][:, y0:y1, x0:x1].copy()
    assert y.dtype == np.float32
    z = torch.zeros(c.B, c.h, c.w, channels, dtype=dtype)
    z[..., :3] = torch.from_numpy(np.ascontiguousarray(y)).to(dtype)  # round to nearest
    return z


def augment_reference(u8: torch.Tensor, *, size, pad=0, fill=0, crop="random", flip=True, mean=IMAGENET_MEAN,
                      std=IMAGENET_STD, channels=3, dtype=torch.bfloat16, seed=0, stream=0, step=0, sample_offset=0,
                      mix=None) -> torch.Tensor:
    """:func:`augment_batch` in numpy on the CPU (the kernel's oracle): the ``[B, C, h, w]`` channels_last
    view, on ``u8``'s device. ``dtype=torch.float32`` (here only): the fp32 values before the cast."""
    c = _validate(u8, size, pad, fill, crop, flip, mean, std, channels, dtype, seed, stream, step, sample_offset, mix,
                  None, None, uncast_ok=True)
    z = _reference(u8, c, int(pad), int(fill), crop, flip, channels, dtype, seed, stream, step, sample_offset)
    return z.to(u8.device).permute(0, 3, 1, 2)


def augment_batch(u8: torch.Tensor, *, size, pad=0, fill=0, crop="random", flip=True, mean=IMAGENET_MEAN,
                  std=IMAGENET_STD, channels=3, dtype=torch.bfloat16, seed=0, stream=0, step=0, sample_offset=0,
                  mix=None, dev_block=None, out=None) -> torch.Tensor:
    """Crop, flip, normalise and mix the ``uint8 [B, H, W, 3]`` batch ``u8`` (module docstring); returns
    the ``[B, channels, h, w]`` view of the NHWC buffer (``out`` when given). ``mix``: a
    :class:`MixDraw` (or ``(mode, lam, box)``). ``dev_block`` (GPU only): the 8-word int32 device block
    of :func:`block_set`, which then supplies ``step``, the mode, the box and ``lam``."""
    c = _validate(u8, size, pad, fill, crop, flip, mean, std, channels, dtype, seed, stream, step, sample_offset, mix,
                  dev_block, out)
    pad, fill = int(pad), int(fill)
    if not u8.is_cuda:
        z = _reference(u8, c, pad, fill, crop, flip, channels, dtype, seed, stream, step, sample_offset)
        if out is None:
            return z.permute(0, 3, 1, 2)
        (out if out.shape == z.shape else out.permute(0, 2, 3, 1)).copy_(z)
        return out if tuple(out.shape) == (c.B, channels, c.h, c.w) else out.permute(0, 3, 1, 2)
    A = _ext.get(required=True)
    buf = out if out is not None else torch.empty(c.B, c.h, c.w, channels, device=u8.device, dtype=dtype)
    A.augment_batch(u8.data_ptr(), buf.data_ptr(), c.B, c.H, c.W, c.h, c.w, channels, DTYPE_CODE[dtype], int(seed),
                    int(stream), int(step), int(sample_offset), c.mix.mode, list(c.mix.box), c.mix.lam, pad, fill,
                    int(crop == "center"), int(bool(flip)), c.a.tolist(), c.b.tolist(), _ptr(dev_block), _stream(u8))
    return buf if tuple(buf.shape) == (c.B, channels, c.h, c.w) and out is not None else buf.permute(0, 3, 1, 2)


# ---- the resampling form: a per-sample box resized bilinearly (csrc/kernels/resize_crop.hip) ----------
RRC_MAX_SIDE = 16384  # every index product of the resampling then fits 32 bits
_RRC_ATTEMPTS = 10


def _box_table(op: str, boxes, B: int) -> np.ndarray:
    """A host table as int64 ``[B, 5]``."""
    t = boxes.detach().cpu().numpy() if isinstance(boxes, torch.Tensor) else np.asarray(boxes)
    if t.ndim != 2 or t.shape != (B, 5) or t.dtype.kind not in "iu":
        raise ValueError(f"{op}: boxes is an integer table [{B}, 5] of (top, left, bh, bw, flip), got "
                         f"{t.dtype} {tuple(t.shape)}")
    return t.astype(np.int64)


def clamp_boxes(boxes, H: int, W: int) -> np.ndarray:
    """The kernel's clamp of a box table (int64 ``[n, 5]``): ``top`` into ``[0, H - 1]``, ``bh`` into ``[1, H -
    top]``, columns likewise, ``flip & 1``. A table of boxes inside the image is unchanged."""
    t = np.array(boxes.detach().cpu().numpy() if isinstance(boxes, torch.Tensor) else boxes, dtype=np.int64)
    top = np.clip(t[:, 0], 0, H - 1)
    left = np.clip(t[:, 1], 0, W - 1)
    bh = np.clip(t[:, 2], 1, H - top)
    bw = np.clip(t[:, 3], 1, W - left)
    return np.stack([top, left, bh, bw, t[:, 4] & 1], axis=1)


def _check_boxes(op: str, t: np.ndarray, H: int, W: int) -> None:
    """A host table holds boxes inside the image: ``ValueError`` naming the first sample that does not."""
    bad = ~((t[:, 0] >= 0) & (t[:, 2] >= 1) & (t[:, 0] + t[:, 2] <= H) & (t[:, 1] >= 0) & (t[:, 3] >= 1)
            & (t[:, 1] + t[:, 3] <= W) & ((t[:, 4] == 0) | (t[:, 4] == 1)))
    if bad.any():
        b = int(np.argmax(bad))
        raise ValueError(f"{op}: the box of sample {b}, (top, left, bh, bw, flip) = {tuple(int(v) for v in t[b])}, "
                         f"must lie inside the {H} x {W} image with flip 0 or 1")


def _resample_terms(idx: np.ndarray, n_src: np.ndarray, n_out: int):
    """``(p0, p1, f)`` of output indices ``idx`` (int64, broadcast against ``n_src``): half-pixel centres,
    the weight ``f`` of ``p1`` in 1/2048, rounded."""
    num = (2 * idx + 1) * n_src - n_out
    den = 2 * n_out
    pos = num >= 0
    p0 = np.where(pos, num // den, 0)
    f = np.where(pos, ((num % den) * 2048 + n_out) // den, 0)
    return p0, np.minimum(p0 + 1, n_src - 1), f


def _resample(img: np.ndarray, t: np.ndarray, h: int, w: int) -> np.ndarray:
    """The resampled bytes ``[B, h, w, 3]`` (int64) of the clamped table ``t``."""
    B = img.shape[0]
    top, left, bh, bw, flip = (t[:, c:c + 1] for c in range(5))  # [B, 1]
    j = np.arange(w, dtype=np.int64)[None, :]
    x0, x1, fx = _resample_terms(np.where(flip == 1, w - 1 - j, j), bw, w)  # [B, w]
    y0, y1, fy = _resample_terms(np.arange(h, dtype=np.int64)[None, :], bh, h)  # [B, h]
    bi = np.arange(B)[:, None, None]
    ra, rb = (top + y0)[:, :, None], (top + y1)[:, :, None]
    ca, cb = (left + x0)[:, None, :], (left + x1)[:, None, :]
    p00, p01 = img[bi, ra, ca].astype(np.int64), img[bi, ra, cb].astype(np.int64)  # [B, h, w, 3]
    p10, p11 = img[bi, rb, ca].astype(np.int64), img[bi, rb, cb].astype(np.int64)
    fx, fy = fx[:, None, :, None], fy[:, :, None, None]
    t0 = p00 * (2048 - fx) + p01 * fx
    t1 = p10 * (2048 - fx) + p11 * fx
    return (t0 * (2048 - fy) + t1 * fy + (1 << 21)) >> 22


class _RrcCall(NamedTuple):
    B: int
    H: int
    W: int
    h: int
    w: int
    mix: MixDraw
    a: np.ndarray
    b: np.ndarray


def _validate_rrc(u8, size, mean, std, channels, dtype, mix, dev_block, out, uncast_ok=False) -> _RrcCall:
    op = "resized_crop_batch"
    B, H, W, h, w = _check_input(op, u8, size)
    if min(H, W, h, w) < 1 or max(H, W, h, w) > RRC_MAX_SIDE:
        raise ValueError(f"{op}: the sides of the image and of the output must be in [1, {RRC_MAX_SIDE}], got "
                         f"{H} x {W} -> {h} x {w}")
    mix = _check_output(op, u8, B, h, w, channels, dtype, mix, dev_block, out, uncast_ok)
    a, b = norm_constants(mean, std)
    return _RrcCall(B, H, W, h, w, mix, a, b)


def _rrc_reference(u8: torch.Tensor, t: np.ndarray, c: _RrcCall, channels, dtype) -> torch.Tensor:
    """The NHWC ``[B, h, w, channels]`` result on the CPU from the host table ``t``, clamped here."""
    v = _resample(u8.detach().cpu().numpy(), clamp_boxes(t, c.H, c.W), c.h, c.w) if c.B else \
        np.zeros((0, c.h, c.w, 3), dtype=np.int64)
    y = v.astype(np.float32) * c.a.reshape(1, 1, 1, 3)  # the product rounded to fp32 ...
    y = y + c.b.reshape(1, 1, 1, 3)  # ... then the sum
    mode, lam, (y0, x0, y1, x1) = c.mix
    if mode == MODE_MIXUP:
        yp = y[::-1]
        d = y - yp
        t_ = np.float32(lam) * d
        y = yp + t_
    elif mode == MODE_CUTMIX:
        y = y.copy()
        y[:, y0:y1, x0:x1] = y[::-1][:, y0:y1, x0:x1].copy()
    assert y.dtype == np.float32
    z = torch.zeros(c.B, c.h, c.w, channels, dtype=dtype)
    z[..., :3] = torch.from_numpy(np.ascontiguousarray(y)).to(dtype)  # round to nearest
    return z


def resized_crop_reference(u8: torch.Tensor, boxes, *, size, mean=IMAGENET_MEAN, std=IMAGENET_STD, channels=3,
                           dtype=torch.bfloat16, mix=None) -> torch.Tensor:
    """:func:`resized_crop_batch` in numpy on the CPU (the kernel's oracle): the ``[B, C, h, w]``
    channels_last view, on ``u8``'s device. ``boxes`` (numpy or a tensor anywhere) goes through the
    kernel's clamp (:func:`clamp_boxes`), so a table of valid boxes is used as it is.
    ``dtype=torch.float32`` (here only): the fp32 values before the cast."""
    c = _validate_rrc(u8, size, mean, std, channels, dtype, mix, None, None, uncast_ok=True)
    z = _rrc_reference(u8, _box_table("resized_crop_batch", boxes, c.B), c, channels, dtype)
    return z.to(u8.device).permute(0, 3, 1, 2)


def resized_crop_batch(u8: torch.Tensor, boxes, *, size, mean=IMAGENET_MEAN, std=IMAGENET_STD, channels=3,
                       dtype=torch.bfloat16, mix=None, dev_block=None, out=None) -> torch.Tensor:
    """Resample each sample's box of the ``uint8 [B, H, W, 3]`` batch ``u8`` to ``size`` (bilinear,
    half-pixel centres, no antialias: ``F.interpolate(mode="bilinear", align_corners=False)`` and cv2's
    ``INTER_LINEAR``, in integer arithmetic with cv2's 11-bit weights), flip, normalise and mix; returns
    the ``[B, channels, h, w]`` view of the NHWC buffer (``out`` when given). Sides at most 16384.

    ``boxes``: int32 ``[B, 5]`` of ``(top, left, bh, bw, flip)``, a box inside the image
    (:func:`rrc_boxes`, :func:`center_boxes`). Output column ``j`` (``j' = w - 1 - j`` under a flip):
    ``num = (2 j' + 1) bw - w``, ``den = 2 w``; ``num < 0``: ``x0 = 0, fx = 0``, else ``x0 = num // den``,
    ``fx = ((num % den) * 2048 + w) // den``; ``x1 = min(x0 + 1, bw - 1)``; rows likewise without flip.
    Per channel ``t0 = p00 (2048 - fx) + p01 fx``, ``t1`` likewise on row ``y1``, ``v = (t0 (2048 - fy) + t1
    fy + 2^21) >> 22``; from the byte ``v`` on the arithmetic is :func:`augment_batch`'s, the partner
    ``B - 1 - b`` with its own box and flip.

    A host table (numpy, a CPU tensor) is validated (``ValueError`` naming the sample) and, for a GPU
    batch, uploaded with one small copy on the current stream. A table on the GPU is used as it is; since
    it forms addresses, the kernel clamps every box to the image first (:func:`clamp_boxes`), and so
    does the reference. CPU tensors run :func:`resized_crop_reference`."""
    op = "resized_crop_batch"
    c = _validate_rrc(u8, size, mean, std, channels, dtype, mix, dev_block, out)
    on_device = isinstance(boxes, torch.Tensor) and boxes.is_cuda
    if on_device:
        if not (u8.is_cuda and boxes.device == u8.device and boxes.dtype == torch.int32
                and tuple(boxes.shape) == (c.B, 5) and boxes.is_contiguous()):
            raise ValueError(f"{op}: a device table of boxes is a dense int32 [{c.B}, 5] tensor on the input's GPU")
    else:
        table = _box_table(op, boxes, c.B)
        _check_boxes(op, table, c.H, c.W)
    if not u8.is_cuda:
        z = _rrc_reference(u8, table, c, channels, dtype)
        if out is None:
            return z.permute(0, 3, 1, 2)
        (out if out.shape == z.shape else out.permute(0, 2, 3, 1)).copy_(z)
        return out if tuple(out.shape) == (c.B, channels, c.h, c.w) else out.permute(0, 3, 1, 2)
    R = _ext.rrc()
    if not on_device:  # pageable memory: the copy is ordered with the stream
        boxes = torch.from_numpy(table.astype(np.int32)).to(u8.device)
    buf = out if out is not None else torch.empty(c.B, c.h, c.w, channels, device=u8.device, dtype=dtype)
    R.resized_crop_batch(u8.data_ptr(), buf.data_ptr(), boxes.data_ptr(), c.B, c.H, c.W, c.h, c.w, channels,
                         DTYPE_CODE[dtype], 0, c.mix.mode, list(c.mix.box), c.mix.lam, c.a.tolist(), c.b.tolist(),
                         _ptr(dev_block), _stream(u8))
    return buf if tuple(buf.shape) == (c.B, channels, c.h, c.w) and out is not None else buf.permute(0, 3, 1, 2)


def _pair(op: str, name: str, v):
    try:
        lo, hi = (float(x) for x in v)
    except (TypeError, ValueError):
        raise TypeError(f"{op}: {name} is a pair (lo, hi), got {v!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo <= hi):
        raise ValueError(f"{op}: {name} must satisfy 0 < lo <= hi, got {v!r}")
    return lo, hi


def rrc_boxes(n: int, H: int, W: int, *, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip=True, seed=0, stream=0, step=0,
              sample_offset=0, return_attempts=False):
    """The boxes ``int32 [n, 5]`` of torchvision's ``RandomResizedCrop.get_params`` for samples
    ``sample_offset .. sample_offset + n`` of ``H x W`` images, on the host, vectorised over the batch.

    Up to 10 attempts per sample. Attempt ``k`` of sample ``s`` is one Philox4x32-10 call, key the seed,
    counter ``(s lo, s hi, stream | (k + 1) << 26, step)`` (so ``stream < 2^26`` here; the translation
    crop's own call is ``k + 1 = 0``), words ``w0..w3``, ``u_k = w_k * 2^-32`` in float64: ``area = H W
    (s0 + u0 (s1 - s0))``, ``aspect = exp(log r0 + u1 (log r1 - log r0))``, ``bw = round(sqrt(area *
    aspect))``, ``bh = round(sqrt(area / aspect))`` (round half to even, as Python's ``round``); accepted
    when ``0 < bw <= W`` and ``0 < bh <= H``, then ``top = (w2 (H - bh + 1)) >> 32``, ``left = (w3 (W - bw +
    1)) >> 32``. After 10 failures: torchvision's fallback, the central crop with the image's aspect
    clamped into ``ratio``. The flip is the bit ``w2 & 1`` of the sample's :func:`sample_draws` call: a
    sample flips exactly when it does under the translation crop; ``flip=False`` forces 0.

    A box is a function of ``(seed, stream, step, s)`` alone: splitting a batch or moving a sample
    between ranks does not change it. The draws are float64 on the host and nothing on the device
    reproduces them; a libm that differs in the last bit of ``exp`` or ``log`` can move a box by one
    pixel, in roughly one draw in 10^13. ``return_attempts=True``: also the int64 array of failed attempts
    per sample (10: the fallback ran)."""
    op = "rrc_boxes"
    _check_ids(op, seed, stream, step, sample_offset)
    if int(stream) >= 1 << 26:
        raise ValueError(f"{op}: stream must be in [0, 2^26), got {stream}")
    n, H, W = int(n), int(H), int(W)
    if n < 0 or not (1 <= H <= RRC_MAX_SIDE and 1 <= W <= RRC_MAX_SIDE):
        raise ValueError(f"{op}: n is not negative and the image sides are in [1, {RRC_MAX_SIDE}], got {n}, {H} x {W}")
    s0, s1 = _pair(op, "scale", scale)
    r0, r1 = _pair(op, "ratio", ratio)
    l0, l1 = math.log(r0), math.log(r1)
    s = np.arange(int(sample_offset), int(sample_offset) + n, dtype=np.uint64)
    key = np.array([int(seed) & 0xFFFFFFFF, int(seed) >> 32], dtype=np.uint64)
    top, left = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    bh, bw = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    attempts = np.full(n, _RRC_ATTEMPTS, dtype=np.int64)
    for k in range(_RRC_ATTEMPTS):
        open_ = attempts == _RRC_ATTEMPTS
        if not open_.any():
            break
        ctr = np.stack([s & np.uint64(0xFFFFFFFF), s >> np.uint64(32),
                        np.full_like(s, int(stream) | ((k + 1) << 26)), np.full_like(s, int(step))], axis=-1)
        wd = philox4x32(ctr, key).astype(np.uint64).reshape(-1, 4)
        u0, u1 = wd[:, 0].astype(np.float64) * 2.0 ** -32, wd[:, 1].astype(np.float64) * 2.0 ** -32
        area = (H * W) * (s0 + u0 * (s1 - s0))
        aspect = np.exp(l0 + u1 * (l1 - l0))
        cw = np.rint(np.sqrt(area * aspect)).astype(np.int64)
        ch = np.rint(np.sqrt(area / aspect)).astype(np.int64)
        ok = open_ & (cw > 0) & (cw <= W) & (ch > 0) & (ch <= H)
        ct = (wd[:, 2] * (H - np.where(ok, ch, H) + 1).astype(np.uint64)) >> np.uint64(32)  # 32 x 32 -> 64
        cl = (wd[:, 3] * (W - np.where(ok, cw, W) + 1).astype(np.uint64)) >> np.uint64(32)
        top, left = np.where(ok, ct.astype(np.int64), top), np.where(ok, cl.astype(np.int64), left)
        bh, bw = np.where(ok, ch, bh), np.where(ok, cw, bw)
        attempts = np.where(ok, k, attempts)
    failed = attempts == _RRC_ATTEMPTS
    if failed.any():
        in_ratio = W / H
        if in_ratio < r0:
            fw, fh = W, int(round(W / r0))
        elif in_ratio > r1:
            fh = H
            fw = int(round(H * r1))
        else:
            fw, fh = W, H
        fh, fw = max(1, min(H, fh)), max(1, min(W, fw))
        bh, bw = np.where(failed, fh, bh), np.where(failed, fw, bw)
        top, left = np.where(failed, (H - fh) // 2, top), np.where(failed, (W - fw) // 2, left)
    if flip and n:
        fl = sample_draws(n, seed, stream, step, sample_offset, 1, 1)[2]
    else:
        fl = np.zeros(n, dtype=np.int64)
    boxes = np.stack([top, left, bh, bw, fl], axis=1).astype(np.int32).reshape(n, 5)
    return (boxes, attempts) if return_attempts else boxes


def center_boxes(n: int, H: int, W: int, size, crop_pct: float = 0.875) -> np.ndarray:
    """The evaluation transform as one box per sample, ``int32 [n, 5]``: ``Resize`` (the shorter relative
    side to ``size / crop_pct``) then ``CenterCrop(size)``. ``s = min(H / h, W / w) * crop_pct``, ``bh = max(1,
    min(H, round(h s)))``, ``bw`` likewise, centred, no flip. For a set stored at 8/7 of the crop (256 ->
    224) it is the identity scale: the plain centre crop."""
    op = "center_boxes"
    n, H, W = int(n), int(H), int(W)
    h, w = (int(size), int(size)) if isinstance(size, int) else (int(v) for v in size)
    if n < 0 or min(H, W, h, w) < 1:
        raise ValueError(f"{op}: n is not negative and the sides are positive, got {n}, {H} x {W} -> {h} x {w}")
    if not (math.isfinite(crop_pct) and 0 < crop_pct <= 1):
        raise ValueError(f"{op}: crop_pct must lie in (0, 1], got {crop_pct}")
    s = min(H / h, W / w) * float(crop_pct)
    bh = max(1, min(H, int(round(h * s))))
    bw = max(1, min(W, int(round(w * s))))
    return np.tile(np.array([[(H - bh) // 2, (W - bw) // 2, bh, bw, 0]], dtype=np.int32), (n, 1))


def block_set(block: torch.Tensor, step: int, mix: MixDraw | None = None) -> None:
    """Fill the device block (8 int32 words on a GPU) for the coming call: one tiny launch on the
    current stream, outside a captured region."""
    mix = MixDraw() if mix is None else MixDraw(*mix)
    _check_ids("aug_block_set", 0, 0, step)
    if not (block.is_cuda and block.dtype == torch.int32 and block.numel() >= BLOCK_WORDS and block.is_contiguous()):
        raise ValueError(f"aug_block_set: the block is a dense int32 GPU tensor of {BLOCK_WORDS} words")
    _ext.get(required=True).aug_block_set(block.data_ptr(), int(step), int(mix.mode), [int(v) for v in mix.box],
                                          float(mix.lam), _stream(block))


def block_lam(block: torch.Tensor) -> torch.Tensor:
    """The block's ``lam`` word as a 0-dim fp32 tensor (a view: it follows the block)."""
    return block[_BLOCK_LAM:_BLOCK_LAM + 1].view(torch.float32)[0]


def _cutmix_box(rng, size, lam: float):
    """timm's ``rand_bbox``: a box of ``sqrt(1 - lam)`` of each side around a uniform centre, clipped."""
    h, w = size
    ratio = math.sqrt(max(0.0, 1.0 - lam))
    cut_h, cut_w = int(h * ratio), int(w * ratio)
    cy = int(rng.integers(0, h))
    cx = int(rng.integers(0, w))
    y0, y1 = min(max(cy - cut_h // 2, 0), h), min(max(cy + cut_h // 2, 0), h)
    x0, x1 = min(max(cx - cut_w // 2, 0), w), min(max(cx + cut_w // 2, 0), w)
    return y0, x0, y1, x1


def draw_mix(seed: int, stream: int, step: int, size, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0,
             prob: float = 1.0, switch_prob: float = 0.5, *, lam: float | None = None) -> MixDraw:
    """The batch's mixing for ``step``, on the host, from ``numpy.random.Generator(Philox(key=seed,
    counter=[0, 0, step, stream]))``. (numpy's Philox counts its blocks in the counter's word 0: with
    the step there, step ``s + 1`` would replay step ``s``'s numbers from the fifth on, and consecutive
    steps did draw the same mixing. In the upper words every ``(step, stream)`` owns 2^128 blocks.)
    By timm's rules: with probability ``prob`` the batch mixes; with
    both alphas positive it is cutmix with probability ``switch_prob``; ``lambda ~ Beta(alpha, alpha)``;
    the cutmix box has ``sqrt(1 - lambda)`` of each side around a uniform centre, clipped to the image,
    and the returned ``lam`` is then ``1 - area / (h * w)``. ``lam`` (keyword): use this lambda instead
    of the Beta draw (tests of the edge values)."""
    _check_ids("draw_mix", seed, stream, step)
    h, w = (int(v) for v in size)
    if h < 1 or w < 1:
        raise ValueError(f"draw_mix: size must be positive, got {size}")
    if mixup_alpha < 0 or cutmix_alpha < 0 or not 0 <= prob <= 1 or not 0 <= switch_prob <= 1:
        raise ValueError("draw_mix: alphas are not negative, probabilities lie in [0, 1]")
    if mixup_alpha == 0 and cutmix_alpha == 0:
        return MixDraw()
    rng = np.random.Generator(np.random.Philox(key=int(seed), counter=[0, 0, int(step), int(stream)]))
    if not rng.random() < prob:
        return MixDraw()
    if mixup_alpha > 0 and cutmix_alpha > 0:
        cut = bool(rng.random() < switch_prob)
    else:
        cut = cutmix_alpha > 0
    alpha = cutmix_alpha if cut else mixup_alpha
    drawn = float(rng.beta(alpha, alpha))
    lam_ = drawn if lam is None else float(lam)
    if not 0.0 <= lam_ <= 1.0:
        raise ValueError(f"draw_mix: lam must lie in [0, 1], got {lam_}")
    if not cut:
        return MixDraw(MODE_MIXUP, lam_, (0, 0, 0, 0))
    y0, x0, y1, x1 = _cutmix_box(rng, (h, w), lam_)
    return MixDraw(MODE_CUTMIX, 1.0 - ((y1 - y0) * (x1 - x0)) / (h * w), (y0, x0, y1, x1))


def mix_targets(labels: torch.Tensor, num_classes: int, lam, label_smoothing: float = 0.0) -> torch.Tensor:
    """``lam * S(y) + (1 - lam) * S(y.flip(0))``, ``[B, K]`` fp32, with ``S = onehot * (1 - eps) + eps /
    K``. ``lam``: a float or a 0-dim tensor on ``labels``' device (no host read: capturable)."""
    if labels.dim() != 1 or labels.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"mix_targets: labels are a 1-D integer tensor, got {labels.dtype} {tuple(labels.shape)}")
    if int(num_classes) < 1:
        raise ValueError(f"mix_targets: num_classes must be positive, got {num_classes}")
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"mix_targets: label_smoothing must lie in [0, 1), got {label_smoothing}")
    K = int(num_classes)
    s = torch.full((labels.shape[0], K), label_smoothing / K, device=labels.device, dtype=torch.float32)
    s.scatter_(1, labels.long().unsqueeze(1), 1.0 - label_smoothing + label_smoothing / K)
    if isinstance(lam, torch.Tensor):
        lam = lam.to(torch.float32)
        rest = 1.0 - lam
    else:  # the fp32 values the tensor route computes with, so that both routes give the same bits
        lam32 = np.float32(lam)
        lam, rest = float(lam32), float(np.float32(1.0) - lam32)
    return lam * s + rest * s.flip(0)


class DeviceAugment:
    """The training input pipeline on the device: ``x, y = aug(images_u8, labels)``.

    ``images``: ``uint8 [B, H, W, 3]``; ``x``: the ``[B, channels, h, w]`` channels_last batch of
    :func:`augment_batch` (random crop of ``size`` from the image zero-extended by ``pad``, flip,
    normalise, and the batch's mixup / cutmix). ``y``: ``labels`` untouched when nothing mixes and
    ``label_smoothing == 0``, else the soft targets ``[B, num_classes]`` of :func:`mix_targets`
    (``targets="dense"``, the default) or, with ``targets="labels"``, ``MixedLabels(labels, lam,
    label_smoothing)`` for :func:`..xent.softmax_cross_entropy`: ``lam`` the float of the draw, or the
    block's device word under ``use_block=True``; no dense matrix is built.

    ``step`` defaults to an internal counter that advances once per call; ``sample_offset`` defaults
    to ``local_rank() * B`` once ``Init()`` ran (ranks draw different crops from one seed), else 0.
    ``aug.eval()`` gives the centre crop without flip or mix, the same every call; ``aug.train()``
    switches back.

    HIP-graph use: ``aug.prepare(step)`` (outside the captured region, before each replay) draws the
    step's mixing on the host and writes it into the device block with one tiny launch;
    ``aug(images, labels, use_block=True)`` launches the kernel on the block and forms the targets
    from the block's ``lam`` word, so the captured graph is the same every step.

    ``crop="resized"`` is the ImageNet recipe on :func:`resized_crop_batch`: training draws
    torchvision's ``RandomResizedCrop(size, scale, ratio)`` boxes on the host (:func:`rrc_boxes`, one box
    per ``(seed, step, sample_offset + b)``) and uploads the table with one small copy; ``eval()`` is
    ``Resize`` + ``CenterCrop`` as :func:`center_boxes` with ``crop_pct``. ``pad`` and ``fill`` must be 0.
    Its graph route keeps a persistent device table: ``aug.prepare(step, batch=B, image_size=(H, W))``
    also writes the step's boxes into it (without ``image_size`` before the instance has seen a batch,
    the first ``use_block`` call writes the table and has to be outside a captured region, as a warm-up
    call is), and ``aug(images, labels, use_block=True)`` launches on the block and that table.
    ``crop="pad"`` (the default) is the translation crop described above.
    """

    def __init__(self, size, *, pad=0, fill=0, flip=True, mean=IMAGENET_MEAN, std=IMAGENET_STD, channels=3,
                 dtype=torch.bfloat16, seed=0, mixup_alpha=0.0, cutmix_alpha=0.0, mix_prob=1.0, switch_prob=0.5,
                 label_smoothing=0.0, num_classes=None, targets="dense", crop="pad", scale=(0.08, 1.0),
                 ratio=(3 / 4, 4 / 3), crop_pct=0.875):
        if crop not in ("pad", "resized"):
            raise ValueError(f"DeviceAugment: crop is 'pad' or 'resized', got {crop!r}")
        if crop == "resized" and (int(pad) != 0 or int(fill) != 0):
            raise ValueError("DeviceAugment: with crop='resized' a box lies inside the image: pad and fill must be 0")
        self.crop = crop
        self.scale, self.ratio = _pair("DeviceAugment", "scale", scale), _pair("DeviceAugment", "ratio", ratio)
        if not (math.isfinite(crop_pct) and 0 < crop_pct <= 1):
            raise ValueError(f"DeviceAugment: crop_pct must lie in (0, 1], got {crop_pct}")
        self.crop_pct = float(crop_pct)
        self._table = None  # the graph route's persistent device table of boxes, and the image size it is for
        self._image_size = None
        self._pending = None  # prepare's (step, batch, offset) while the image size is not known yet
        if targets not in ("dense", "labels"):
            raise ValueError(f"DeviceAugment: targets is 'dense' or 'labels', got {targets!r}")
        self.targets = targets
        self.size = (int(size), int(size)) if isinstance(size, int) else tuple(int(v) for v in size)
        if len(self.size) != 2 or min(self.size) < 1:
            raise ValueError(f"DeviceAugment: size is a positive int or (h, w), got {size!r}")
        if channels not in (3, 4):
            raise ValueError(f"DeviceAugment: channels must be 3 or 4, got {channels}")
        if dtype not in (torch.bfloat16, torch.float16):
            raise TypeError(f"DeviceAugment: dtype must be torch.bfloat16 or torch.float16, got {dtype}")
        if mixup_alpha < 0 or cutmix_alpha < 0:
            raise ValueError("DeviceAugment: the alphas are not negative")
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"DeviceAugment: label_smoothing must lie in [0, 1), got {label_smoothing}")
        self.mixes = mixup_alpha > 0 or cutmix_alpha > 0
        if (self.mixes or label_smoothing > 0) and num_classes is None and targets == "dense":
            raise ValueError("DeviceAugment: mixup / cutmix / label smoothing form soft targets: give num_classes")
        _check_ids("DeviceAugment", seed, 0, 0)
        norm_constants(mean, std)
        self.pad, self.fill, self.flip = int(pad), int(fill), bool(flip)
        self.mean, self.std = tuple(mean), tuple(std)
        self.channels, self.dtype, self.seed = channels, dtype, int(seed)
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.mix_prob, self.switch_prob = float(mix_prob), float(switch_prob)
        self.label_smoothing, self.num_classes = float(label_smoothing), num_classes
        self.step = 0
        self.training = True
        self._block = None

    # ---- mode ---------------------------------------------------------------------------------
    def train(self, mode: bool = True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    # ---- state --------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, state: dict) -> None:
        _check_ids("DeviceAugment", state["seed"], 0, state["step"])
        self.seed, self.step = int(state["seed"]), int(state["step"])

    # ---- calls --------------------------------------------------------------------------------
    def draw(self, step: int) -> MixDraw:
        """The mixing of ``step`` (host)."""
        if not self.mixes:
            return MixDraw()
        return draw_mix(self.seed, 0, step, self.size, self.mixup_alpha, self.cutmix_alpha, self.mix_prob,
                        self.switch_prob)

    def _take_step(self, step):
        if step is None:
            step = self.step
            self.step += 1
        return int(step)

    @staticmethod
    def _offset(sample_offset, B: int) -> int:
        if sample_offset is not None:
            return int(sample_offset)
        from ..parallel import Initialized, local_rank
        return local_rank() * B if Initialized() else 0

    def block(self, device) -> torch.Tensor:
        """The device block (created on first use)."""
        device = torch.empty(0, device=device).device  # with its index
        if self._block is None or self._block.device != device:
            self._block = torch.zeros(BLOCK_WORDS, dtype=torch.int32, device=device)
            block_set(self._block, 0, MixDraw())
        return self._block

    def prepare(self, step=None, device=None, *, batch=None, sample_offset=None, image_size=None) -> MixDraw:
        """Write ``step``'s mixing into the device block (one launch; call it outside a captured region,
        before each replay). Returns the draw. ``crop="resized"``: also draws the boxes of the ``batch``
        samples of ``image_size = (H, W)`` and copies them into the persistent device table (created on
        first use for that ``batch``; one small copy from pageable memory, ordered with the stream)."""
        if device is None:
            device = self._block.device if self._block is not None else torch.device("cuda", torch.cuda.current_device())
        if self.crop == "resized":
            if batch is None:
                raise ValueError("DeviceAugment: with crop='resized' prepare needs batch=B (the table of boxes)")
            batch = int(batch)
            if self._table is not None and self._table.shape[0] != batch:
                raise ValueError(f"DeviceAugment: the device table of boxes was created for batch "
                                 f"{self._table.shape[0]}, got batch={batch}")
            if image_size is not None:
                self._image_size = tuple(int(v) for v in image_size)
        step = self._take_step(step)
        mix = self.draw(step)
        if self.crop == "resized":
            # the image size is not known before the first batch: the table is then written by the first
            # use_block call, which has to be outside a captured region (the usual warm-up call)
            self._pending = (step, batch, self._offset(sample_offset, batch))
            if self._image_size is not None:
                self._write_table(self.block(device).device)
        block_set(self.block(device), step, mix)
        return mix

    def _write_table(self, device) -> None:
        step, batch, offset = self._pending
        host = torch.from_numpy(self._boxes(batch, *self._image_size, step, offset))
        if self._table is None:
            self._table = host.to(device)
        else:
            self._table.copy_(host)
        self._pending = None

    def _boxes(self, B: int, H: int, W: int, step: int, offset: int) -> np.ndarray:
        return rrc_boxes(B, H, W, scale=self.scale, ratio=self.ratio, flip=self.flip, seed=self.seed, step=step,
                         sample_offset=offset)

    def _call_resized(self, images, labels, step, sample_offset, use_block, out):
        op = "DeviceAugment"
        common = dict(size=self.size, mean=self.mean, std=self.std, channels=self.channels, dtype=self.dtype, out=out)
        B, H, W, _, _ = _check_input("resized_crop_batch", images, self.size)
        if not self.training:
            if use_block:
                raise ValueError(f"{op}: use_block is for the training mode")
            return resized_crop_batch(images, center_boxes(B, H, W, self.size, self.crop_pct), **common), labels
        if use_block:
            if step is not None:
                raise ValueError(f"{op}: with use_block the step comes from prepare(step)")
            if not images.is_cuda:
                raise ValueError(f"{op}: use_block needs GPU tensors")
            if self._table is None and self._pending is not None and self._pending[1] == B:
                if torch.cuda.is_current_stream_capturing():
                    raise ValueError(f"{op}: the device table of boxes is written by the first use_block call, "
                                     "which must be outside a captured region (or give prepare image_size=(H, W))")
                self._image_size = (H, W)
                self._write_table(images.device)
            if self._table is None:
                raise ValueError(f"{op}: with crop='resized' and use_block, call prepare(step, batch=B) first")
            if self._table.shape[0] != B or self._image_size != (H, W) or self._table.device != images.device:
                raise ValueError(f"{op}: the device table of boxes is for {self._table.shape[0]} images of "
                                 f"{self._image_size} on {self._table.device}, got {B} of {(H, W)} on {images.device}")
            block = self.block(images.device)
            x = resized_crop_batch(images, self._table, dev_block=block, **common)
            return x, self._targets(labels, block_lam(block))
        self._image_size = (H, W)
        step = self._take_step(step)
        mix = self.draw(step)
        x = resized_crop_batch(images, self._boxes(B, H, W, step, self._offset(sample_offset, B)), mix=mix, **common)
        return x, self._targets(labels, mix.lam)

    def _targets(self, labels, lam):
        if labels is None:
            return None
        if not self.mixes and self.label_smoothing == 0:
            return labels
        if self.targets == "labels":
            return MixedLabels(labels, lam, self.label_smoothing)
        return mix_targets(labels, self.num_classes, lam, self.label_smoothing)

    def __call__(self, images, labels=None, step=None, *, sample_offset=None, use_block=False, out=None):
        if self.crop == "resized":
            return self._call_resized(images, labels, step, sample_offset, use_block, out)
        common = dict(size=self.size, pad=self.pad, fill=self.fill, mean=self.mean, std=self.std,
                      channels=self.channels, dtype=self.dtype, out=out)
        if not self.training:
            if use_block:
                raise ValueError("DeviceAugment: use_block is for the training mode")
            x = augment_batch(images, crop="center", flip=False, **common)
            return x, labels
        offset = self._offset(sample_offset, images.shape[0] if hasattr(images, "shape") and len(images.shape) else 0)
        if use_block:
            if step is not None:
                raise ValueError("DeviceAugment: with use_block the step comes from prepare(step)")
            if not images.is_cuda:
                raise ValueError("DeviceAugment: use_block needs GPU tensors")
            block = self.block(images.device)
            x = augment_batch(images, flip=self.flip, seed=self.seed, sample_offset=offset, dev_block=block, **common)
            return x, self._targets(labels, block_lam(block))
        step = self._take_step(step)
        mix = self.draw(step)
        x = augment_batch(images, flip=self.flip, seed=self.seed, step=step, sample_offset=offset, mix=mix, **common)
        return x, self._targets(labels, mix.lam)


__all__ = ["augment_batch", "augment_reference", "resized_crop_batch", "resized_crop_reference", "rrc_boxes",
           "center_boxes", "clamp_boxes", "sample_draws", "MixDraw", "draw_mix", "mix_targets", "DeviceAugment",
           "block_set", "block_lam", "norm_constants", "IMAGENET_MEAN", "IMAGENET_STD"]
