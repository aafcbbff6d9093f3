"""Philox4x32-10 and the stochastic bf16 rounding built on it, vectorised in numpy.

The CPU path of the ``sr=`` variants of the fused optimisers (``ops.optim``) and the oracle of the
GPU kernels (``csrc/kernels/optim_sr.h``): the same generator, the same counter layout, the same
integer arithmetic, so the two agree bit for bit.

Rounding ``sr(x, r)`` of an fp32 value with bits ``u`` and 16 random bits ``r``: the bf16 with bits
``(u + r) >> 16``; inf and NaN (exponent field all ones) take the round-to-nearest cast (inf as it is;
a NaN stays a NaN, here the quieted ``(u >> 16) | 0x40``: which NaN a cast yields is the platform's). A value
that bf16 represents is unchanged for every ``r``, the sign is kept (the add acts on the magnitude
bits), and the value moves away from zero with probability ``(u & 0xffff) / 65536`` exactly.

Random bits of element ``i`` of a leaf: ``e = offset + i``, ``q = e >> 3``, ``j = e & 7``; one
Philox call with key ``(seed & 0xffffffff, seed >> 32)`` and counter ``(q & 0xffffffff, q >> 32,
stream * 4 + slot, step)`` yields the words ``w0..w3`` and ``r = (w[j >> 1] >> (16 * (j & 1))) &
0xffff``. ``slot``: 0 the parameter, 1..3 the state tensors.
"""
from __future__ import annotations

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(counter, key, rounds: int = 10) -> np.ndarray:
    """Philox4x32 over arrays: ``counter`` ``[..., 4]`` and ``key`` ``[..., 2]`` (broadcast against
    each other) of 32-bit words; returns the ``[..., 4]`` uint32 output words."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(rounds):
        if r:
            k0 = (k0 + np.uint64(W0)) & _MASK
            k1 = (k1 + np.uint64(W1)) & _MASK
        p0 = np.uint64(M0) * c0  # 32 x 32 -> 64: no overflow in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def check_ids(seed: int, stream: int, slot: int, step: int) -> None:
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"stochastic rounding: seed must be in [0, 2^64), got {seed}")
    if not 0 <= int(stream) < 1 << 30:
        raise ValueError(f"stochastic rounding: stream must be in [0, 2^30), got {stream}")
    if not 0 <= int(slot) < 4:
        raise ValueError(f"stochastic rounding: slot must be 0..3, got {slot}")
    if not 0 <= int(step) < 1 << 32:
        raise ValueError(f"stochastic rounding: step must be a uint32, got {step}")


def random_bits(n: int, seed: int, stream: int, slot: int, step: int, offset: int = 0) -> np.ndarray:
    """The 16 random bits (uint32 array of ``n`` values below 65536) of elements ``offset ..
    offset + n`` of a leaf."""
    check_ids(seed, stream, slot, step)
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    offset = int(offset)
    q0, q1 = offset >> 3, (offset + n - 1) >> 3
    q = np.arange(q0, q1 + 1, dtype=np.uint64)
    ctr = np.stack([q & _MASK, q >> _S32, np.full_like(q, int(stream) * 4 + int(slot)), np.full_like(q, int(step))],
                   axis=-1)
    words = philox4x32(ctr, np.array([int(seed) & 0xFFFFFFFF, int(seed) >> 32], dtype=np.uint64))
    halves = np.stack([words & np.uint32(0xFFFF), words >> np.uint32(16)], axis=-1).reshape(-1)  # [q][w][lo, hi]
    lo = offset - (q0 << 3)
    return halves[lo:lo + n]


def sr_round(x: torch.Tensor, r) -> torch.Tensor:
    """``sr(x, r)`` per element: ``x`` fp32 (any shape, dense), ``r`` an array of as many 16-bit values in
    ``x``'s memory order (or one int for all). Returns bf16 of ``x``'s shape."""
    if x.dtype != torch.float32:
        raise TypeError(f"stochastic rounding rounds fp32 values, got {x.dtype}")
    xc = x.detach().cpu().contiguous()
    u = xc.view(torch.int32).numpy().view(np.uint32).reshape(-1)
    r = np.broadcast_to(np.asarray(r, dtype=np.uint32), u.shape)
    bits = ((u.astype(np.uint64) + r.astype(np.uint64)) >> np.uint64(16)).astype(np.uint16)
    special = (u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    if special.any():
        # what the round-to-nearest cast does to them: inf as it is, a NaN quieted (sign and upper payload kept)
        hi = (u >> np.uint32(16)).astype(np.uint16)
        rn = np.where((u & np.uint32(0x007FFFFF)) != 0, hi | np.uint16(0x0040), hi)
        bits = np.where(special, rn, bits)
    out = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16).reshape(xc.shape)
    return out.to(x.device)


def sr_reference(x: torch.Tensor, seed: int, stream: int = 0, slot: int = 0, step: int = 0,
                 offset: int = 0) -> torch.Tensor:
    """The stochastically rounded bf16 of the fp32 leaf ``x`` (elements in memory order, element ``i``
    being element ``offset + i`` of the random stream ``(seed, stream, slot, step)``)."""
    return sr_round(x, random_bits(x.numel(), seed, stream, slot, step, offset))


__all__ = ["philox4x32", "random_bits", "sr_round", "sr_reference", "check_ids"]
