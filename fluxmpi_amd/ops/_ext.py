"""Loader for the in-tree native extension ``fluxmpi_amd._C``.

``_C`` is one shared object, built by ``fluxmpi_amd/_build.py`` with hipcc for
gfx950, that contains

* the CDNA4 HIP kernels (multi-tensor pack/unpack/scale, fused Adam/SGD
  families, fused BatchNorm(+ReLU) for NHWC), and
* the native RCCL communicator (``csrc/comm/rccl_comm.cpp``).

The binding layer is plain pybind11 that takes raw device pointers and a HIP
stream handle, so the kernels are independent of the ATen C++ ABI and can be
launched on any PyTorch stream (including inside HIP-graph capture).

Policy: on a machine with a GPU the native path is mandatory. If the
extension is missing we raise :class:`NativeExtensionError` instead of
silently running an eager PyTorch fallback (``FLUXMPI_ALLOW_FALLBACK=1``
overrides this for debugging only). On CPU-only machines the kernels are not
needed: every op has a PyTorch reference implementation used for CPU tensors
and as the numerics oracle in tests.
"""
from __future__ import annotations

import importlib
import importlib.util
import os

import torch

from ..utils.errors import NativeExtensionError

_MOD = None
_TRIED = False
_ERR: Exception | None = None


def _try_import():
    global _MOD, _TRIED, _ERR
    if _TRIED:
        return _MOD
    _TRIED = True
    try:
        _MOD = importlib.import_module("fluxmpi_amd._C")
    except Exception as e:  # ImportError, or undefined-symbol OSError
        _MOD = None
        _ERR = e
    return _MOD


def available() -> bool:
    return _try_import() is not None


def gpu_present() -> bool:
    try:
        return torch.cuda.is_available()
    except Exception:
        return False


def get(required: bool = True):
    """Return the ``_C`` module.

    ``required=True`` raises when it cannot be imported. Callers handling CPU
    tensors pass ``required=False`` and use the PyTorch path on ``None``.
    """
    mod = _try_import()
    if mod is None and required:
        if os.environ.get("FLUXMPI_ALLOW_FALLBACK", "0") == "1":
            return None
        raise NativeExtensionError(
            "fluxmpi_amd._C (the gfx950 HIP extension) is not built or failed to load: "
            f"{_ERR!r}. Run `python -c 'import fluxmpi_amd; fluxmpi_amd.build()'`."
        )
    return mod


_EXTRA: dict = {}


def _extra(name: str, what: str):
    """A further pybind11 module ``fluxmpi_amd.<name>`` of the shared object ``_C`` was loaded from (its
    ``PyInit_<name>``): new entries get a module of their own, so ``_C`` itself keeps the surface
    ``tests/golden/c_api_surface.json`` records. Missing: an error, as for ``_C``."""
    if name not in _EXTRA:
        C = get(required=True)
        if C is None:
            raise NativeExtensionError(f"fluxmpi_amd.{name} needs the native extension fluxmpi_amd._C")
        spec = importlib.util.spec_from_file_location(f"fluxmpi_amd.{name}", C.__file__)
        try:
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        except Exception as e:
            raise NativeExtensionError(
                f"fluxmpi_amd.{name} ({what} of {C.__file__}) failed to load: {e!r}. "
                "Rebuild: `python -c 'import fluxmpi_amd; fluxmpi_amd.build()'`.") from e
        _EXTRA[name] = mod
    return _EXTRA[name]


def scale():
    """The ``_C_scale`` module: the fused optimisers' entries with the loss-scaling arguments
    (``dev_skip``, ``nonfinite_flag``, ``dev_pre``), ``mt_check_finite`` and ``loss_scale_update``."""
    return _extra("_C_scale", "the loss-scaling entries")


def ema():
    """The ``_C_ema`` module: ``mt_ema`` and ``ema_advance`` (the exponential moving average of the
    weights, ``csrc/kernels/optim_ema.hip``)."""
    return _extra("_C_ema", "the weight-EMA entries")


def sr():
    """The ``_C_sr`` module: the fused optimisers' entries with the stochastic-rounding arguments,
    ``mt_stochastic_round`` and ``sr_advance`` (``csrc/kernels/optim_sr.h``, ``optim_sr.hip``)."""
    return _extra("_C_sr", "the stochastic-rounding entries")


def c3ds():
    """The ``_C_c3ds`` module: ``conv3ds_bwd`` (the one-pass backward around the dual BatchNorm of a
    stage-1 downsample block, ``csrc/kernels/conv3ds_bwd.hip``)."""
    return _extra("_C_c3ds", "the downsample-block backward entry")


def bn2c3():
    """The ``_C_bn2c3`` module: ``bn_relu_conv1x1_fwd`` (bn2 apply + ReLU + conv3 forward of a bottleneck in
    one kernel, ``csrc/kernels/bn_relu_conv1x1_fwd.hip``)."""
    return _extra("_C_bn2c3", "the bn2 + conv3 forward entry")


def aug():
    """The ``_C_aug`` module: ``augment_batch`` and ``aug_block_set`` (the device input pipeline,
    ``csrc/kernels/augment.hip``)."""
    return _extra("_C_aug", "the input-pipeline entries")


def require_for(t: torch.Tensor):
    """The extension if ``t`` lives on the GPU (mandatory there), else ``None``."""
    if t.is_cuda:
        return get(required=True)
    return None
