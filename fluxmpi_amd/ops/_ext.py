"""Loader for the in-tree native extension ``fluxmpi_amd._C``.

``_C`` is one shared object and one Python module (``csrc/bindings.cpp``), built by
``fluxmpi_amd/_build.py`` with hipcc for gfx950, that contains

* the CDNA4 HIP kernels: the multi-tensor copies and fused optimisers (with gradient clipping, loss
  scaling, weight EMA and stochastic rounding), the normalisation, attention, GEMM and convolution
  kernels, the ResNet one-pass nodes, the DEQ cell and solver, the device input pipeline, and
* the native RCCL communicator (``csrc/comm/rccl_comm.cpp``).

Every native call goes through :func:`get`; a new entry is one more ``m.def`` in ``_C``
(``tests/test_bindings_surface.py`` says what may change in its surface). The exceptions go through
:func:`submodule`: the fused softmax cross-entropy entries (:func:`xent`, ``_C_xent``) and the
resized-crop entry (:func:`rrc`, ``_C_rrc``) are further pybind11 modules of the same shared object,
until ``_C``'s recorded surface is next re-recorded.

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


_SUB: dict = {}


def submodule(name: str, what: str):
    """A further pybind11 module ``fluxmpi_amd.<name>`` of the shared object ``_C`` was loaded from (its
    ``PyInit_<name>``); ``what`` names its entries in the error. Missing: an error, as for ``_C``."""
    mod = _SUB.get(name)
    if mod is None:
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
        _SUB[name] = mod
    return mod


def xent():
    """The ``_C_xent`` module (``xent_fwd``, ``xent_finish``, ``xent_bwd``; ``csrc/kernels/xent.hip``)."""
    return submodule("_C_xent", "the cross-entropy entries")


def rrc():
    """The ``_C_rrc`` module (``resized_crop_batch``; ``csrc/kernels/resize_crop.hip``)."""
    return submodule("_C_rrc", "the resized-crop entry")


def require_for(t: torch.Tensor):
    """The extension if ``t`` lives on the GPU (mandatory there), else ``None``."""
    if t.is_cuda:
        return get(required=True)
    return None
