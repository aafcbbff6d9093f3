"""``DDP``: the high-performance data-parallel training engine.

This is what the reference's step loop (per-leaf blocking,
host-staged allreduce inside ``Optimisers.update``) becomes when designed
for MI355X + RCCL over xGMI:

1. **Flat bucket views.** At construction every trainable parameter is moved
   into a contiguous per-bucket buffer and ``p.data`` / ``p.grad`` become
   strided views into it (channels_last weights keep their strides). Autograd
   then accumulates gradients straight into the communication buffer: there
   is no pack/unpack on the hot path and the optimiser runs over a few large
   flat buffers.
2. **Buckets in backward order.** Buckets are filled from the last parameter
   to the first (the order autograd produces gradients); the first bucket is
   small (``first_bucket_mb``, 4 MiB) so communication starts early, the rest
   are ``bucket_mb`` (16 MiB). Sizing: a ring allreduce over xGMI is per-link
   bound and pays ~10-30 us per collective, so buckets must be MBs; but the
   bucket that closes last (the first layers) is fully exposed after
   backward, and in a CNN most parameters sit in the LAST stages (ResNet-50:
   ~30 of 51 MB in layer4), so a 64 MiB bucket would hold back almost all
   traffic until backward ends. 16 MiB gives 4-5 bf16 buckets for ResNet-50,
   all but ~3 MB of them overlapped with the rest of backward.
3. **Backward/comm overlap.** A post-accumulate-grad hook per parameter counts
   down its bucket; a full bucket is allreduced immediately on the
   communicator's own HIP stream (fenced by an event recorded on
   the compute stream). Buckets are launched strictly in index order on every
   rank, so collectives can never be mismatched across ranks.
4. **Fused optimiser.** ``step()`` waits per bucket and runs one fused
   multi-tensor HIP kernel per bucket (Adam/AdamW/Descent/Momentum/Nesterov,
   RMSProp/AdaGrad/Lion/AdaMax/AMSGrad/NAdam/AdaBelief/AdaDelta, each also with
   WeightDecay, with Optimisers.jl numerics; optional fp32 master weights for bf16
   models). Step-dependent scalars (``beta^t``) live on the device, so the
   whole step can be captured in a HIP graph.
5. **Semantics.** Gradients are SUMmed like the reference; ``average=True``
   scales by ``1/world`` inside the optimiser kernel (free).
6. **World of one.** With nothing to communicate (world 1) the engine neither
   registers hooks nor packs: the fused optimiser reads autograd's gradient
   tensors in place (pointer lists, no copy into the flat buffer).
   ``force_comm=True`` (``FLUXMPI_FORCE_COMM=1``) runs the full N>1 path
   anyway — hooks, packing, real collectives on the communicator's stream
   with event fencing — so a single GPU exercises and measures it.

The Optimisers.jl-compatible state tree is available via
:meth:`DDP.optimiser_state` (``Leaf(rule, (mt, vt, βt))`` with tensor views
into the flat moment buffers).
"""
from __future__ import annotations

import math
import os
import weakref
from contextlib import contextmanager
from dataclasses import dataclass, field

import torch

from .. import optimisers as O
from ..ops import multi_tensor as mt
from ..ops import _ext
from ..ops import graddst
from ..ops import optim as fused
from ..utils.config import get_config
from ..utils import profiling
from ..utils.debug import Watchdog, check_replicas, check_same_structure
from . import runtime
from .comm import Communicator, ReduceOp


# module -> weakref to its engine: the engine holds the module strongly, so a strong value here
# would keep every engine ever built (model, flat buffers, masters, moments) alive for good
_ENGINES: "weakref.WeakKeyDictionary[torch.nn.Module, weakref.ref]" = weakref.WeakKeyDictionary()


def engine_for(module: torch.nn.Module) -> "DDP | None":
    """The DDP engine managing ``module`` (None if there is none, or it was discarded)."""
    ref = _ENGINES.get(module)
    return ref() if ref is not None else None


@dataclass
class LossScale:
    """Dynamic loss scaling (``torch.cuda.amp.GradScaler``'s rule) for :class:`DDP`.

    The loss is multiplied by ``scale`` (:meth:`DDP.scale_loss`) so that small fp16 gradients do not
    underflow; the update kernels divide it out again. A step whose reduced gradient holds an inf or
    a NaN is skipped and the scale multiplied by ``backoff``; after ``interval`` clean steps in a
    row it is multiplied by ``growth``. The scale stays in ``[min_scale, max_scale]``.
    ``growth = backoff = 1`` is a static scale (which still skips non-finite steps)."""
    init: float = 2.0 ** 16
    growth: float = 2.0
    backoff: float = 0.5
    interval: int = 2000
    min_scale: float = 1.0
    max_scale: float = 2.0 ** 24

    def __post_init__(self):
        vals = (self.init, self.growth, self.backoff, self.min_scale, self.max_scale)
        if not all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in vals):
            raise ValueError(f"LossScale: scales and factors are finite numbers, got {vals}")
        if self.init <= 0 or self.min_scale <= 0:
            raise ValueError(f"LossScale: the scale must be positive, got init={self.init} min_scale={self.min_scale}")
        if not self.min_scale <= self.init <= self.max_scale:
            raise ValueError(f"LossScale: need min_scale <= init <= max_scale, got {self.min_scale}, {self.init}, "
                             f"{self.max_scale}")
        if self.growth < 1.0:
            raise ValueError(f"LossScale: growth must be >= 1 (it raises the scale), got {self.growth}")
        if not 0.0 < self.backoff <= 1.0:
            raise ValueError(f"LossScale: backoff must be in (0, 1] (it lowers the scale), got {self.backoff}")
        if isinstance(self.interval, bool) or int(self.interval) != self.interval or self.interval < 1:
            raise ValueError(f"LossScale: interval is a positive number of steps, got {self.interval}")
        self.interval = int(self.interval)

    @staticmethod
    def parse(spec) -> "LossScale | None":
        """``None | "dynamic" | float | LossScale`` as :class:`DDP` takes it; a float is a static scale."""
        if spec is None or isinstance(spec, LossScale):
            return spec
        if isinstance(spec, str):
            if spec == "dynamic":
                return LossScale()
            raise ValueError(f"DDP: loss_scale is None, 'dynamic', a number or a LossScale, got {spec!r}")
        if isinstance(spec, bool) or not isinstance(spec, (int, float)):
            raise TypeError(f"DDP: loss_scale is None, 'dynamic', a number or a LossScale, got {type(spec).__name__}")
        v = float(spec)
        if not (math.isfinite(v) and v > 0):
            raise ValueError(f"DDP: a static loss scale must be positive and finite, got {spec}")
        return LossScale(init=v, growth=1.0, backoff=1.0, min_scale=v, max_scale=v)


@dataclass
class EMA:
    """Exponential moving average of the weights for :class:`DDP` (``timm``'s ``ModelEmaV2/V3``, the
    DeiT and "ResNet strikes back" recipes): after every ``every``-th applied optimiser step
    ``e <- e + (1 - d_t) (x - e)`` with ``x`` the fp32 master (else the parameter).

    ``warmup``: ``d_t = min(decay, (1 + n) / (10 + n))`` with ``n`` the EMA updates done so far, so
    that the first updates follow the weights closely; without it ``d_t = decay``. ``every > 1``
    updates the average on every ``every``-th applied step only (choose ``decay`` for that cadence)."""
    decay: float = 0.9999
    warmup: bool = True
    every: int = 1

    def __post_init__(self):
        d = self.decay
        if isinstance(d, bool) or not isinstance(d, (int, float)) or not 0.0 <= d < 1.0:
            raise ValueError(f"EMA: need 0 <= decay < 1, got {d!r}")
        if isinstance(self.every, bool) or not isinstance(self.every, (int, float)) \
                or int(self.every) != self.every or self.every < 1:
            raise ValueError(f"EMA: every is a positive number of steps, got {self.every!r}")
        self.decay, self.every, self.warmup = float(d), int(self.every), bool(self.warmup)

    @staticmethod
    def parse(spec) -> "EMA | None":
        """``None | float | EMA`` as :class:`DDP` takes it; a float is ``EMA(decay=float)``."""
        if spec is None or isinstance(spec, EMA):
            return spec
        if isinstance(spec, bool) or not isinstance(spec, (int, float)):
            raise TypeError(f"DDP: ema is None, a decay or an EMA, got {type(spec).__name__}")
        return EMA(decay=float(spec))


@dataclass
class _Bucket:
    index: int
    dtype: torch.dtype
    device: torch.device
    params: list
    offsets: list
    numel: int
    flat_param: torch.Tensor | None = None
    flat_grad: torch.Tensor | None = None
    master: torch.Tensor | None = None
    exp_avg: torch.Tensor | None = None
    exp_avg_sq: torch.Tensor | None = None
    state3: torch.Tensor | None = None  # third state buffer (AMSGrad's running maximum)
    pending: int = 0
    ready: bool = False
    launched: bool = False
    packed: bool = False
    work: object = None
    names: list = field(default_factory=list)
    comm_buf: torch.Tensor | None = None
    carry: torch.Tensor | None = None
    applied: bool = False  # overlap_opt: this step's update already enqueued (during backward)
    clip: torch.Tensor | None = None  # gradient clipping: [2, leaves] per-leaf sums of squares / scales
    partials: torch.Tensor | None = None  # ... and the sum-of-squares kernel's per-workgroup partials
    adapted: list = field(default_factory=list)  # LARS / LAMB: positions of the leaves that take the trust ratio
    plain: list = field(default_factory=list)    # ... and of the 1-D leaves that take Momentum / Adam
    ratios: torch.Tensor | None = None     # ... the adapted leaves' trust ratios (a slice of the dtype's table)
    lw_work: torch.Tensor | None = None    # ... and the layer-wise kernels' norm partials
    ema: torch.Tensor | None = None  # DDP(ema=...): the averaged weights, flat, fp32 (fp64 buckets: fp64)


def _strided_view(flat: torch.Tensor, like: torch.Tensor, offset: int) -> torch.Tensor:
    """A view of ``flat[offset:offset+numel]`` with ``like``'s sizes and (dense) strides."""
    return flat.as_strided(like.size(), like.stride(), flat.storage_offset() + offset)


def _same_layout(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same shape and the same strides on every dimension of size > 1 (memory order)."""
    return a.shape == b.shape and all(sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n > 1)


def _is_dense(t: torch.Tensor) -> bool:
    """Non-overlapping and dense (contiguous under some dim permutation)."""
    if t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last):
        return True
    dims = sorted(range(t.dim()), key=lambda d: t.stride(d))
    expect = 1
    for d in dims:
        if t.size(d) != 1 and t.stride(d) != expect:
            return False
        expect *= t.size(d)
    return True


class DDP:
    """Data-parallel wrapper: ``loss = ddp(x)...; loss.backward(); ddp.step()``.

    Parameters
    ----------
    module: the model (already on its device, in its compute dtype/memory format).
    rule:   an ``optimisers`` rule (Adam, Descent, Momentum, Nesterov, RMSProp, AdaGrad, Lion, AdaMax,
            AMSGrad, NAdam, AdaBelief, AdaDelta; all but the SGD family also in a chain with
            WeightDecay, as AdamW is; or the layer-wise LARS / LAMB, on their own: their decay is
            the rule's, their updates always run leaf by leaf and :meth:`trust_ratios` shows the
            ratios), optionally
            behind a clip: ``OptimiserChain(ClipNorm(omega), rule)`` (per-leaf L2 norm) or
            ``OptimiserChain(ClipGrad(delta), rule)``; the engine runs it with fused flat-buffer
            kernels (the clip inside the update kernel, the norms from a deterministic
            multi-tensor sum of squares on the updates' stream: over all buckets at once in
            ``step()``, in front of each bucket's update with ``overlap_opt``).
    clip_global_norm: clip the whole gradient to this L2 norm (``clip_grad_norm_`` semantics):
            ``step()`` takes every bucket's sum of squares once the last bucket is reduced, then
            runs all updates, which read one device scalar. Not with ``overlap_opt=True`` (an
            update cannot start before the last bucket is reduced) and not with a ``ClipNorm``
            chain; with ``ClipGrad`` the global scale is applied first.
            :meth:`grad_norm` returns the step's global gradient norm in either clip mode.
    loss_scale: ``None`` (default: nothing is launched that was not before), ``"dynamic"``
            (``LossScale()``), a number (a static scale, which still skips non-finite steps:
            ``loss_scale=1.0`` is the plain non-finite guard of a bf16 / fp32 model) or a
            :class:`LossScale`. Train on ``ddp.scale_loss(loss).backward()``. In ``step()``, on the
            updates' stream and without a host read (HIP-graph capturable): every bucket's reduced
            gradient is tested element by element for inf / NaN (inside the norm pass when the
            engine clips by a norm, else in one multi-tensor pass), every update kernel divides the
            scale out (norms and clamps see the unscaled gradient) and leaves at once when the test
            found something, and one thread then updates the scale. The test reads the REDUCED
            gradient, whose bits are the same on every rank, so the decision needs no collective
            and the replicas cannot disagree; an fp16 SUM that overflows on the wire is caught the
            same way and backs the scale off. A skipped step leaves parameters, masters, moments,
            ``beta^t`` and trust ratios bit-identical. Every bucket is tested before the first
            update, so not with ``overlap_opt=True``; and not with ``step(zero_grad=False)`` (two
            backwards at two scales cannot be summed in one carry; ``no_sync()`` accumulation
            between two steps is fine). :meth:`loss_scale`, :meth:`skipped_steps` and
            :meth:`step_skipped` read the scaler.
    ema:    ``None`` (default: nothing is allocated or launched that was not before), a decay
            (``EMA(decay=...)``) or an :class:`EMA`: the engine keeps an exponential moving average of
            the weights, one flat buffer per bucket in fp32 (fp64 buckets: fp64), taken from the fp32
            masters (the parameters where there are none) by one streaming kernel per bucket right
            behind the bucket's update, on its stream, with every rule, clip mode, ``loss_scale``,
            ``overlap_opt``, ``no_sync()``, ``step(zero_grad=False)`` and ``GraphedStep``. A step the
            loss scaler skips leaves the average, its update count and its decay bit-identical. The
            buffers are broadcast with the masters at construction and every rank then applies the
            same arithmetic to the same bits, so replicas stay equal without a collective per step.
            :meth:`ema_parameters`, :meth:`ema_decay` and :meth:`ema_updates` read it,
            :meth:`ema_state_dict` exports it, ``with ddp.ema_weights():`` evaluates with it, and
            :meth:`state_dict` carries it. Parameter changes from outside the engine do not reset it.
    master_weights: keep fp32 master copies (+ fp32 moments) for low-precision params.
    stochastic_rounding: ``None`` (default: nothing is allocated or launched that was not before),
            ``True`` (seed 0) or an int, the seed, the same on every rank. With
            ``master_weights=False`` the bf16 buckets' updates round every bf16 store — the parameter
            and the bf16 moments — stochastically (``ops.philox``: Philox4x32-10 inside the update
            kernels, the bucket index as stream, each leaf's offset in the bucket as its place in it,
            so the flat and the per-leaf route draw the same bits), which makes the 14 B per element
            layout without masters trainable: a store is unbiased, where round to nearest drops every
            update below half an ulp. fp32 and fp64 buckets are untouched. One device counter, advanced
            once per applied step (not by a step the loss scaler skips), read by :meth:`sr_step` and
            carried by :meth:`state_dict`. Every rank applies the same arithmetic to the same bits
            with the same random bits, so replicas stay equal. ``ValueError`` with
            ``master_weights=True`` or LARS / LAMB, ``TypeError`` with an fp16 bucket.
    average: divide the summed gradient by the world size (default False = reference SUM).
    overlap: launch bucket allreduces from backward hooks (default: ``FLUXMPI_OVERLAP``).
    broadcast: synchronise parameters and buffers from ``root_rank`` at construction.
    overlap_opt: per-bucket optimiser overlap (default ``FLUXMPI_OVERLAP_OPT``): as soon as a
            bucket's gradients are complete (and, when communicating, its allreduce is enqueued)
            its fused update is enqueued behind it — on the communicator's in-order stream, or on
            a side stream at world 1 — instead of after the whole backward in ``step()``. Safe
            because a bucket is complete only after every backward node that reads its
            parameters has run (a parameter's post-accumulate hook fires once, after all its
            uses); ``step()`` then only fences. Contract: every backward that completes buckets
            is followed by ``step()`` (no inspection of reduced-but-unapplied gradients).
    """

    def __init__(self, module: torch.nn.Module, rule: O.AbstractRule | None = None, *,
                 bucket_mb: float | None = None, first_bucket_mb: float | None = None,
                 master_weights: bool = True, average: bool = False, overlap: bool | None = None,
                 broadcast: bool = True, root_rank: int = 0, comm: Communicator | None = None,
                 comm_dtype: torch.dtype | None = None, watchdog: bool | None = None,
                 grad_mode: str | None = None, force_comm: bool | None = None,
                 tail_bucket_mb: float | None = None, overlap_opt: bool | None = None,
                 clip_global_norm: float | None = None, loss_scale=None, ema=None,
                 stochastic_rounding: bool | int | None = None):
        cfg = get_config()
        self._sr_seed = None
        if stochastic_rounding is not None and stochastic_rounding is not False:
            if master_weights:
                raise ValueError("DDP: stochastic_rounding rounds the bf16 parameters and moments themselves; it "
                                 "replaces the fp32 masters: pass master_weights=False")
            self._sr_seed = 0 if stochastic_rounding is True else int(stochastic_rounding)
            if not 0 <= self._sr_seed < 1 << 64:
                raise ValueError(f"DDP: stochastic_rounding seed must be in [0, 2^64), got {stochastic_rounding}")
        self._ls = LossScale.parse(loss_scale)
        self._ema = EMA.parse(ema)
        self._ema_swapped = False  # inside `with ema_weights():`
        if self._ls is not None and overlap_opt:
            raise ValueError("DDP: loss_scale tests every bucket's gradient before the first update, so the "
                             "updates cannot overlap with backward: drop overlap_opt=True")
        if clip_global_norm is not None and overlap_opt:
            raise ValueError("DDP: clip_global_norm needs every bucket's norm before the first update, so the "
                             "updates cannot overlap with backward: drop overlap_opt=True")
        self.clip_global_norm = None if clip_global_norm is None else float(clip_global_norm)
        # "steal": autograd hands over each freshly produced gradient (no in-place accumulate
        # kernel per parameter, no zero fill) and one multi-tensor launch per bucket packs them
        # into the flat buffer; "view": p.grad is a view into the flat buffer (autograd adds in).
        self.grad_mode = grad_mode or cfg.extra.get("grad_mode", "steal")
        if self.grad_mode not in ("steal", "view"):
            raise ValueError(f"DDP: grad_mode must be 'steal' or 'view', got {self.grad_mode!r}")
        self.module = module
        self.rule = rule if rule is not None else O.Adam()
        self.average = average
        self.overlap = cfg.overlap if overlap is None else overlap
        self.master_weights = master_weights
        params = [p for p in module.parameters() if p.requires_grad]
        if not params:
            raise ValueError("DDP: module has no trainable parameters")
        self.device = params[0].device
        if comm is None:
            comm = runtime.comm_for(params[0]) if runtime.Initialized() else None
        self.comm = comm
        self.world = comm.size if comm is not None else 1
        self.force_comm = cfg.force_comm if force_comm is None else bool(force_comm)
        if self.force_comm and comm is None:
            raise RuntimeError("DDP(force_comm=True) needs a communicator: call fluxmpi_amd.Init() first")
        # collectives are issued whenever there is a peer, or when forced (world-1 rehearsal)
        self.communicate = comm is not None and (self.world > 1 or self.force_comm)
        # measurement tool (FLUXMPI_EMULATE_COMM="WGS:GBPS[:THREADS[:LDS_KB]]"): with each bucket's
        # collective, hold WGS workgroups (THREADS threads, LDS_KB of LDS each) on the comm stream
        # for the time a ring allreduce of the bucket would take at GBPS bus bandwidth on 8
        # ranks — RCCL's CU footprint, which a world of one lacks
        self._emulate = None
        emu = cfg.extra.get("emulate_comm") or os.environ.get("FLUXMPI_EMULATE_COMM", "")
        if emu and self.communicate and self.device.type == "cuda":
            f = emu.split(":")
            self._emulate = (int(f[0]), float(f[1]), int(f[2]) if len(f) > 2 else 256,
                             int(f[3]) * 1024 if len(f) > 3 else 0)
        if comm_dtype is None:
            comm_dtype = {"fp32": torch.float32, "float32": torch.float32, "bf16": torch.bfloat16,
                          "bfloat16": torch.bfloat16, "fp16": torch.float16}.get(cfg.comm_dtype)
        self.comm_dtype = comm_dtype
        # measured bucket plan (parallel/bucket_plan.py): at N > 1, unless sizes were given
        self.bucket_plan, self.comm_probe = "default", None
        explicit = bucket_mb is not None or first_bucket_mb is not None or tail_bucket_mb is not None \
            or cfg.buckets_explicit
        if self.communicate and self.world > 1 and (cfg.bucket_plan == "measured"
                                                    or (cfg.bucket_plan == "auto" and not explicit)):
            from . import bucket_plan as BP
            nbytes: dict = {}
            for p in params:
                nbytes[p.dtype] = nbytes.get(p.dtype, 0) + p.numel() * p.element_size()
            wire = comm_dtype or max(nbytes, key=nbytes.get)
            plan, rec = BP.measured_plan(comm, self.device, wire, sum(nbytes.values()),
                                         cpu_comm=runtime.cpu_comm() if runtime.Initialized() else None)
            bucket_mb, first_bucket_mb, tail_bucket_mb = plan["bucket_mb"], plan["first_bucket_mb"], plan["tail_bucket_mb"]
            self.bucket_plan, self.comm_probe = "measured", {"samples": rec, "plan": plan}
        bb = int((bucket_mb if bucket_mb is not None else cfg.bucket_mb) * (1 << 20))
        fb = int((first_bucket_mb if first_bucket_mb is not None else cfg.first_bucket_mb) * (1 << 20))
        tb = int((tail_bucket_mb if tail_bucket_mb is not None else cfg.tail_bucket_mb) * (1 << 20))
        names = {id(p): n for n, p in module.named_parameters()}
        self.buckets = self._build_buckets(params, bb, fb, names, tb)
        self._param_bucket = {}
        for b in self.buckets:
            for p in b.params:
                self._param_bucket[id(p)] = b
        # direct delivery ("steal" mode with collectives): the package's weight-gradient kernels
        # allocate each parameter's gradient in its bucket slice (ops/graddst.py), so the
        # per-bucket pack finds it in place (the pack was one copy kernel per bucket)
        self.direct_grads = bool(cfg.direct_grads) and self.communicate and self.grad_mode == "steal"
        for b in self.buckets:
            for p, o in zip(b.params, b.offsets):
                if self.direct_grads:
                    graddst.attach(p, b.flat_grad, o)
                else:
                    graddst.detach(p)  # a previous engine's buckets are not this one's
        self._hooks = []
        self._sync_enabled = True
        # per-bucket optimiser overlap: on the communicator's in-order stream (behind the bucket's
        # allreduce) when it has one, on a side stream when nothing is communicated, else in
        # step() (host-synchronous collectives: nothing to overlap with)
        want_opt = cfg.overlap_opt if overlap_opt is None else bool(overlap_opt)
        if self.clip_global_norm is not None or self._ls is not None:
            want_opt = False
        self.overlap_opt = want_opt and self.overlap and self.grad_mode == "steal"
        self._opt_stream = None  # None: the update runs right after the (host-waited) reduction
        if self.overlap_opt and self.device.type == "cuda":
            if not self.communicate:
                self._opt_stream = torch.cuda.Stream(self.device)
            elif getattr(comm, "in_order", False) and getattr(comm, "stream", None) is not None:
                self._opt_stream = comm.stream
        if self.overlap and (self.communicate or self.overlap_opt):
            for p in params:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._on_grad_ready))
        self._setup_optimizer()
        self.debug_checks = cfg.debug_checks
        self.watchdog = None
        if self.world > 1 and runtime.Initialized():
            # every rank must build the same bucket plan, or collectives would mismatch
            check_same_structure([(str(b.dtype), b.numel, len(b.params)) for b in self.buckets],
                                 comm=runtime.cpu_comm(), what="DDP bucket plan")
        if self.communicate and runtime.Initialized():
            if watchdog if watchdog is not None else cfg.extra.get("watchdog", True):
                self.watchdog = Watchdog(comm, timeout_s=cfg.timeout_s)
        if broadcast and self.communicate:
            self.broadcast_parameters(root_rank)
        self._next_launch = 0
        self._direct_cache: dict = {}
        self._views: dict = {}
        self._record_versions()
        self._carry_live = False
        self._carry_hook = None
        self.collectives_launched = 0  # gradient-bucket allreduces issued so far
        self.pack_copies = 0  # gradients the bucket packs had to copy (not delivered in place)
        self.pack_copied: dict = {}  # shape -> copies (which producers still miss their slices)
        _ENGINES[module] = weakref.ref(self)
        self.zero_grad()
        self.step_count = 0
        # exposed-communication timing (off by default: event timing costs a little)
        self.timing = bool(cfg.profile)
        self._comm_events: list = []

    # ------------------------------------------------------------------ setup
    @staticmethod
    def _taper(group: list, esz: int, tail_bytes: int) -> list:
        """Split the bucket that closes LAST (the first layers: their gradients come at the very
        end of backward, so its whole allreduce is exposed) into pieces that grow geometrically
        towards the front: from the end, at most tail, 2 tail, 4 tail, ... bytes. The layers
        before the final tail then launch mid-backward and only ``tail_bytes`` stay exposed
        (ResNet-50's last 14 MB bucket mixed layer3, ready mid-backward,
        with layer1 / stem)."""
        out, cur, cur_bytes, cap = [], [], 0, tail_bytes
        for p in reversed(group):  # from the parameter whose gradient comes last
            nb = p.numel() * esz
            if cur and cur_bytes + nb > cap:
                out.append(list(reversed(cur)))
                cur, cur_bytes, cap = [], 0, cap * 2
            cur.append(p)
            cur_bytes += nb
        if cur:
            out.append(list(reversed(cur)))
        out.reverse()
        if len(out) > 1 and sum(p.numel() for p in out[0]) * esz < tail_bytes:
            out[1] = out[0] + out[1]  # no sliver bucket at the front: one collective fewer
            out.pop(0)
        return out

    def _build_buckets(self, params, bucket_bytes, first_bytes, names, tail_bytes=0):
        rev = list(reversed(params))
        by_dtype: dict = {}
        for p in rev:
            by_dtype.setdefault(p.dtype, []).append(p)
        buckets: list[_Bucket] = []
        for dt, ps in by_dtype.items():
            esz = torch.empty((), dtype=dt).element_size()
            groups, cur, cur_bytes = [], [], 0
            limit = first_bytes
            for p in ps:
                nb = p.numel() * esz
                if cur and cur_bytes + nb > limit:
                    groups.append(cur)
                    cur, cur_bytes, limit = [], 0, bucket_bytes
                cur.append(p)
                cur_bytes += nb
            if cur:
                groups.append(cur)
            if tail_bytes > 0 and len(groups) > 1:
                groups = groups[:-1] + self._taper(groups[-1], esz, tail_bytes)
            for g in groups:
                buckets.append(self._make_bucket(len(buckets), dt, g, names))
        # launch order = expected completion order: a bucket is ready when its LAST parameter
        # (in backward order) has its gradient. Ordering by the first parameter instead would
        # put a small bucket of another dtype (ResNet's fp32 BatchNorm parameters, spread over
        # the whole network) early in the sequence and hold every later bucket's allreduce
        # until the end of backward. Identical on every rank (built from the parameter list).
        order = {id(p): i for i, p in enumerate(rev)}
        buckets.sort(key=lambda b: max(order[id(p)] for p in b.params))
        for i, b in enumerate(buckets):
            b.index = i
        return buckets

    def _make_bucket(self, idx, dtype, params, names):
        for p in params:
            if not _is_dense(p):
                raise ValueError(f"DDP: parameter {names.get(id(p))} is not dense")
        offs, total = mt.aligned_offsets([p.numel() for p in params], dtype)
        dev = params[0].device
        flat_p = torch.zeros(total, dtype=dtype, device=dev)
        flat_g = torch.zeros(total, dtype=dtype, device=dev)
        with torch.no_grad():
            for p, o in zip(params, offs):
                v = _strided_view(flat_p, p, o)
                v.copy_(p.data)
                p.data = v
                if self.grad_mode == "view":
                    p.grad = _strided_view(flat_g, p, o)
        return _Bucket(idx, dtype, dev, list(params), offs, total, flat_p, flat_g,
                       names=[names.get(id(p), "?") for p in params])

    def _setup_optimizer(self):
        r = self.rule
        # a leading ClipNorm(p=2) / ClipGrad of a chain rides in the update kernels
        self._clip_rule, self._chain_where = None, None
        if isinstance(r, O.OptimiserChain):
            plan = r.fused_plan(engine=True)
            if plan is None:
                raise TypeError(f"DDP: no fused kernel for rule {r!r}; use the functional optimisers API")
            self._clip_rule, r, self._chain_where = plan
        self._per_leaf = isinstance(self._clip_rule, O.ClipNorm)
        if self._per_leaf and self.clip_global_norm is not None:
            raise ValueError("DDP: clip_global_norm and a ClipNorm chain both rescale by a norm; use one of them")
        self._norms = self._per_leaf or self.clip_global_norm is not None
        self._upd = r  # the update rule behind the clip
        self.wd = 0.0
        if isinstance(r, O.OptimiserChain):  # the plan's (rule, WeightDecay) pair
            r, self.wd = r.opts[0], r.opts[1].gamma
        self._inner = r  # the rule whose kernel runs
        if isinstance(r, O.Adam):
            self.kind, self.adam = "adam", r
        elif isinstance(r, O._KernelRule):
            self.kind = r._kind
        elif isinstance(r, O.LARS):
            self.kind = "lars"
        elif isinstance(r, O.LAMB):
            self.kind = "lamb"
        elif isinstance(r, O.Nesterov):
            self.kind = "nesterov"
        elif isinstance(r, O.Momentum):
            self.kind = "momentum"
        elif isinstance(r, O.Descent):
            self.kind = "descent"
        else:
            raise TypeError(f"DDP: no fused kernel for rule {r!r}; use the functional optimisers API")
        # the kernel rules of ops.optim.rule_: state buffers per bucket, and whether beta^t is kept
        _, self._nstate, self._has_bt = fused.RULES.get(self.kind, (None, 0, self.kind in ("adam", "lamb")))
        self._layerwise = self.kind in fused.LAYERWISE
        if self.kind == "lars" and self.clip_global_norm is not None:
            raise ValueError("DDP: LARS rescales every leaf's gradient by its own norm, which undoes a global "
                             "clip: drop clip_global_norm (LAMB takes it)")
        dev = self.device
        # stochastic rounding: the generator's step counter {uint32 step, 7 unused} on the device
        self._sr_block = None
        if self._sr_seed is not None:
            if self._layerwise:
                raise ValueError(f"DDP: stochastic_rounding has no {self.kind.upper()} kernels")
            if any(b.dtype == torch.float16 for b in self.buckets):
                raise TypeError("DDP: stochastic_rounding is defined for bf16 parameters; this model has fp16 ones")
            self._sr_block = fused.sr_block(dev)
        for b in self.buckets:
            low = b.dtype in (torch.bfloat16, torch.float16)
            use_master = self.master_weights and low
            sdt = torch.float32 if use_master else b.dtype
            if use_master:
                b.master = b.flat_param.float()
            if self.kind in ("adam", "lamb"):
                b.exp_avg = torch.zeros(b.numel, dtype=sdt, device=dev)
                b.exp_avg_sq = torch.zeros(b.numel, dtype=sdt, device=dev)
            elif self.kind in ("momentum", "nesterov", "lars"):
                b.exp_avg = torch.zeros(b.numel, dtype=sdt, device=dev)
            elif self._nstate:
                # AdaGrad's and AMSGrad's states start at epsilon (Optimisers.jl init), the rest at 0
                fill = float(r.epsilon) if self.kind in ("adagrad", "amsgrad") else 0.0
                bufs = [torch.full((b.numel,), fill, dtype=sdt, device=dev) for _ in range(self._nstate)]
                b.exp_avg, b.exp_avg_sq, b.state3 = (bufs + [None, None])[:3]
        # gradient norms: per bucket dtype one [2, leaves] buffer of per-leaf sums of squares and
        # scales and one of the sum-of-squares kernel's partials; every bucket owns a slice, so the
        # norms of all buckets can be taken in one multi-tensor call (step()) or bucket by bucket
        # (overlap_opt)
        self._clip_groups = []
        if self._norms:
            by_dtype: dict = {}
            for b in self.buckets:
                by_dtype.setdefault(b.dtype, []).append(b)
            for dt, bs in by_dtype.items():
                at = torch.float64 if dt == torch.float64 else torch.float32
                buf = torch.zeros(2, sum(len(b.params) for b in bs), dtype=at, device=dev)
                parts = torch.zeros(sum(fused.sumsq_partials(b.params) for b in bs), dtype=at, device=dev)
                off = poff = 0
                for b in bs:
                    k, kp = len(b.params), fused.sumsq_partials(b.params)
                    b.clip, b.partials = buf[:, off:off + k], parts[poff:poff + kp]
                    off, poff = off + k, poff + kp
                self._clip_groups.append((bs, buf, parts))
        # layer-wise rules: each bucket's leaves split once into adapted and 1-D ones, and per bucket
        # dtype one table of trust ratios and one workspace of norm partials, a slice per bucket
        if self._layerwise:
            by_dtype = {}
            for b in self.buckets:
                b.adapted = [i for i, p in enumerate(b.params) if r._adapts(p)]
                b.plain = [i for i, p in enumerate(b.params) if not r._adapts(p)]
                by_dtype.setdefault(b.dtype, []).append(b)
            for dt, bs in by_dtype.items():
                at = torch.float64 if dt == torch.float64 else torch.float32
                need = [fused.layerwise_workspace([b.params[i] for i in b.adapted]) for b in bs]
                table = torch.ones(sum(len(b.adapted) for b in bs), dtype=at, device=dev)
                work = torch.zeros(sum(need), dtype=at, device=dev)
                off = woff = 0
                for b, kw in zip(bs, need):
                    b.ratios, b.lw_work = table[off:off + len(b.adapted)], work[woff:woff + kw]
                    off, woff = off + len(b.adapted), woff + kw
        # [sum of squares, norm, global clip scale] of the step's whole gradient (device, fp32)
        self._clip_slot = torch.zeros(3, dtype=torch.float32, device=dev) if self._norms else None
        # loss scaling: the scaler's device block {scale, 1/scale, growth tracker, skipped steps, last
        # step skipped, non-finite flag} and the views the kernels and the accessors take of it
        self._ls_block = None
        if self._ls is not None:
            self._ls_block = fused.loss_scale_block(self._ls.init, dev)
            f = self._ls_block.view(torch.float32)
            self._ls_scale, self._ls_inv = f[fused.LS_SCALE], f[fused.LS_INV:fused.LS_INV + 1]
            self._ls_flag = self._ls_block[fused.LS_FLAG:fused.LS_FLAG + 1]
        # weight EMA: per bucket one flat buffer in compute precision, started from the master (else the
        # parameters) leaf by leaf, so that the alignment padding between leaves is zero: finite. And the
        # EMA device block {1 - d_t, d_t, updates, steps since the last one, hold}
        self._ema_block = None
        if self._ema is not None:
            for b in self.buckets:
                b.ema = torch.zeros(b.numel, dtype=torch.float64 if b.dtype == torch.float64 else torch.float32,
                                    device=dev)
                self._ema_restart(b)
            self._ema_block = fused.ema_block(self._ema.decay, self._ema.warmup, self._ema.every, dev)
        if self._has_bt:
            a = self._inner
            # device hyper block [lr, beta1^t, beta2^t]; beta^t starts at beta (Optimisers.jl init)
            self.hyper = torch.tensor([a.eta, a.beta[0], a.beta[1]], dtype=torch.float32, device=dev)
        else:  # [lr]; AdaDelta has no learning rate (the entry is not read)
            self.hyper = torch.tensor([getattr(self._inner, "eta", 0.0)], dtype=torch.float32, device=dev)

    def broadcast_parameters(self, root_rank: int = 0):
        """One broadcast per flat bucket (+ its fp32 master) + module buffers (``synchronize``
        of the model). Broadcasting the masters keeps them bit-identical on every rank."""
        if hasattr(self, "_versions"):
            self._sync_masters()  # the root's outside edits reach its master before it is sent
        with torch.no_grad():
            for b in self.buckets:
                self.comm.broadcast(b.flat_param, root_rank)
                if b.master is not None:
                    self.comm.broadcast(b.master, root_rank)
                if b.ema is not None:  # replicas start from one average and apply the same arithmetic to it
                    self.comm.broadcast(b.ema, root_rank)
            # buffers and the parameters outside every bucket (requires_grad=False: a frozen
            # backbone or embedding) — the reference's synchronize! reaches every leaf
            bucketed = {id(p) for b in self.buckets for p in b.params}
            rest, seen = [], set()
            for t in list(self.module.parameters()) + list(self.module.buffers()):
                if id(t) not in bucketed and id(t) not in seen and t.numel() > 0:
                    seen.add(id(t))
                    rest.append(t.detach())
            if rest:
                from .bucket import broadcast_tensors
                broadcast_tensors(rest, root_rank, comm=self.comm, force_comm=self.force_comm)
        if hasattr(self, "_versions"):
            self._record_versions()  # params and masters were written together: nothing stale

    # ------------------------------------------------------------------ hooks
    @contextmanager
    def no_sync(self):
        """Gradient accumulation: backward passes inside do not launch allreduces."""
        prev, self._sync_enabled = self._sync_enabled, False
        try:
            yield
        finally:
            self._sync_enabled = prev

    def _on_grad_ready(self, p):
        if not self._sync_enabled:
            return
        b = self._param_bucket[id(p)]
        if b.pending <= 0 or b.launched:
            # a second backward reached this bucket before step(): its first gradients are
            # already being reduced (and, with overlap_opt, applied to the weights the second
            # backward may have read) — accumulating into them would silently drop or corrupt
            # the update, so refuse loudly (accumulate under no_sync() instead)
            raise RuntimeError(
                f"DDP: a second backward reached gradient bucket {b.index} before step(); its "
                "gradients were already " + ("reduced and applied" if self.overlap_opt else "sent for reduction")
                + ". Accumulate gradients inside `with ddp.no_sync():` and run the last backward "
                "outside it, then step()")
        b.pending -= 1
        if b.pending == 0:
            b.ready = True
            self._launch_ready()

    def _launch_ready(self):
        while self._next_launch < len(self.buckets) and self.buckets[self._next_launch].ready:
            self._launch(self.buckets[self._next_launch])
            self._next_launch += 1

    def _launch(self, b: _Bucket):
        if b.launched:
            return
        b.launched = True
        if self.overlap_opt and not self._masters_synced:
            self._sync_masters()  # outside edits reach the masters before the step's first update
            self._masters_synced = True
        if self.communicate:
            self._launch_comm(b)
        if self.overlap_opt:
            self._apply_overlapped(b)

    def _apply_overlapped(self, b: _Bucket):
        """Enqueue bucket ``b``'s update now. Communicating: behind its allreduce on the in-order
        comm stream (stream order is the dependency: no fence, no host wait). World 1: on the
        side stream, after an event on the compute stream (the bucket's gradients are produced
        there) — the compute stream goes on with backward."""
        gscale = 1.0 / self.world if self.average else 1.0
        st = self._opt_stream
        if st is None:
            # no in-order device stream (CPU tensors, gloo on device tensors): wait for the
            # reduction here, then update on the current stream — the same order, no overlap
            if self.communicate:
                self._finish(b)
                self._add_carry(b)
                self._apply(b, gscale)
            elif not self._apply_direct(b, gscale):
                self._pack(b)
                self._apply(b, gscale)
            b.applied = True
            return
        if not self.communicate:
            st.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(st):
            if self.communicate:
                if b.comm_buf is not None and self.comm_dtype != b.dtype:
                    mt.unpack(b.comm_buf, [b.flat_grad], [0])
                self._add_carry(b)
                self._apply(b, gscale)
            elif not self._apply_direct(b, gscale):
                self._pack(b)
                self._apply(b, gscale)
        b.applied = True

    def _launch_comm(self, b: _Bucket):
        self._pack(b)
        buf = b.flat_grad
        if self.comm_dtype is not None and self.comm_dtype != b.dtype:
            # K5: cast the bucket to the wire dtype (e.g. fp32 grads sent as bf16) in one launch
            if b.comm_buf is None:
                b.comm_buf = torch.empty(b.numel, dtype=self.comm_dtype, device=b.device)
            mt.pack([b.flat_grad], b.comm_buf, [0])
            buf = b.comm_buf
        with profiling.range(f"fluxmpi.allreduce.bucket{b.index}"):
            if self._emulate is not None and hasattr(self.comm, "stream"):
                wgs, gbps, thr, lds = self._emulate
                nbytes = buf.numel() * buf.element_size()
                us = 2.0 * 7.0 / 8.0 * nbytes / (gbps * 1e3)  # ring allreduce, 8 ranks
                self.comm.stream.wait_stream(torch.cuda.current_stream(self.device))
                _ext.get(required=True).emulate_comm(wgs, max(us, 5.0), self.comm.stream.cuda_stream, thr, lds)
            b.work = self.comm.allreduce(buf, ReduceOp.SUM, async_op=True)
        self.collectives_launched += 1
        if self.watchdog is not None:
            self.watchdog.track(b.work, f"allreduce of gradient bucket {b.index} ({b.numel} elements)")

    # ------------------------------------------------------------------ public
    def __call__(self, *args, **kw):
        return self.module(*args, **kw)

    forward = __call__

    def zero_grad(self):
        """Reset the gradients and re-arm the hooks. "view" mode zeroes the flat buffers (one
        fill launch per dtype); "steal" mode drops the per-step gradient tensors."""
        if self.grad_mode == "view":
            mt.fill_([b.flat_grad for b in self.buckets], 0.0)
        self._drop_carry()
        self._rearm()
        for b in self.buckets:
            for p, o in zip(b.params, b.offsets):
                if self.grad_mode == "steal":
                    p.grad = None
                elif p.grad is None or p.grad.data_ptr() != b.flat_grad.data_ptr() + o * b.flat_grad.element_size():
                    # someone replaced .grad (e.g. set_to_none): restore the view
                    p.grad = _strided_view(b.flat_grad, p, o)

    def _rearm(self):
        """Reset the per-step bucket state (countdowns, launch/pack flags) for the next backward."""
        for b in self.buckets:
            b.pending = len(b.params)
            b.ready = b.launched = b.packed = b.applied = False
            b.work = None
            if getattr(self, "direct_grads", False):
                for p in b.params:
                    graddst.rearm(p)
        self._next_launch = 0
        self._masters_synced = False
        self._norm_started = False  # clipping: the step's first bucket starts the global sum afresh
        self._deferred = []  # norm clipping in step(): the updates wait for all buckets' norms

    def _note_copy(self, p) -> None:
        self.pack_copies += 1
        key = "x".join(str(d) for d in p.shape)
        self.pack_copied[key] = self.pack_copied.get(key, 0) + 1

    def _pack(self, b: _Bucket):
        """"steal" mode: copy the bucket's gradients into its flat buffer, one multi-tensor launch.

        Autograd's layout contract gives every gradient its parameter's (dense) strides, and the
        flat slice is a view with the same strides, so a raw copy of ``numel`` elements is exact.
        Parameters that received no gradient get zeros.
        """
        if self.grad_mode != "steal" or b.packed:
            return
        b.packed = True
        views = self._grad_views(b)
        srcs, dptrs, ns = [], [], []
        for p, dst, dptr in views:
            g = p.grad
            if g is None:
                dst.zero_()
            elif g.data_ptr() == dptr:
                if not _same_layout(g, dst):
                    dst.copy_(g.clone())
                    self._note_copy(p)
                # else already in place (delivered by the producing op, or p.grad set to the view)
            elif g.dtype is b.dtype and g.is_cuda and g.stride() == dst.stride():
                # the common case: autograd's layout contract (the parameter's dense strides)
                srcs.append(g)
                dptrs.append(dptr)
                ns.append(dst.numel())
                self._note_copy(p)
            elif g.is_cuda and g.dtype == b.dtype and _same_layout(g, p) and _is_dense(g):
                srcs.append(g)
                dptrs.append(dptr)
                ns.append(dst.numel())
                self._note_copy(p)
            else:
                dst.copy_(g)
                self._note_copy(p)
        if srcs:
            C = _ext.get(required=True)
            code = mt.DTYPE_CODE[b.dtype]
            C.mt_copy([g.data_ptr() for g in srcs], dptrs, ns, code, code, 1.0,
                      torch.cuda.current_stream(b.device).cuda_stream)
        # from here on p.grad aliases the (soon reduced) flat buffer, as in "view" mode
        for p, dst, _ in views:
            p.grad = dst

    def _grad_views(self, b: _Bucket) -> list:
        """``(param, view of its flat-gradient slice, slice address)`` per parameter (cached)."""
        v = self._views.get(b.index)
        if v is None:
            es = b.flat_grad.element_size()
            base = b.flat_grad.data_ptr()
            v = [(p, _strided_view(b.flat_grad, p, o), base + o * es) for p, o in zip(b.params, b.offsets)]
            self._views[b.index] = v
        return v

    def reduce_gradients(self):
        """Make sure every bucket has been allreduced (launch the rest, in order) and wait."""
        if self.overlap_opt:
            raise RuntimeError("DDP.reduce_gradients: with overlap_opt the updates run with the "
                               "reductions; call step() (or build the engine with overlap_opt=False)")
        for b in self.buckets:
            b.ready = True
        self._launch_ready()
        for b in self.buckets:
            self._pack(b)
            self._finish(b)

    def _fence_all(self):
        """One compute-stream fence for all buckets when the communicator runs every collective on
        one in-order stream (RcclComm): waiting for the last bucket's event covers the others. A
        cross-queue wait costs the compute queue a dependency round trip each (measured: the
        eager --force-comm step paid ~0.3 ms over 5 per-bucket waits, the captured graph none)."""
        if not getattr(self.comm, "in_order", False):
            return
        works = [b.work for b in self.buckets if b.work is not None]
        if len(works) < 2 or not all(hasattr(w, "covered") for w in works):
            return
        works[-1].wait()
        for w in works[:-1]:
            w.covered()

    def _finish(self, b: _Bucket):
        """Make the compute stream wait for bucket ``b``'s allreduce (and cast it back)."""
        if b.work is not None:
            b.work.wait()
            b.work = None
            if b.comm_buf is not None and self.comm_dtype != b.dtype:
                mt.unpack(b.comm_buf, [b.flat_grad], [0])

    def _arm_carry(self):
        """``step(zero_grad=False)`` with communication: the flat buffers hold the REDUCED sum
        S1. Accumulating the next backward into them and reducing again would apply
        ``W*S1 + S2``; the reference semantics (gradients summed over ranks, then applied:
        ``/root/reference/src/optimizer.jl:20-23``) ask for ``S1 + S2``. So S1 moves to a carry
        buffer that is added back after the next reduction, and the next forward (a one-shot
        pre-hook) clears the local gradients so only the new local part is reduced. Until that
        forward ``p.grad`` still shows S1."""
        for b in self.buckets:
            if b.carry is None:
                b.carry = torch.empty_like(b.flat_grad)
            b.carry.copy_(b.flat_grad)
        self._carry_live = True
        if self._carry_hook is None:
            self._carry_hook = self.module.register_forward_pre_hook(lambda m, a: self._start_carry())

    def _start_carry(self):
        """First forward after ``step(zero_grad=False)``: drop the (reduced) gradients."""
        if self._carry_hook is not None:
            self._carry_hook.remove()
            self._carry_hook = None
        if self.grad_mode == "view":
            mt.fill_([b.flat_grad for b in self.buckets], 0.0)
        else:
            for b in self.buckets:
                for p in b.params:
                    p.grad = None

    def _drop_carry(self):
        self._carry_live = False
        if self._carry_hook is not None:
            self._carry_hook.remove()
            self._carry_hook = None

    def _add_carry(self, b: _Bucket):
        if self._carry_live and b.carry is not None:
            b.flat_grad.add_(b.carry)

    def step(self, zero_grad: bool = True):
        """Finish the gradient allreduces and apply the fused optimiser to every bucket.

        The buckets are re-armed here whatever ``zero_grad`` is, so a following
        backward + ``step(zero_grad=False)`` (gradient accumulation across steps)
        launches, packs and waits on every bucket again; the applied gradient of that
        step is the sum over ranks of both backwards' gradients (see ``_arm_carry``).
        """
        if self._ls is not None and not zero_grad:
            raise RuntimeError("DDP.step(zero_grad=False) with loss_scale: the kept gradient and the next backward's "
                               "may carry two different scales and cannot be summed; accumulate inside "
                               "`with ddp.no_sync():` between two steps instead")
        if self._ema_swapped:
            raise RuntimeError("DDP.step inside `with ddp.ema_weights():`: the parameters hold the averaged weights; "
                               "leave the context before training on")
        gscale = 1.0 / self.world if self.average else 1.0
        if not (self.overlap_opt and self._masters_synced):
            self._sync_masters()
        if self._carry_hook is not None:
            self._start_carry()  # no forward since step(zero_grad=False): no new local gradient
        if self.overlap_opt:
            self._step_overlapped()
            self._finish_step(zero_grad)
            return
        if not self.communicate and self.grad_mode == "steal":
            # nothing to reduce: the optimiser reads autograd's gradients where they are
            for b in self.buckets:
                if not self._apply_direct(b, gscale):
                    self._pack(b)
                    self._apply(b, gscale)
            self._finish_step(zero_grad)
            return
        for b in self.buckets:
            if not b.launched:
                b.ready = True
        self._launch_ready()
        if self.timing and self.device.type == "cuda":
            # exposed communication: from the end of backward (all grads produced on the
            # compute stream) until the compute stream may consume the last reduced bucket
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            self._fence_all()
            for b in self.buckets:
                self._pack(b)
                self._finish(b)
            e1.record()
            self._comm_events.append((e0, e1))
            for b in self.buckets:
                self._add_carry(b)
                self._apply(b, gscale)
        else:
            self._fence_all()
            for b in self.buckets:
                self._pack(b)
                self._finish(b)
                self._add_carry(b)
                self._apply(b, gscale)
        self._finish_step(zero_grad)

    def _step_overlapped(self):
        """step() with the per-bucket updates already enqueued during backward: enqueue the
        rest (buckets whose hooks did not complete them: unused parameters, no_sync), then ONE
        compute-stream fence on the optimiser stream (in order: it covers every bucket's
        allreduce and update)."""
        for b in self.buckets:
            if not b.launched:
                b.ready = True
        if self.timing and self.communicate:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
        self._launch_ready()
        if self._opt_stream is not None:
            torch.cuda.current_stream(self.device).wait_stream(self._opt_stream)
        for b in self.buckets:
            if b.work is not None:
                b.work.covered() if hasattr(b.work, "covered") else b.work.wait()
                b.work = None
        if self.timing and self.communicate:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self._comm_events.append((e0, e1))

    def _finish_step(self, zero_grad: bool):
        if self._deferred:
            # gradient norms with the updates in step(): ONE multi-tensor sum of squares over the
            # leaves of all buckets of a dtype (two launches per 24 leaves instead of per bucket)
            # and one fold into the global sum, then every bucket's update. Loss scaling: the
            # non-finite test of every bucket in front of the first update, inside that pass when
            # there is one, else one multi-tensor pass of its own
            grads = {b.index: (gs, gscale) for b, _, gs, gscale in self._deferred}
            for bs, buf, parts in self._clip_groups:
                gs_all = [g for b in bs for g in grads[b.index][0]]
                self._enqueue_norms(gs_all, buf, parts, grads[bs[0].index][1])
            if self._ls is not None and not self._norms:
                fused.check_finite_([g for _, _, gs, _ in self._deferred for g in gs], self._ls_flag)
            for b, st, gs, gscale in self._deferred:
                self._run_update(st, gs, gscale, b)
            self._deferred = []
        if self._has_bt:
            fused.adam_advance_(self.hyper, self._inner.beta[0], self._inner.beta[1],
                                dev_skip=self._ls_flag if self._ls is not None else None)
        if self._sr_seed is not None:
            fused.sr_advance_(self._sr_block, dev_skip=self._ls_flag if self._ls is not None else None)
        if self._ema is not None:  # in front of the scaler update, which clears the flag the EMA kernels read
            e = self._ema
            fused.ema_advance_(self._ema_block, decay=e.decay, warmup=e.warmup, every=e.every,
                               dev_skip=self._ls_flag if self._ls is not None else None)
        if self._ls is not None:
            ls = self._ls
            fused.loss_scale_update_(self._ls_block, growth=ls.growth, backoff=ls.backoff, interval=ls.interval,
                                     min_scale=ls.min_scale, max_scale=ls.max_scale)
        self.step_count += 1
        if self.watchdog is not None:
            self.watchdog.check()
        if self.debug_checks and self.world > 1:
            check_replicas(self.module, comm=runtime.cpu_comm())
        self._rearm()
        self._record_versions()  # the optimiser's own writes are not "outside" changes
        if zero_grad:
            self.zero_grad()
        elif self.communicate:
            self._arm_carry()

    # ------------------------------------------------------------------ masters
    def _record_versions(self):
        self._versions = [[p._version for p in b.params] for b in self.buckets]

    def _sync_masters(self):
        """Pick up parameter changes made outside the engine (``load_state_dict``,
        ``checkpoint.load``, ``synchronize``, in-place edits): a changed version counter
        means the fp32 master of that parameter is stale, so it is re-read from the param."""
        for b, vs in zip(self.buckets, self._versions):
            for i, p in enumerate(b.params):
                if p._version != vs[i]:
                    if b.master is not None:
                        o = b.offsets[i]
                        with torch.no_grad():
                            _strided_view(b.master, p, o).copy_(p.detach())
                    vs[i] = p._version

    def refresh_master(self):
        """Re-read every fp32 master weight from its (low-precision) parameter."""
        with torch.no_grad():
            for b in self.buckets:
                if b.master is not None:
                    b.master.copy_(b.flat_param)
        self._record_versions()

    def exposed_comm_ms(self, reset: bool = True) -> float | None:
        """Mean exposed (not overlapped with backward) allreduce time per step, in ms,
        over the steps run with ``timing=True`` since the last reset; None if none."""
        if not self._comm_events:
            return None
        torch.cuda.synchronize(self.device)
        ms = [a.elapsed_time(b) for a, b in self._comm_events]
        if reset:
            self._comm_events.clear()
        return sum(ms) / len(ms)

    def _slices(self, b: _Bucket) -> tuple:
        """Per-leaf slices (memory order) of the bucket's flat parameters, moments and masters (cached)."""
        st = self._direct_cache.get(b.index)
        if st is None:
            def sl(flat):
                return [flat[o:o + p.numel()] for p, o in zip(b.params, b.offsets)] if flat is not None else None
            st = (sl(b.flat_param), sl(b.exp_avg), sl(b.exp_avg_sq), sl(b.master), sl(b.state3))
            self._direct_cache[b.index] = st
        return st

    def _run_update(self, st: tuple, gs: list, gscale: float, b: _Bucket):
        """One fused update launch over ``st = (params, m, v, masters, third state)`` lists and their
        gradients."""
        ps, ms, vs, ws, s3 = st
        kw = {}
        if isinstance(self._clip_rule, O.ClipGrad):
            kw["clip_delta"] = self._clip_rule.delta
        elif self._per_leaf:
            kw["tscale"] = b.clip[1]
        if self.clip_global_norm is not None:
            kw["dev_gscale"] = self._clip_slot[2:3]  # under a loss scale: inverse scale x clip scale
        elif self._ls is not None:
            kw["dev_gscale"] = self._ls_inv
        if self._ls is not None:
            kw["dev_skip"] = self._ls_flag
        if self._sr_seed is not None and b.dtype == torch.bfloat16:
            # one launch over the flat bucket, or its leaves at their offsets in it: the same bits
            flat = len(ps) == 1 and ps[0] is b.flat_param
            kw["sr"] = fused.SR(self._sr_seed, stream=b.index, dev_block=self._sr_block,
                                offsets=[0] if flat else b.offsets)
        if self._layerwise:
            self._run_layerwise(st, gs, gscale, b, kw)
        elif self.kind == "adam":
            a = self.adam
            fused.adam_(ps, gs, ms, vs, lr=a.eta, beta1=a.beta[0], beta2=a.beta[1], eps=a.epsilon, bc1=0.0,
                        bc2=0.0, weight_decay=self.wd, grad_scale=gscale, masters=ws, dev_hyper=self.hyper, **kw)
        elif self._nstate:
            fused.rule_(self.kind, ps, gs, [ms, vs, s3][:self._nstate], weight_decay=self.wd, grad_scale=gscale,
                        masters=ws, dev_hyper=self.hyper, **self._inner._hyper(), **kw)
        else:
            mom = {"descent": 0.0}.get(self.kind, getattr(self._upd, "rho", 0.0))
            fused.sgd_(ps, gs, ms, lr=self._upd.eta, momentum=mom, nesterov=self.kind == "nesterov",
                       weight_decay=self.wd, grad_scale=gscale, masters=ws, dev_lr=self.hyper, **kw)
        if self._ema is not None:
            # directly behind the bucket's last update launch, on its stream: one launch over the whole
            # flat bucket (padding included), reading the master the update wrote a moment ago
            fused.ema_([b.ema], [b.master if b.master is not None else b.flat_param], dev_block=self._ema_block,
                       dev_skip=kw.get("dev_skip"))

    def _run_layerwise(self, st: tuple, gs: list, gscale: float, b: _Bucket, kw: dict):
        """LARS / LAMB over the bucket's per-leaf lists: the two-phase kernels on the adapted leaves,
        Momentum's / Adam's kernel (no decay, the same device hyper block) on the 1-D ones."""
        ps, ms, vs, ws, _ = st
        r = self._inner
        for idx, adapt in ((b.adapted, True), (b.plain, False)):
            if not idx:
                continue
            pick = lambda l: [l[i] for i in idx] if l is not None else None  # noqa: E731
            p, g, m, v, w = pick(ps), pick(gs), pick(ms), pick(vs), pick(ws)
            if self.kind == "lars":
                if adapt:
                    fused.lars_(p, g, m, lr=r.eta, momentum=r.rho, trust=r.trust, weight_decay=r.decay,
                                eps=r.epsilon, grad_scale=gscale, masters=w, dev_hyper=self.hyper,
                                ratios=b.ratios, workspace=b.lw_work, **kw)
                else:
                    fused.sgd_(p, g, m, lr=r.eta, momentum=r.rho, grad_scale=gscale, masters=w, dev_lr=self.hyper,
                               **kw)
            elif adapt:
                fused.lamb_(p, g, m, v, lr=r.eta, beta1=r.beta[0], beta2=r.beta[1], eps=r.epsilon, bt1=0.0, bt2=0.0,
                            weight_decay=r.decay, grad_scale=gscale, masters=w, dev_hyper=self.hyper,
                            ratios=b.ratios, workspace=b.lw_work, **kw)
            else:
                fused.adam_(p, g, m, v, lr=r.eta, beta1=r.beta[0], beta2=r.beta[1], eps=r.epsilon, bc1=0.0, bc2=0.0,
                            grad_scale=gscale, masters=w, dev_hyper=self.hyper, **kw)

    def _enqueue_norms(self, gs: list, buf: torch.Tensor, parts: torch.Tensor, gscale: float):
        """Per-leaf sums of squares of ``gs`` into ``buf[0]`` (two deterministic launches per 24
        leaves) with the ClipNorm scales into ``buf[1]``, then the fold into the step's global sum
        / norm / global scale (one workgroup; the step's first call starts the sum afresh) — all on
        the current stream, no host read."""
        # loss scaling: the non-finite check rides in the pass, and the norms are the unscaled gradient's
        flag, pre = (self._ls_flag, self._ls_inv) if self._ls is not None else (None, None)
        fused.sumsq_(gs, buf[0], scales=buf[1] if self._per_leaf else None,
                     omega=self._clip_rule.omega if self._per_leaf else 0.0, grad_scale=gscale, partials=parts,
                     flag=flag, dev_pre=pre)
        fused.clip_total_(buf[0], self._clip_slot, accumulate=self._norm_started,
                          omega=self.clip_global_norm or 0.0, grad_scale=gscale, dev_pre=pre)
        self._norm_started = True

    def _update(self, b: _Bucket, st: tuple, gs: list, gscale: float):
        """The bucket's update on the current stream. With norm clipping and ``overlap_opt`` the
        bucket's norms are enqueued right in front of it (a leaf never spans buckets); otherwise
        the update waits for ``_finish_step``, which takes the norms of all buckets at once —
        ``clip_global_norm`` needs the last bucket's norm before the first update anyway."""
        if self._norms or self._ls is not None:  # (a loss scale switches overlap_opt off)
            if not self.overlap_opt:
                self._deferred.append((b, st, gs, gscale))
                return
            self._enqueue_norms(gs, b.clip, b.partials, gscale)
        self._run_update(st, gs, gscale, b)

    def _apply(self, b: _Bucket, gscale: float):
        if self._norms or self._layerwise:
            # per-leaf norms: the update reads the flat bucket leaf by leaf (as _apply_direct does)
            self._update(b, self._slices(b), [v.as_strided((v.numel(),), (1,)) for _, v, _ in self._grad_views(b)],
                         gscale)
            return
        one = lambda t: [t] if t is not None else None  # noqa: E731
        self._update(b, ([b.flat_param], one(b.exp_avg), one(b.exp_avg_sq), one(b.master), one(b.state3)),
                     [b.flat_grad], gscale)

    def _apply_direct(self, b: _Bucket, gscale: float) -> bool:
        """Fused optimiser on the autograd gradients in place (no pack). False if some gradient
        cannot be read directly (missing, other dtype/layout/device): the caller packs instead."""
        grads = []
        for p in b.params:
            g = p.grad
            if g is None:
                return False
            if not (g.dtype is b.dtype and g.stride() == p.stride() and g.device == b.device):
                if g.dtype != b.dtype or g.device != b.device or not _same_layout(g, p) or not _is_dense(g):
                    return False
            grads.append(g)
        # the flat slices are in memory order; a gradient with its parameter's strides is too
        gs = [g.view(-1) if g.is_contiguous() else g.as_strided((g.numel(),), (1,)) for g in grads]
        self._update(b, self._slices(b), gs, gscale)
        return True

    def grad_norm(self) -> torch.Tensor:
        """The last step's global L2 norm of the gradient the rule saw — after reduction, carry and
        the ``average`` scale, before clipping — as a 0-dim fp32 tensor on the engine's device.
        Never synchronises (read it after ``step()``, on the stream ``step()`` ran on). Available
        with a ``ClipNorm`` chain or ``clip_global_norm``."""
        if not self._norms:
            raise RuntimeError("DDP.grad_norm: the engine computes gradient norms only when it clips by one: "
                               "use an OptimiserChain(ClipNorm(omega), rule) or clip_global_norm=...")
        return self._clip_slot[1]

    def scale_loss(self, loss: torch.Tensor) -> torch.Tensor:
        """``loss * scale`` with the scaler's device scalar (no host read: usable inside a
        ``GraphedStep`` ``loss_fn``); call ``backward()`` on the result. A 16-bit loss is taken to
        fp32 first (2^16 is beyond fp16). Without ``loss_scale`` the loss comes back as it is."""
        if self._ls is None:
            return loss
        if loss.dtype in (torch.float16, torch.bfloat16):
            loss = loss.float()
        return loss * self._ls_scale

    def _scaler(self, what: str) -> torch.Tensor:
        if self._ls is None:
            raise RuntimeError(f"DDP.{what}: the engine was built without loss_scale")
        return self._ls_block

    def loss_scale(self) -> torch.Tensor:
        """The current loss scale (the one the next backward is to be scaled by): a 0-dim fp32 view
        of the scaler's device block. Never synchronises (read it after ``step()``, on the stream
        ``step()`` ran on), like :meth:`skipped_steps` and :meth:`step_skipped`."""
        return self._scaler("loss_scale").view(torch.float32)[fused.LS_SCALE]

    def skipped_steps(self) -> torch.Tensor:
        """Steps skipped so far for a non-finite gradient (0-dim int32 device view). ``step_count``
        counts them too: the host never learns which steps were skipped."""
        return self._scaler("skipped_steps")[fused.LS_SKIPPED]

    def step_skipped(self) -> torch.Tensor:
        """1 if the last ``step()`` was skipped, else 0 (0-dim int32 device view)."""
        return self._scaler("step_skipped")[fused.LS_LAST]

    def sr_step(self) -> torch.Tensor:
        """The stochastic-rounding generator's step counter — applied steps so far; a step the loss
        scaler skipped does not count — as a 0-dim int32 device view (the uint32's bits). Never
        synchronises (read it after ``step()``, on the stream ``step()`` ran on)."""
        if self._sr_seed is None:
            raise RuntimeError("DDP.sr_step: the engine was built without stochastic_rounding")
        return self._sr_block[0]

    def trust_ratios(self) -> dict:
        """``{name: ratio}`` of the last step's trust ratios under LARS / LAMB: 0-dim device tensors
        (fp32; fp64 for fp64 parameters), views of the engine's tables, so they follow later steps.
        The 1-D leaves, which are not adapted, are absent. Never synchronises (read it after
        ``step()``, on the stream ``step()`` ran on)."""
        if not self._layerwise:
            raise RuntimeError("DDP.trust_ratios: only the layer-wise rules (LARS, LAMB) have trust ratios")
        return {b.names[i]: b.ratios[k] for b in self.buckets for k, i in enumerate(b.adapted)}

    # ------------------------------------------------------------------ weight EMA
    def _ema_restart(self, b: _Bucket):
        """Bucket ``b``'s average := its master (else its parameters), in place, leaf by leaf (the
        padding between leaves keeps its zeros)."""
        src = b.master if b.master is not None else b.flat_param
        with torch.no_grad():
            for p, o in zip(b.params, b.offsets):
                b.ema[o:o + p.numel()].copy_(src[o:o + p.numel()])

    def _averaging(self, what: str) -> EMA:
        if self._ema is None:
            raise RuntimeError(f"DDP.{what}: the engine was built without ema")
        return self._ema

    def ema_parameters(self) -> dict:
        """``{name: averaged weight}``: views of the engine's flat EMA buffers (fp32; fp64 for fp64
        parameters) with the parameter's shape and strides, so they follow later steps. Never
        synchronises (read them after ``step()``, on the stream ``step()`` ran on), like
        :meth:`ema_decay` and :meth:`ema_updates`.

        The average follows the fp32 masters (the parameters where there are none) as the optimiser
        writes them. A parameter change from outside the engine (``load_state_dict`` on the module,
        an in-place edit: what ``step()`` copies into the masters) does NOT reset it: the average
        moves towards the new weights at the rate ``1 - d_t`` like after any other step."""
        self._averaging("ema_parameters")
        return {n: _strided_view(b.ema, p, o) for b in self.buckets for n, p, o in zip(b.names, b.params, b.offsets)}

    def ema_decay(self) -> torch.Tensor:
        """The decay ``d_t`` the coming EMA update uses (0-dim fp32 device view)."""
        self._averaging("ema_decay")
        return self._ema_block.view(torch.float32)[fused.EMA_DECAY]

    def ema_updates(self) -> torch.Tensor:
        """EMA updates done so far (0-dim int32 device view): applied steps, every ``every``-th one."""
        self._averaging("ema_updates")
        return self._ema_block[fused.EMA_UPDATES]

    def ema_state_dict(self) -> dict:
        """``module.state_dict()`` (its keys and dtypes, copies) with every parameter the engine
        trains replaced by its average, cast to the parameter's dtype. Everything else — buffers,
        frozen parameters, BatchNorm's running statistics, which are averages already and are not
        averaged again — is the live tensor's copy."""
        avg = self.ema_parameters()
        sd = self.module.state_dict()
        out = type(sd)()
        for k, v in sd.items():
            out[k] = avg[k].to(v.dtype, copy=True) if k in avg else v.detach().clone()
        if hasattr(sd, "_metadata"):
            out._metadata = sd._metadata
        return out

    @contextmanager
    def ema_weights(self):
        """Evaluation with the averaged weights: inside, the module's parameters hold the EMA cast to
        their dtype; on exit the training parameters are back bit for bit. The masters, the moments
        and the average itself are never touched, and the swap does not count as an outside edit of
        the parameters. ``step()`` inside raises. Plain copies, not a hot path."""
        self._averaging("ema_weights")
        if self._ema_swapped:
            raise RuntimeError("DDP.ema_weights: already inside the context")
        self._sync_masters()  # an outside edit made before the swap reaches the masters first
        with torch.no_grad():
            saved = [b.flat_param.clone() for b in self.buckets]
            for b in self.buckets:
                b.flat_param.copy_(b.ema)
        self._ema_swapped = True
        try:
            yield self.module
        finally:
            with torch.no_grad():
                for b, s in zip(self.buckets, saved):
                    b.flat_param.copy_(s)
            self._ema_swapped = False
            self._record_versions()

    def set_lr(self, lr: float):
        """Change the learning rate (device-side, so captured graphs see it)."""
        if not hasattr(self._inner, "eta"):
            raise ValueError(f"DDP.set_lr: {type(self._inner).__name__} has no learning rate")
        self.hyper[0].fill_(lr)
        self._inner.eta = lr

    # ------------------------------------------------------------------ state
    def optimiser_state(self):
        """Optimisers.jl-layout state tree ``{name: Leaf(rule, state)}`` (views, no copies)."""
        out = {}
        if self._has_bt:
            bt = self.hyper[1:].tolist()
        for b in self.buckets:
            for name, p, o in zip(b.names, b.params, b.offsets):
                n = p.numel()
                # moments follow the parameter's memory order (NHWC for channels_last weights)
                if self._has_bt:  # Adam, AdaMax, NAdam, AdaBelief: (m, v, βt)
                    st = (_strided_view(b.exp_avg, p, o), _strided_view(b.exp_avg_sq, p, o), tuple(bt))
                elif self._nstate > 1:  # AdaDelta (acc, Δ), AMSGrad (m, v, v̂)
                    st = tuple(_strided_view(t, p, o) for t in (b.exp_avg, b.exp_avg_sq, b.state3)[:self._nstate])
                elif b.exp_avg is not None:
                    st = _strided_view(b.exp_avg, p, o)
                else:
                    st = None
                if self._clip_rule is not None:
                    # the chain's tuple of member states: (clip: None, update rule's state...)
                    if isinstance(self._upd, O.OptimiserChain):  # rule + WeightDecay behind the clip
                        st = (None, (st, None)) if self._chain_where == 1 else (None, st, None)
                    else:
                        st = (None, st)
                elif isinstance(self._upd, O.OptimiserChain) and self.kind != "adam":
                    st = (st, None)  # (rule, WeightDecay); an unclipped AdamW keeps its bare Adam state
                out[name] = O.Leaf(self.rule, st)
        return out

    def state_dict(self):
        sd = {
            "module": self.module.state_dict(),
            "step": self.step_count,
            "hyper": self.hyper.detach().cpu(),
            "buckets": [{"master": b.master.detach().cpu() if b.master is not None else None,
                         "m": b.exp_avg.detach().cpu() if b.exp_avg is not None else None,
                         "v": b.exp_avg_sq.detach().cpu() if b.exp_avg_sq is not None else None}
                        for b in self.buckets],
        }
        for b, s in zip(self.buckets, sd["buckets"]):
            if b.state3 is not None:  # only the rules with a third state buffer (AMSGrad) add the key
                s["s3"] = b.state3.detach().cpu()
        if self._ls is not None:
            blk = self._ls_block.detach().cpu()
            sd["loss_scale"] = {"scale": float(blk.view(torch.float32)[fused.LS_SCALE]),
                                "growth_tracker": int(blk[fused.LS_TRACKER]), "skipped": int(blk[fused.LS_SKIPPED])}
        if self._sr_seed is not None:
            sd["sr"] = {"seed": self._sr_seed, "step": int(self._sr_block[0]) & 0xFFFFFFFF}
        if self._ema is not None:
            blk = self._ema_block.detach().cpu()
            sd["ema"] = {"buckets": [b.ema.detach().to("cpu", copy=True) for b in self.buckets],
                         "num_updates": int(blk[fused.EMA_UPDATES]), "since": int(blk[fused.EMA_SINCE])}
        return sd

    def load_state_dict(self, sd):
        with torch.no_grad():
            self.module.load_state_dict(sd["module"])
            self.step_count = int(sd["step"])
            self.hyper.copy_(sd["hyper"])
            for b, s in zip(self.buckets, sd["buckets"]):
                if b.master is not None:
                    if s["master"] is not None:
                        b.master.copy_(s["master"])
                    else:  # checkpoint without masters: start them from the loaded params
                        b.master.copy_(b.flat_param)
                if s["m"] is not None:
                    b.exp_avg.copy_(s["m"])
                if s["v"] is not None:
                    b.exp_avg_sq.copy_(s["v"])
                if b.state3 is not None:
                    b.state3.copy_(s["s3"])
            if self._ls is not None:
                # in place: captured graphs and the accessors' views keep pointing at the block; a
                # checkpoint without a scaler state starts from the constructor's values
                ls = sd.get("loss_scale") or {"scale": self._ls.init, "growth_tracker": 0, "skipped": 0}
                self._ls_block.copy_(fused.loss_scale_block(ls["scale"], "cpu", tracker=ls["growth_tracker"],
                                                            skipped=ls["skipped"]))
            if self._sr_seed is not None:
                # in place too; the seed is the constructor's (every rank's); without the key: step 0
                self._sr_block.copy_(fused.sr_block("cpu", step=int((sd.get("sr") or {}).get("step", 0))))
            if self._ema is not None:
                # in place as well; a checkpoint without an average starts one from the loaded masters
                # (parameters where there are none), with no update counted
                saved = sd.get("ema")
                for i, b in enumerate(self.buckets):
                    if saved is not None:
                        b.ema.copy_(saved["buckets"][i])
                    else:
                        self._ema_restart(b)
                e = self._ema
                self._ema_block.copy_(fused.ema_block(e.decay, e.warmup, e.every, "cpu",
                                                      updates=saved["num_updates"] if saved else 0,
                                                      since=saved["since"] if saved else 0))
        self._record_versions()

    def num_parameters(self) -> int:
        return sum(p.numel() for b in self.buckets for p in b.params)

    def comm_summary(self) -> dict:
        """What the engine communicates per step (for bench records)."""
        return {"communicate": self.communicate, "force_comm": self.force_comm,
                "overlap": bool(self.overlap and self.communicate), "grad_mode": self.grad_mode,
                "buckets": len(self.buckets),
                "bucket_mb": [round(b.numel * b.flat_grad.element_size() / 2 ** 20, 2) for b in self.buckets],
                "comm": (self.comm.name if self.communicate else "none"),
                "direct_grads": self.direct_grads, "overlap_opt": self.overlap_opt,
                "bucket_plan": self.bucket_plan,
                "comm_probe": self.comm_probe,
                # gradients the packs copied per step so far (0: every one delivered in place)
                "pack_copies_per_step": round(self.pack_copies / max(1, self.step_count), 2),
                # the parameter shapes the packs copied (total over the steps so far), most first
                "pack_copied_shapes": dict(sorted(self.pack_copied.items(), key=lambda kv: -kv[1])[:8])}

    def bucket_summary(self) -> list:
        return [{"index": b.index, "dtype": str(b.dtype), "numel": b.numel, "params": len(b.params),
                 "mbytes": b.numel * b.flat_grad.element_size() / 2 ** 20} for b in self.buckets]

    def remove_hooks(self):
        for h in self._hooks:
            h.remove()
        self._hooks.clear()


__all__ = ["DDP", "LossScale", "EMA"]
