"""Inputs, staged float64 references, a call recorder, the stage-wise checker, a float32 emulation and
planted defects for one training-mode ResNet bottleneck (``models/resnet.Bottleneck`` on
``ops/fused_block``), shared by ``test_block_edges_gpu.py`` (plain helper module: no fixtures, no tests,
nothing imported from the extension at import time).

The block is checked stage by stage, never end to end: every stage's reference starts from the bf16
values the device STORED for the tensors entering that stage (the recorder keeps them), so no bound
compounds across stages (the method of test_conv3ds_bn_bwd_gpu.py).

    c1 = x . W1, a1 = relu(bn1(c1)), c2 = conv3x3_s(a1, W2), a2 = relu(bn2(c2)), c3 = a2 . W3,
    side = x | bn_ds(x_s . W_ds), out = relu(bn3(c3) + side)           and the adjoint of each stage.

Bounds (nothing fitted to kernel output):

* a GEMM / implicit-GEMM stage of our kernels (forward, input gradient, filter gradient):
  ``mfma_edges.bound(R, A, K, "bf16")`` per element, K the reduction length (channels, 9 x channels,
  output pixels); R, A from float64 convolutions of the stored operands and of their absolute values.
  Stages that MIOpen ran on the route are not held to it (their results are the next stage's inputs).
* a BatchNorm stage: ``norm_edges.bn_check_fwd`` / ``bn_check_bwd`` (statistics, running statistics,
  the counter, y, the stored mask, dx, dgamma, dbeta); a ReLU whose sign the bound cannot decide may
  go either way (``undecided`` / ``check_either``), at most 1e-3 of a tensor.
* nodes that never store an intermediate compose two references and, to first order, two bounds:
  - one-pass backward (``conv3_bn3_relu``, ``conv3ds_bn_relu``): bn3's dx (reference dx, bound ddx of
    ``bn_bwd_ref``, its bf16 rounding included: the kernel rounds the MFMA operand) feeds
    d_a2 = dx . W and dW = dx^T . a2: bound(R, (|dx| + ddx) |W|, K, "bf16") + ddx |W| (likewise with |a2|).
  - ``bn_relu_conv1x1``: a2 (reference and bound dy of ``affine_fwd_ref``, bf16 rounding included)
    feeds c3 = a2 . W3 and dW3 = dc3^T . a2 the same way; backward, da = dc3 . W3 (bound b_da, a bf16
    GEMM result) enters bn2's backward, which is linear in it: sums + sum b_da (x |xhat|), dx +
    |A| (b_da + mean b_da) + |A invstd (x - mean)| mean(b_da |xhat|) on top of ``bn_bwd_ref``.
  - ``dual_bn_relu``: z = z3 + z_ds with dz = dz3 + dz_ds + 2u |z| (one more fp32 addition).
* the block input's gradient arrives as one tensor: dc1 . W1 + side, side = mask . dy exactly (identity
  block, through the GradLink or from autograd) or the downsample's input gradient (a bf16 GEMM result
  with bound b2): bound(R1, A1, K1, "res", side) + (1 + u8) b2 + u8 bound(R1, A1, K1, "bf16"), which
  covers the addition in the dgrad epilogue and autograd's addition of two bf16 tensors.
* a ``c3=`` hand-over (``bn_relu_conv3``) must reach its consumer bit for bit.

Exact case (``exact_conv3``): on a route that stores a2 (identity block, ``CONV3BN3=0``: ``bn_from_stats``
then ``conv1x1_hybrid``) the test substitutes, at the recorder boundary, ternary a2 and W3 for conv3's
arguments and a ternary gradient for the one arriving at c3 (``mfma_edges.linbwd_inputs("ternary")``: sums
of arbitrary bf16 gradients would not be exact), so c3, d_a2 and dW3 are small integers and must EQUAL the
float64 results of the stored operands.
"""
import contextlib
import inspect
import io
import re

import torch
import torch.nn.functional as F

from . import mfma_edges as E
from . import norm_edges as N
from .mfma_edges import TINY, U8

BF = torch.bfloat16
U32 = N.U32
EPS, MOM = 1e-5, 0.1
# (cin, width, stride, downsample) of ResNet-50's eight block kinds
KINDS = ((64, 64, 1, True), (256, 64, 1, False), (256, 128, 2, True), (512, 128, 1, False),
         (512, 256, 2, True), (1024, 256, 1, False), (1024, 512, 2, True), (2048, 512, 1, False))
ENTRIES = ("conv1x1_stats", "conv1x1_hybrid", "conv1x1_downsample", "bn_from_stats", "bn_relu_conv3",
           "bn_relu_conv1x1", "dual_bn_relu", "conv3x3", "conv3x3_s2", "conv3_bn3_relu", "conv3ds_bn_relu")
DEFECTS = ("res_missing_last_tile", "res_twice", "stats_swapped", "sums_swapped_bwd", "mask_shifted",
           "dbeta_32_63_zero", "biased_running_var", "c3_recomputed", "wgrad_slab_omitted")


def kind_id(kind):
    return f"{kind[0]}-{kind[1]}-s{kind[2]}-{'ds' if kind[3] else 'id'}"


def route(**kw):
    """One arm of ``Bottleneck.forward``'s route tree. impl: conv_impl; ours1 / ours3 / ours3s2 / ds_ours: the
    ``*_forward_is_ours`` answers; ds_fwd: ``DS_FWD``; bn2conv3 / conv3bn3 / conv3ds / dual: the switches;
    o3: ``conv1x1_forward_is_ours`` for conv3's shape where it differs from conv1's (None: as ours1);
    masked: ``masked_links_ok``; needs: the block input requires a gradient; wgrad: ``conv_choice.WGRAD``;
    big: the 3 x 74 x 74 batch (stride 2: 3 x 148 x 148, 74 x 74 after conv2), 16428 pixels where
    ``bn2conv3_ok`` looks: the smallest our shapes offer above its 64-pixels-per-compute-unit gate (16384 on
    256 compute units) that is no multiple of 32."""
    r = dict(impl="hybrid", ours1=True, o3=None, ours3=True, ours3s2=True, ds_ours=True, ds_fwd="ours", bn2conv3=False,
             conv3bn3=2, conv3ds=1, dual=True, masked=True, needs=True, wgrad="ours", big=False)
    assert set(kw) <= set(r), kw
    r.update(kw)
    return r


def route_id(r):
    d = route()
    return ",".join(f"{k}={v}" for k, v in r.items() if d[k] != v) or "default"


def o3_of(r):
    return r["ours1"] if r["o3"] is None else r["o3"]


def ds_stats(kind, r):
    return bool(kind[3] and r["dual"] and {"ours": r["ds_ours"], "force": True, "miopen": False}[r["ds_fwd"]])


def plan(kind, r):
    """[(entry, stage)]: the public entry points ``Bottleneck.forward`` calls on this arm, in order."""
    cin, width, stride, ds = kind
    hy = r["impl"] == "hybrid"
    p = [("conv1x1_hybrid" if hy else "conv1x1_stats", "conv1"),
         ("bn_from_stats" if (not hy or r["ours1"]) else "FusedBatchNorm2d", "bn1")]
    dual = ds and r["dual"]
    c3ds = hy and dual and r["conv3ds"] in (1, 2) and kind[:3] == (64, 64, 1)
    if ds and not c3ds:
        p.append(("conv1x1_downsample", "ds"))
        if not dual:
            p.append(("FusedBatchNorm2d", "bn_ds"))
    if not hy:
        p += [("conv3x3" if stride == 1 else "nn.Conv2d", "conv2"), ("bn_relu_conv1x1", "bn2+conv3"),
              ("dual_bn_relu", "bn3+bn_ds") if dual else ("bn_from_stats", "bn3")]
        return p
    p.append(("conv3x3" if stride == 1 else "conv3x3_s2", "conv2"))
    b2c3 = r["bn2conv3"] and r["big"] and width in (64, 128) and o3_of(r)
    p.append(("bn_relu_conv3", "bn2+conv3fwd") if b2c3 else ("bn_from_stats", "bn2"))
    o3 = b2c3 or o3_of(r)
    if not ds and ((width == 64 and r["conv3bn3"] >= 1) or (width == 128 and r["conv3bn3"] >= 2)) \
            and (r["masked"] or not r["needs"]):
        return p + [("conv3_bn3_relu", "conv3+bn3")]
    if c3ds:
        return p + [("conv3ds_bn_relu", "conv3+ds+bn3")]
    p.append(("conv1x1_hybrid", "conv3"))
    p.append(("dual_bn_relu", "bn3+bn_ds") if dual else ("bn_from_stats" if o3 else "FusedBatchNorm2d", "bn3"))
    return p


def rows(t):
    """[N, C, H, W] -> [N H W, C] (what the NHWC kernels see); other ranks as they are."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) if t.dim() == 4 else t


def unrows(t2, n, h, w):
    return t2.view(n, h, w, -1).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------- inputs

def make_inputs(kind, family, big=False, seed=0):
    """x and the filters from ``mfma_edges``' family (uniform / cancel), BatchNorm weights of both signs in
    +-[0.5, 1.5), biases |b| in [2^-4, 1) of both signs (about half of each ReLU active: the normalised
    values are centred), an upstream gradient in (-1, 1) with exact zeros. Batch 3 at 10 x 10 (stride 1:
    300 pixels, nine 32-pixel tiles and 12) or 12 x 12 (stride 2: 432 -> 108 pixels); ``big``: 74 x 74
    (stride 2: 148 x 148 -> 74 x 74)."""
    cin, width, stride, ds = kind
    cout = 4 * width
    n = 3
    h = 74 * stride if big else (10 if stride == 1 else 12)
    ho = h // stride
    x2, w1 = E.gemm_inputs(family, n * h * h, width, cin, seed)
    _, w2 = E.conv_inputs(family, 1, width, 4, 4, width, seed)
    _, w3 = E.gemm_inputs(family, 8, cout, width, seed + 1)
    _, wds = E.gemm_inputs(family, 8, cout, cin, seed + 2)
    g = E._gen("block", family, cin, width, stride, int(big), seed)
    inp = dict(x=unrows(x2, n, h, h), w1=w1.view(width, cin, 1, 1), w2=w2, w3=w3.view(cout, width, 1, 1),
               wds=wds.view(cout, cin, 1, 1) if ds else None)
    for name, c in (("bn1", width), ("bn2", width), ("bn3", cout), ("bn_ds", cout)):
        w, b = N.affine(g, c)
        inp[name] = dict(w=w, b=b)
    dy = (torch.rand(n * ho * ho * cout, generator=g) * 2 - 1)
    dy[::97] = 0
    inp["dy"] = unrows(dy.view(n * ho * ho, cout).bfloat16(), n, ho, ho)
    return inp


# ------------------------------------------------------------------------------- the recorder

SAVED = {"_BNFromStats": ("x", "mask", "w32", "b32", "mean", "inv"), "_FusedBN": ("x", "mask", "w32", "b32", "mean", "inv"),
         "_BN2Conv3": ("c2", "w32", "b32", "mean", "inv"),
         "_Conv3BN3": ("a2", "weight", "c3", "mask", "w32", "b32", "mean", "inv"),
         "_DualBN": ("c3", "cds", "mask", "w32", "mean", "inv", "w232", "mean2", "inv2"),
         "_Conv3DsBN": ("a2", "w3", "x", "wds", "c3", "cds", "mask", "w32", "mean", "inv", "w232", "mean2", "inv2"),
         "_BNReluConv1x1": ("c2", "w32", "b32", "mean", "inv", "scale", "shift", "weight")}
KEEP = ("mask", "mean", "inv", "mean2", "inv2", "c3", "cds")


def _cpu(t):
    return t.detach().to("cpu", copy=True)


class Recorder:
    """Context manager: wraps the public entry points ``Bottleneck.forward`` calls (``ENTRIES`` of
    ``ops.fused_block``, ``FusedBatchNorm2d.forward`` and ``nn.Conv2d.forward``) and keeps, per call,
    ``dict(name, t, meta)``: t holds CPU copies of the tensor arguments under their parameter names (a
    BatchNorm module ``p`` as p.w, p.b, p.rm0 / p.rv0 / p.nbt0 before and p.rm / p.rv / p.nbt after the
    call; a convolution module as p.w), the results (y, or y0, y1), what the autograd node saved of
    ``KEEP`` (s.mean, s.mask, ...), the gradient arriving at every differentiable tensor argument and
    result (d.<name>, through ``Tensor.register_hook``) and, after :meth:`finish`, the parameters' gradients
    (g.<name>). ``links`` are the GradLink / SideGradLink objects seen."""

    def __init__(self):
        self.record, self.links, self._undo, self._params = [], [], [], []

    def __enter__(self):
        from fluxmpi_amd.ops import fused_block as fb
        from fluxmpi_amd.ops.batchnorm import FusedBatchNorm2d
        for name in ENTRIES:
            self._patch(fb, name, name)
        self._patch(FusedBatchNorm2d, "forward", "FusedBatchNorm2d")
        self._patch(torch.nn.Conv2d, "forward", "nn.Conv2d")
        return self

    def __exit__(self, *exc):
        for owner, attr, orig in reversed(self._undo):
            setattr(owner, attr, orig)
        self._undo = []

    def _patch(self, owner, attr, name):
        orig = getattr(owner, attr)
        sig = inspect.signature(orig)

        def wrapper(*a, **k):
            ba = sig.bind(*a, **k)
            ba.apply_defaults()
            e = dict(name=name, t={}, meta={})
            t, mods = e["t"], []
            for p, v in ba.arguments.items():
                p = {"self": "bn" if name == "FusedBatchNorm2d" else "conv", "input": "x"}.get(p, p)
                if isinstance(v, torch.nn.Parameter):
                    t[p] = _cpu(v)
                    self._params.append((t, "g." + p, v))
                elif isinstance(v, torch.Tensor):
                    t[p] = _cpu(v)
                    if v.requires_grad:
                        v.register_hook(lambda g, key="d." + p: t.__setitem__(key, _cpu(g)))
                elif isinstance(v, torch.nn.modules.batchnorm._BatchNorm):
                    t[p + ".w"], t[p + ".b"] = _cpu(v.weight), _cpu(v.bias)
                    t[p + ".rm0"], t[p + ".rv0"], t[p + ".nbt0"] = _cpu(v.running_mean), _cpu(v.running_var), _cpu(v.num_batches_tracked)
                    self._params += [(t, f"g.{p}.w", v.weight), (t, f"g.{p}.b", v.bias)]
                    mods.append((p, v))
                elif isinstance(v, torch.nn.Conv2d):
                    t[p + ".w"] = _cpu(v.weight)
                    self._params.append((t, f"g.{p}.w", v.weight))
                elif v is None or isinstance(v, (bool, int, float, str)):
                    e["meta"][p] = v
                else:  # a link
                    e["meta"][p] = type(v).__name__
                    self.links.append(v)
            out = orig(*a, **k)
            for p, v in mods:
                t[p + ".rm"], t[p + ".rv"], t[p + ".nbt"] = _cpu(v.running_mean), _cpu(v.running_var), _cpu(v.num_batches_tracked)
            outs = {"y": out} if isinstance(out, torch.Tensor) else {f"y{i}": o for i, o in enumerate(out)}
            node = None
            for key, o in outs.items():
                t[key] = _cpu(o)
                if o.requires_grad:
                    node = node or o.grad_fn
                    o.register_hook(lambda g, key="d." + key: t.__setitem__(key, _cpu(g)))
            names = SAVED.get(type(node).__name__.replace("Backward", "")) if node is not None else None
            if names:
                assert len(names) == len(node.saved_tensors), \
                    f"{type(node).__name__} saves {len(node.saved_tensors)} tensors, SAVED lists {len(names)}: update SAVED"
                for key, s in zip(names, node.saved_tensors):
                    if key in KEEP and s is not None:
                        t["s." + key] = _cpu(s)
            self.record.append(e)
            return out

        setattr(owner, attr, wrapper)
        self._undo.append((owner, attr, orig))

    def finish(self):
        """After the backward: the parameters' gradients into the record."""
        for t, key, p in self._params:
            if p.grad is not None:
                t[key] = _cpu(p.grad)
        return self.record


# ------------------------------------------------------------------------------- references

def conv_ref(op, x, w, dy, stride):
    """(R, A, K) in float64 of a convolution's forward / input gradient ("dgrad") / filter gradient
    ("wgrad") from the given operands (any float dtype) and of their absolute values; pad = k // 2."""
    k = w.shape[-1]
    pad = k // 2
    if op == "fwd":
        f = lambda a, b: F.conv2d(a, b, None, stride, pad)
        a, b, K = x.double(), w.double(), w[0].numel()
    elif op == "dgrad":
        f = lambda a, b: torch.nn.grad.conv2d_input(tuple(x.shape), b, a, stride, pad)
        a, b, K = dy.double(), w.double(), w.shape[0] * k * k
    else:
        f = lambda a, b: torch.nn.grad.conv2d_weight(a, tuple(w.shape), b, stride, pad)
        a, b, K = x.double(), dy.double(), dy.numel() // dy.shape[1]
    return f(a, b), f(a.abs(), b.abs()), K


class Walk:
    """The checker: walks a record (the recorder's or the emulation's) along ``plan(kind, route)``.
    ``errs``: every failure, each beginning with its stage; ``ratios``: the worst |err| / bound per stage;
    ``und``: the undecided share per ReLU."""

    def __init__(self, kind, r):
        self.kind, self.r, self.errs, self.ratios, self.und = kind, r, [], {}, {}
        self.bounded = set()  # stages that ran at least one bounded check: each must show in ``ratios``
        self.side = None  # (reference, bound) of a downsample input gradient that is never stored

    def run(self, record):
        names = [e["name"] for e in record]
        want = plan(self.kind, self.r)
        if names != [n for n, _ in want]:
            self.errs.append(f"route: the entries seen {names} are not {[n for n, _ in want]}")
            return self
        buf = io.StringIO()  # every bounded check prints "<stage> <what>: worst |err| / bound <ratio>"
        with contextlib.redirect_stdout(buf):
            for e, (_, st) in zip(record, want):
                if "Conv" not in e["name"] and not e["name"].startswith(("conv1x1_", "conv3x3")):
                    self.bounded.add(st)  # (the plain convolutions add themselves where a stage of ours ran)
                getattr(self, "_" + e["name"].replace(".", "_"))(st, e)
            self._block_input(record, want)
        print(buf.getvalue(), end="")
        for st, ratio in re.findall(r"^(\S+) [^\n]*: worst \|err\| / bound (\S+)$", buf.getvalue(), re.M):
            self.ratios[st] = max(self.ratios.get(st, 0.0), float(ratio))
        lost = sorted(self.bounded - set(self.ratios))
        if lost:  # the table is parsed from what ``mfma_edges.check`` prints: a changed format must not empty it
            self.errs.append(f"ratios: no 'worst |err| / bound' line was parsed for {lost}")
        for st, ratio in self.ratios.items():
            print(f"RATIO {kind_id(self.kind)} [{route_id(self.r)}] {st}: {ratio:.3f}")
        return self

    # ---- convolutions
    def _conv(self, st, e, fwd, dgrad, wgrad, stride=1, wkey="weight", x="x", y="y", dy="d.y", dx="d.x"):
        t = e["t"]
        xs, w = t[x], t[wkey]
        if fwd or wgrad or (dgrad and dx in t):
            self.bounded.add(st)
        if fwd:
            R, A, K = conv_ref("fwd", xs, w, None, stride)
            E.check(f"{st} forward", t[y], R, E.bound(R, A, K, "bf16"), self.errs)
        if dgrad and dx not in t:
            self.errs.append(f"{st} input-gradient: no gradient arrived at the stage's input")
        elif dgrad:
            R, A, K = conv_ref("dgrad", xs, w, t[dy], stride)
            E.check(f"{st} input-gradient", t[dx], R, E.bound(R, A, K, "bf16"), self.errs)
        if wgrad:
            R, A, K = conv_ref("wgrad", xs, w, t[dy], stride)
            E.check(f"{st} filter-gradient", t["g." + wkey], R, E.bound(R, A, K, "bf16"), self.errs)

    def _conv1x1_stats(self, st, e):
        self._conv(st, e, True, False, True)  # (the input gradient is the block input's: _block_input)

    def _conv1x1_hybrid(self, st, e):
        given = e["t"].get("c") is not None
        if given and not torch.equal(e["t"]["c"].view(torch.int16), e["t"]["y"].view(torch.int16)):
            self.errs.append(f"{st} c= hand-over: the result is not the c3 handed over, bit for bit")
        ours = self.r["ours1"] if st == "conv1" else o3_of(self.r)
        self._conv(st, e, ours and not given, st != "conv1", self.r["wgrad"] == "ours")

    def _conv1x1_downsample(self, st, e):
        self._conv(st, e, ds_stats(self.kind, self.r), False, self.r["wgrad"] == "ours", self.kind[2])

    def _conv3x3(self, st, e):
        self._conv(st, e, self.r["ours3"], True, self.r["wgrad"] == "ours")

    def _conv3x3_s2(self, st, e):  # (its input gradient runs on MIOpen unless FLUXMPI_S2_DGRAD=1)
        self._conv(st, e, self.r["ours3s2"], False, self.r["wgrad"] == "ours", 2)

    def _nn_Conv2d(self, st, e):
        pass  # MIOpen: its stored results are the next stages' inputs

    # ---- BatchNorm
    def _counter(self, st, t, pre):
        if int(t[pre + ".nbt"]) != int(t[pre + ".nbt0"]) + 1:
            self.errs.append(f"{st} {pre}.num_batches_tracked: {int(t[pre + '.nbt'])} after {int(t[pre + '.nbt0'])}")

    def _bn(self, st, e, x="x", y="y", dy="d.y", dx="d.x", pre="bn", relu=None, dres=False):
        t = e["t"]
        relu = e["meta"].get("relu", False) if relu is None else relu
        res = t.get("residual")
        inp = dict(x=rows(t[x]), w=t[pre + ".w"], b=t[pre + ".b"], res=rows(res) if res is not None else None,
                   dy=rows(t[dy]))
        out = dict(mean=t["s.mean"], inv=t["s.inv"], y=rows(t[y]), mask=t.get("s.mask"), rm=t[pre + ".rm"], rv=t[pre + ".rv"])
        z, dz, und = N.bn_check_fwd(st, inp, out, relu, res is not None, True, BF, self.errs, EPS, MOM,
                                    (t[pre + ".rm0"], t[pre + ".rv0"]))
        self._counter(st, t, pre)
        u = None
        if out["mask"] is not None:
            pos = N.mask_bits(out["mask"], z.shape)
        elif relu:
            pos, u = z > 0, (und if bool(und.any()) else None)
        else:
            pos = torch.ones_like(z, dtype=torch.bool)
        if relu:
            self.und[st] = float(und.double().mean())
        g = inp["dy"].double() * pos
        bout = dict(dx=rows(t[dx]), dw=t[f"g.{pre}.w"], db=t[f"g.{pre}.b"])
        if dres and res is not None:
            if "d.residual" not in t:
                self.errs.append(f"{st} dres: no gradient arrived at the residual")
            else:
                bout["dres"] = rows(t["d.residual"])
        N.bn_check_bwd(st, inp, bout, t["s.mean"], t["s.inv"], g, True, BF, self.errs, und=u)

    def _bn_from_stats(self, st, e):
        self._bn(st, e, dres=self.kind[3])  # (an identity block's residual gradient is the block input's)

    _FusedBatchNorm2d = _bn_from_stats

    def _stats(self, st, t, x2, pre, mk, ik):
        """The statistics part of ``bn_check_fwd`` for a norm inside a fused node: save_mean, save_invstd,
        the running statistics and the counter. Returns float64 (mean, inv, dmean, dinv)."""
        n, C = x2.shape
        mean, var, a1, a2 = N.stats_ref(x2, 0)
        inv, dmean, dinv, _ = N.single_pass_bounds(N.bn_L(n, C), mean, var, a1, a2, EPS)
        E.check(f"{st} {pre}.save_mean", t[mk], mean, dmean + TINY, self.errs)
        E.check(f"{st} {pre}.save_invstd", t[ik], inv, dinv + TINY, self.errs)
        unb = var * n / max(n - 1, 1)
        rm0, rv0 = t[pre + ".rm0"].double(), t[pre + ".rv0"].double()
        dunb = (inv ** -3) * 2 * dinv * n / max(n - 1, 1) + 4 * U32 * unb
        E.check(f"{st} {pre}.running_mean", t[pre + ".rm"], (1 - MOM) * rm0 + MOM * mean,
                MOM * dmean + 4 * U32 * (rm0.abs() + mean.abs()) + TINY, self.errs)
        E.check(f"{st} {pre}.running_var", t[pre + ".rv"], (1 - MOM) * rv0 + MOM * unb,
                MOM * dunb + 4 * U32 * (rv0.abs() + unb) + TINY, self.errs)
        self._counter(st, t, pre)
        return mean, inv, dmean, dinv

    def _dual_fwd(self, st, t, c3, cds):
        zs = []
        for x4, pre, mk, ik in ((c3, "bn", "s.mean", "s.inv"), (cds, "bn_ds", "s.mean2", "s.inv2")):
            x2 = rows(x4)
            mean, inv, dmean, dinv = self._stats(st, t, x2, pre, mk, ik)
            z, _, dz, _ = N.affine_fwd_ref(x2, t[pre + ".w"], t[pre + ".b"], None, False, mean, inv, dmean, dinv, BF)
            zs.append((z, dz))
        z = zs[0][0] + zs[1][0]
        dz = zs[0][1] + zs[1][1] + 2 * U32 * z.abs()
        yr = z.clamp_min(0)
        E.check(f"{st} y", rows(t["y"]), yr, dz + N.rt(BF, yr) + TINY, self.errs)
        und = N.undecided(z, dz, st, self.errs)
        self.und[st] = float(und.double().mean())
        N.check_mask(f"{st} mask", t["s.mask"], z, und, self.errs)
        return N.mask_bits(t["s.mask"], z.shape)

    def _dual_bn_relu(self, st, e):
        t = e["t"]
        pos = self._dual_fwd(st, t, t["c3"], t["cds"])
        g = rows(t["d.y"]).double() * pos
        for x, pre, mk, ik in (("c3", "bn", "s.mean", "s.inv"), ("cds", "bn_ds", "s.mean2", "s.inv2")):
            inp = dict(x=rows(t[x]), w=t[pre + ".w"], dy=rows(t["d.y"]))
            bout = dict(dx=rows(t["d." + x]), dw=t[f"g.{pre}.w"], db=t[f"g.{pre}.b"])
            N.bn_check_bwd(f"{st} {pre}", inp, bout, t[mk], t[ik], g, True, BF, self.errs)

    # ---- nodes that never store an intermediate
    def _one_pass(self, st, tag, t, c, pre, mk, ik, g, act, w, d_act, gw):
        """One branch of the one-pass backward: dgamma / dbeta, then d_act = dx . W and dW = dx^T . act
        from the float64 dx of ``bn_bwd_ref`` and its bound. Returns (reference, bound) of d_act [P, Cin]."""
        inp = dict(x=rows(c), w=t[pre + ".w"], dy=rows(t["d.y"]))
        r = N.bn_bwd_ref(inp, t[mk], t[ik], g, True, BF)
        E.check(f"{st} {tag}{pre}.db", t[f"g.{pre}.b"], r["db"], r["ddb"], self.errs)
        E.check(f"{st} {tag}{pre}.dw", t[f"g.{pre}.w"], r["dw"], r["ddw"], self.errs)
        dx, ddx = r["dx"], r["ddx"]
        w2, a2 = w.reshape(w.shape[0], -1).double(), rows(act).double()
        hi = dx.abs() + ddx
        R = dx @ w2
        bnd = E.bound(R, hi @ w2.abs(), w2.shape[0], "bf16") + ddx @ w2.abs()
        if d_act is False:
            self.errs.append(f"{st} {tag}input-gradient: no gradient arrived at the stage's input")
        elif d_act is not None:
            E.check(f"{st} {tag}input-gradient", rows(d_act), R, bnd, self.errs)
        Rw = dx.t() @ a2
        E.check(f"{st} {tag}filter-gradient", gw.reshape(Rw.shape), Rw,
                E.bound(Rw, hi.t() @ a2.abs(), dx.shape[0], "bf16") + ddx.t() @ a2.abs(), self.errs)
        return R, bnd

    def _handed(self, st, t, key="c3"):
        given = t.get(key) is not None
        if given and not torch.equal(t[key].view(torch.int16), t["s.c3"].view(torch.int16)):
            self.errs.append(f"{st} c3= hand-over: the node normalised another c3 than the one handed over")
        return given

    def _conv3_bn3_relu(self, st, e):
        t = e["t"]
        given = self._handed(st, t)
        if o3_of(self.r) and not given:
            R, A, K = conv_ref("fwd", t["a2"], t["conv.w"], None, 1)
            E.check(f"{st} forward", t["s.c3"], R, E.bound(R, A, K, "bf16"), self.errs)
        inp = dict(x=rows(t["s.c3"]), w=t["bn.w"], b=t["bn.b"], res=rows(t["residual"]), dy=rows(t["d.y"]))
        out = dict(mean=t["s.mean"], inv=t["s.inv"], y=rows(t["y"]), mask=t["s.mask"], rm=t["bn.rm"], rv=t["bn.rv"])
        z, dz, und = N.bn_check_fwd(st, inp, out, True, True, True, BF, self.errs, EPS, MOM, (t["bn.rm0"], t["bn.rv0"]))
        self._counter(st, t, "bn")
        self.und[st] = float(und.double().mean())
        g = inp["dy"].double() * N.mask_bits(t["s.mask"], z.shape)
        self._one_pass(st, "", t, t["s.c3"], "bn", "s.mean", "s.inv", g, t["a2"], t["conv.w"], t.get("d.a2", False), t["g.conv.w"])

    def _conv3ds_bn_relu(self, st, e):
        t = e["t"]
        given = self._handed(st, t)
        if o3_of(self.r) and not given:
            R, A, K = conv_ref("fwd", t["a2"], t["conv3.w"], None, 1)
            E.check(f"{st} conv3-forward", t["s.c3"], R, E.bound(R, A, K, "bf16"), self.errs)
        if ds_stats(self.kind, self.r):
            R, A, K = conv_ref("fwd", t["x"], t["ds_conv.w"], None, 1)
            E.check(f"{st} ds-forward", t["s.cds"], R, E.bound(R, A, K, "bf16"), self.errs)
        pos = self._dual_fwd(st, t, t["s.c3"], t["s.cds"])
        g = rows(t["d.y"]).double() * pos
        self._one_pass(st, "conv3-", t, t["s.c3"], "bn", "s.mean", "s.inv", g, t["a2"], t["conv3.w"], t.get("d.a2", False),
                       t["g.conv3.w"])
        self.side = self._one_pass(st, "ds-", t, t["s.cds"], "bn_ds", "s.mean2", "s.inv2", g, t["x"], t["ds_conv.w"], None,
                                   t["g.ds_conv.w"])

    def _bn_relu_conv3(self, st, e):
        t = e["t"]
        self._bn(st, e, x="c2", y="y0", dy="d.y0", dx="d.c2", relu=True)
        R, A, K = conv_ref("fwd", t["y0"], t["conv.w"], None, 1)
        E.check(f"{st} forward", t["y1"], R, E.bound(R, A, K, "bf16"), self.errs)

    def _bn_relu_conv1x1(self, st, e):
        t = e["t"]
        x2 = rows(t["c2"])
        n = x2.shape[0]
        mean, inv, dmean, dinv = self._stats(st, t, x2, "bn", "s.mean", "s.inv")
        z, a2, dz, da2 = N.affine_fwd_ref(x2, t["bn.w"], t["bn.b"], None, True, mean, inv, dmean, dinv, BF)
        und = N.undecided(z, dz, st, self.errs)
        self.und[st] = float(und.double().mean())
        w2 = t["weight"].reshape(t["weight"].shape[0], -1).double()
        hi = a2 + da2
        R = a2 @ w2.t()
        E.check(f"{st} forward", rows(t["y"]), R, E.bound(R, hi @ w2.abs().t(), w2.shape[1], "bf16") + da2 @ w2.abs().t(),
                self.errs)
        dc3 = rows(t["d.y"]).double()
        Rw = dc3.t() @ a2
        E.check(f"{st} filter-gradient", t["g.weight"].reshape(Rw.shape), Rw,
                E.bound(Rw, dc3.abs().t() @ hi, n, "bf16") + dc3.abs().t() @ da2, self.errs)
        da = dc3 @ w2
        bda = E.bound(da, dc3.abs() @ w2.abs(), w2.shape[0], "bf16")
        g = da * (z > 0)
        inp = dict(x=x2, w=t["bn.w"], dy=da)
        u = und if bool(und.any()) else None
        r = N.bn_bwd_ref(inp, t["s.mean"], t["s.inv"], g, True, BF, u)
        delta = bda * ((z > 0) | und)
        xc = x2.double() - t["s.mean"].double()
        xhat = xc * t["s.inv"].double()
        eb, ew = delta.sum(0), (delta * xhat.abs()).sum(0)
        A = r["A"]
        ddx = r["ddx"] + A.abs() * delta + A.abs() * eb / n + (A * t["s.inv"].double() * xc).abs() * ew / n
        E.check(f"{st} bn.db", t["g.bn.b"], r["db"], r["ddb"] + eb, self.errs)
        E.check(f"{st} bn.dw", t["g.bn.w"], r["dw"], r["ddw"] + ew, self.errs)
        dx = rows(t["d.c2"])
        if u is not None:
            flip = torch.where(g == 0, da, torch.zeros_like(da))
            N.check_either(f"{st} dx", dx, r["dx"], r["dx"] + A * (flip - g), ddx, und, self.errs)
        else:
            E.check(f"{st} dx", dx, r["dx"], ddx, self.errs)

    # ---- the block input's gradient
    def _block_input(self, record, want):
        t = record[0]["t"]
        if not self.r["needs"]:  # (no hook on an input that needs no gradient: the test asserts that it got none)
            return
        if "d.x" not in t:
            self.errs.append("conv1 block-input: no gradient arrived at the block input")
            return
        R1, A1, K1 = conv_ref("dgrad", t["x"], t["weight"], t["d.y"], 1)
        last = record[-1]["t"]
        if not self.kind[3]:
            side = last["d.y"].double() * unrows(N.mask_bits(last["s.mask"], rows(last["d.y"]).shape), *_nhw(last["d.y"]))
            bnd = E.bound(R1, A1, K1, "res", res=side)
        else:
            if self.side is not None:
                side, b2 = (unrows(v, *_nhw(t["x"])) for v in self.side)
            else:
                ds = next(e for e, (_, st) in zip(record, want) if st == "ds")["t"]
                side, A2, K2 = conv_ref("dgrad", ds["x"], ds["weight"], ds["d.y"], self.kind[2])
                b2 = E.bound(side, A2, K2, "bf16")
            # = bound(R1, A1, K1, "res", side) + (1 + u8) b2 + u8 bound(R1, A1, K1, "bf16"), b1 formed once
            b1 = E.bound(R1, A1, K1, "bf16")
            bnd = b1.mul_(1 + U8).add_((R1 + side).abs_().mul_(U8)).add_(b2.mul_(1 + U8))
        self.bounded.add("conv1")
        E.check("conv1 block-input-gradient", t["d.x"], R1 + side, bnd, self.errs)


def _nhw(t):
    return t.shape[0], t.shape[2], t.shape[3]


# ------------------------------------------------------------------------------- the emulation

def _mm(p, q):
    """bf16(P Q^T) with float32 accumulation."""
    return (p.float() @ q.float().t()).bfloat16()


def _bn_state(c):
    return dict(rm0=torch.zeros(c), rv0=torch.ones(c), nbt0=torch.tensor(0))


def _bn_fwd(x4, p, relu, res4, defect=None):
    n, c, h, w = x4.shape
    inp = dict(x=rows(x4), w=p["w"], b=p["b"], res=rows(res4) if res4 is not None else None)
    o = N.bn_emulate_fwd(inp, relu, res4 is not None, True, BF, torch.zeros(16, 2, c), (p["rm0"], p["rv0"]), EPS, MOM, defect)
    o["y4"] = unrows(o["y"], n, h, w)
    o["inp"] = inp
    return o


def _bn_bwd(o, p, g2):
    inp = dict(o["inp"])
    return N.bn_emulate_bwd(inp, o["mean"], o["inv"], g2.float(), True, BF, torch.zeros(16, 2, g2.shape[1]))


def _bn_keys(pre, p, o):
    return {pre + ".w": p["w"], pre + ".b": p["b"], pre + ".rm0": p["rm0"], pre + ".rv0": p["rv0"], pre + ".nbt0": p["nbt0"],
            pre + ".rm": o["rm"], pre + ".rv": o["rv"], pre + ".nbt": p["nbt0"] + 1}


def emulate(kind, r, inp, defect=None):
    """The block in float32 PyTorch on the CPU (float32 accumulation, bf16 where the route stores or a
    kernel rounds an MFMA operand), as a record in the recorder's format; ``defect``: one of ``DEFECTS``."""
    cin, width, stride, ds = kind
    cout = 4 * width
    x, w1, w2, w3, wds, dy = inp["x"], inp["w1"], inp["w2"], inp["w3"], inp["wds"], inp["dy"]
    n, _, h, _ = x.shape
    ho = h // stride
    P = n * ho * ho
    bn = {k: dict(inp[k], **_bn_state(inp[k]["w"].numel())) for k in ("bn1", "bn2", "bn3", "bn_ds")}
    dual = ds and r["dual"]
    names = plan(kind, r)
    # ---- forward
    c1 = unrows(_mm(rows(x), w1.view(width, cin)), n, h, h)
    o1 = _bn_fwd(c1, bn["bn1"], True, None)
    a1 = o1["y4"]
    c2 = F.conv2d(a1.float(), w2.float(), None, stride, 1).bfloat16()
    o2 = _bn_fwd(c2, bn["bn2"], True, None)
    a2 = o2["y4"]
    c3 = unrows(_mm(rows(a2), w3.view(cout, width)), n, ho, ho)
    c3_used = c3
    if defect == "c3_recomputed":  # the consumer ignores c3= and recomputes it, rounded twice
        c3_used = unrows((rows(a2).float() @ w3.view(cout, width).float().t()).half().bfloat16(), n, ho, ho)
    cds = ods = idn = None
    if ds:
        xs = x[:, :, ::stride, ::stride]
        cds = unrows(_mm(rows(xs), wds.view(cout, cin)), n, ho, ho)
    if ds and not dual:
        ods = _bn_fwd(cds, bn["bn_ds"], False, None)
        idn = ods["y4"]
    fdef = "biased_running_var" if defect == "biased_running_var" else None
    if dual:
        o3, ods = _bn_fwd(c3_used, bn["bn3"], False, None, fdef), _bn_fwd(cds, bn["bn_ds"], False, None)
        if defect == "stats_swapped":
            for k in ("mean", "inv"):
                o3[k], ods[k] = ods[k], o3[k]
        zs = []
        for o, p, c in ((o3, bn["bn3"], c3_used), (ods, bn["bn_ds"], cds)):
            sc = p["w"] * o["inv"]
            zs.append(rows(c).float() * sc + (p["b"] - o["mean"] * sc))
        z = zs[0] + zs[1]
        pos = z > 0
        out = unrows(torch.where(pos, z, torch.zeros_like(z)).bfloat16(), n, ho, ho)
        mask = N.mask_bytes(pos)
    else:
        o3 = _bn_fwd(c3_used, bn["bn3"], True, x if not ds else idn, fdef)
        out, mask = o3["y4"], o3["mask"]
        pos = N.mask_bits(mask, (P, cout))
    if defect == "mask_shifted":  # the last partial tile's mask rows read one row off
        pos = pos.clone()
        lo = P - P % 32
        pos[lo:] = pos[lo:].roll(1, 0)
        mask = N.mask_bytes(pos)
    # ---- backward
    g = (rows(dy).float() * pos).bfloat16()
    b3 = _bn_bwd(o3, bn["bn3"], g)
    bds = None
    if ds:
        bds = _bn_bwd(ods, bn["bn_ds"], g)
    if defect == "sums_swapped_bwd":  # each branch's dx formed from the other's finished sums
        for b, o, p, other in ((b3, o3, bn["bn3"], bds), (bds, ods, bn["bn_ds"], dict(b3))):
            xf = o["inp"]["x"].float()
            sc = p["w"] * o["inv"]
            k2, k3 = other["db"] / P, other["dw"] / P
            b["dx"] = (sc * g.float() + (-sc * o["inv"] * k3 * xf + sc * (o["mean"] * o["inv"] * k3 - k2))).bfloat16()
    if defect == "dbeta_32_63_zero":
        b3["db"] = b3["db"].clone()
        b3["db"][32:64] = 0
    dx3 = b3["dx"]
    d_a2 = _mm(dx3, w3.view(cout, width).t())
    keep = torch.ones(P, dtype=torch.bool)
    if defect == "wgrad_slab_omitted":
        keep[32:64] = False
    dw3 = _mm(dx3[keep].t(), rows(a2)[keep].t()).view_as(w3)
    g2 = (d_a2.float() * (o2["y"] > 0)).bfloat16()
    b2 = _bn_bwd(o2, bn["bn2"], g2)
    dc2 = unrows(b2["dx"], n, ho, ho)
    d_a1 = torch.nn.grad.conv2d_input(tuple(a1.shape), w2.float(), dc2.float(), stride, 1).bfloat16()
    dw2 = torch.nn.grad.conv2d_weight(a1.float(), tuple(w2.shape), dc2.float(), stride, 1).bfloat16()
    g1 = (rows(d_a1).float() * (o1["y"] > 0)).bfloat16()
    b1 = _bn_bwd(o1, bn["bn1"], g1)
    dc1 = unrows(b1["dx"], n, h, h)
    dw1 = _mm(b1["dx"].t(), rows(x).t()).view_as(w1)
    if ds:
        dxds = bds["dx"]
        dwds = _mm(dxds.t(), rows(xs).t()).view_as(wds)
        side = torch.zeros(n, cin, h, h)
        side[:, :, ::stride, ::stride] = unrows(_mm(dxds, wds.view(cout, cin).t()), n, ho, ho).float()
    else:
        side = unrows(g, n, h, h).float()
    acc = unrows(rows(dc1).float() @ w1.view(width, cin).float(), n, h, h)
    s2 = rows(side).clone()
    if defect == "res_missing_last_tile":
        s2[n * h * h - (n * h * h) % 32:] = 0
    elif defect == "res_twice":
        s2 = 2 * s2
    dx = (acc + unrows(s2, n, h, h)).bfloat16()
    # ---- the record
    k1, k2, k3 = _bn_keys("bn", bn["bn1"], o1), _bn_keys("bn", bn["bn2"], o2), _bn_keys("bn", bn["bn3"], o3)
    kds = _bn_keys("bn_ds", bn["bn_ds"], ods) if ds else {}
    gb = lambda pre, b: {f"g.{pre}.w": b["dw"], f"g.{pre}.b": b["db"]}
    s3 = {"s.mean": o3["mean"], "s.inv": o3["inv"], "s.mask": mask}
    sds = {"s.mean2": ods["mean"], "s.inv2": ods["inv"]} if dual else {}
    dxk = {"d.x": dx} if r["needs"] else {}
    b2c3 = ("bn_relu_conv3", "bn2+conv3fwd") in names
    dy3 = unrows(dx3, n, ho, ho)
    rec = []
    for name, st in names:
        if st == "conv1":
            t = dict(x=x, weight=w1, y=c1, **dxk, **{"d.y": dc1, "g.weight": dw1})
        elif st == "bn1":
            t = dict(x=c1, y=a1, **k1, **gb("bn", b1), **{"s.mean": o1["mean"], "s.inv": o1["inv"], "d.x": dc1, "d.y": d_a1})
        elif st == "ds":
            t = dict(x=x, weight=wds, y=cds, **dxk, **{"d.y": unrows(dxds, n, ho, ho), "g.weight": dwds})
        elif st == "bn_ds":
            t = dict(x=cds, y=idn, **{k.replace("bn_ds", "bn"): v for k, v in kds.items()},
                     **{"s.mean": ods["mean"], "s.inv": ods["inv"], "d.x": unrows(dxds, n, ho, ho), "d.y": unrows(g, n, ho, ho),
                        "g.bn.w": bds["dw"], "g.bn.b": bds["db"]})
        elif st == "conv2":
            wk = "conv.w" if name == "nn.Conv2d" else "weight"
            t = {"x": a1, wk: w2, "y": c2, "d.x": d_a1, "d.y": dc2, "g." + wk: dw2}
        elif st == "bn2":
            t = dict(x=c2, y=a2, **k2, **gb("bn", b2), **{"s.mean": o2["mean"], "s.inv": o2["inv"], "d.x": dc2,
                                                          "d.y": unrows(d_a2, n, ho, ho)})
        elif st == "bn2+conv3fwd":
            t = dict(c2=c2, y0=a2, y1=c3, **k2, **gb("bn", b2), **{"conv.w": w3, "s.mean": o2["mean"], "s.inv": o2["inv"],
                                                                   "d.c2": dc2, "d.y0": unrows(d_a2, n, ho, ho)})
        elif st == "bn2+conv3":
            t = dict(c2=c2, weight=w3, y=c3, **k2, **gb("bn", b2), **{"s.mean": o2["mean"], "s.inv": o2["inv"], "d.c2": dc2,
                                                                      "d.y": dy3, "g.weight": dw3})
        elif st == "conv3":
            t = dict(x=a2, weight=w3, y=c3_used, **{"d.x": unrows(d_a2, n, ho, ho), "d.y": dy3, "g.weight": dw3})
            if b2c3:
                t["c"] = c3
        elif st == "bn3":
            t = dict(x=c3_used, y=out, residual=x if not ds else idn, **k3, **gb("bn", b3), **s3,
                     **{"d.x": dy3, "d.y": dy})
            if ds:
                t["d.residual"] = unrows(g, n, ho, ho)
        elif st == "bn3+bn_ds":
            t = dict(c3=c3_used, cds=cds, y=out, **k3, **kds, **gb("bn", b3), **gb("bn_ds", bds), **s3, **sds,
                     **{"d.c3": dy3, "d.cds": unrows(dxds, n, ho, ho), "d.y": dy})
        elif st == "conv3+bn3":
            t = dict(a2=a2, residual=x, y=out, **k3, **gb("bn", b3), **s3,
                     **{"conv.w": w3, "s.c3": c3_used, "d.a2": unrows(d_a2, n, ho, ho), "d.y": dy, "g.conv.w": dw3})
            if b2c3:
                t["c3"] = c3
        elif st == "conv3+ds+bn3":
            t = dict(a2=a2, x=x, y=out, **k3, **kds, **gb("bn", b3), **gb("bn_ds", bds), **s3, **sds,
                     **{"conv3.w": w3, "ds_conv.w": wds, "s.c3": c3_used, "s.cds": cds, "d.a2": unrows(d_a2, n, ho, ho),
                        "d.y": dy, "g.conv3.w": dw3, "g.ds_conv.w": dwds})
            if b2c3:
                t["c3"] = c3
        meta = dict(relu=st in ("bn1", "bn2", "bn3"))
        rec.append(dict(name=name, t=t, meta=meta))
    return rec


# ------------------------------------------------------------------------------- the exact case

def exact_operands(pixels, cout, width):
    """Ternary (dy [P, cout], a2 [P, width], W3 [cout, width]) of ``mfma_edges.linbwd_inputs``: at most
    ``width`` products per c3 element, cout / 4 per d_a2 element and P / 4 per dW3 element, all +-1."""
    return E.linbwd_inputs("ternary", pixels, cout, width, 7)


def exact_conv3(t, errs):
    """conv3's forward, input gradient and filter gradient of one recorded ``conv1x1_hybrid`` call on
    substituted ternary operands must equal the float64 results, which are integers that bf16 holds."""
    for what, key, op in (("forward", "y", "fwd"), ("input-gradient", "d.x", "dgrad"), ("filter-gradient", "d.weight", "wgrad")):
        if key not in t:
            errs.append(f"conv3 exact {what}: not recorded")
            continue
        R, A, _ = conv_ref(op, t["x"], t["weight"], t.get("d.y"), 1)
        assert float(A.max()) <= 256 and bool((R.bfloat16().double() == R).all()), "the reference itself must be exact in bf16"
        assert float(R.abs().max()) > 0
        E.check(f"conv3 exact {what}", t[key], R, None, errs)
