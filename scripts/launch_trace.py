"""The sequence of native launches of the ResNet path's Python host layer, as a refactor check.

BatchNorm statistics and weight gradients use float atomics, so a digest of results cannot prove that a
change of host code changed nothing; the launches can: which entries of the extension are called, in
what order, with which scalars, null pointers and dataflow links is fully determined by the host code.
(The same kind of check as ``scripts/isa_equal.py`` for device code and ``scripts/optim_digest.py``.)

:func:`recording` puts a stand-in in place of ``_ext.get()``, the one way into the extension, that forwards
every call and logs ``entry(arguments)``; the vendor calls (``F.conv2d``, ``aten.convolution_backward``) are logged
the same way, tensors as ``shape@address``. An integer >= 2^40 is a device address and is written as
``a<k>``, k the order of first appearance in the case, so the trace does not depend on where the
allocator put things; 0 stays 0, lists go element by element, everything else is written verbatim.
While a case is traced every tensor stays alive (:func:`keep_alive`), so no address is used twice.

    python scripts/launch_trace.py --out trace.json        # the trace (tests/golden/resnet_launch_trace.json)
    python scripts/launch_trace.py --aten --out aten.json   # per case the multiset of (aten op, input shapes)

Both print, per case, which Python function issued which entries (the coverage of the launch sites).
"""
from __future__ import annotations

import argparse
import collections
import contextlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ADDRESS_MIN = 1 << 40

# allocations and views: excluded when two ATen multisets are compared (their counts are still printed).
# aten::to and aten::contiguous are the wrappers that hand back their argument when there is nothing to do;
# a conversion or a layout copy they do make is aten::_to_copy / aten::clone + aten::copy_, which are compared.
ATEN_EXCLUDED = ("aten::to", "aten::contiguous",
                 "aten::empty", "aten::empty_like", "aten::empty_strided", "aten::new_empty", "aten::view",
                 "aten::_unsafe_view", "aten::reshape", "aten::_reshape_alias", "aten::permute", "aten::as_strided",
                 "aten::detach", "aten::alias", "aten::t", "aten::transpose", "aten::expand", "aten::select",
                 "aten::slice", "aten::unsqueeze", "aten::squeeze", "aten::view_as", "aten::expand_as",
                 "aten::result_type", "aten::is_nonzero", "aten::item", "aten::_local_scalar_dense",
                 "aten::resolve_conj", "aten::resolve_neg", "aten::lift_fresh")


class Recorder:
    """The log of one case: ``records`` (strings ``entry(arg,...)``) and ``callers`` (who issued them)."""

    def __init__(self):
        self.records: list = []
        self.callers: list = []
        self._addr: dict = {}

    def sym(self, v):
        if isinstance(v, bool) or v is None:
            return str(v)
        if isinstance(v, int):
            if v >= ADDRESS_MIN:
                return "a%d" % self._addr.setdefault(v, len(self._addr))
            return str(v)
        if isinstance(v, (list, tuple)):
            return "[" + ",".join(self.sym(e) for e in v) + "]"
        if hasattr(v, "data_ptr") and hasattr(v, "shape"):  # a tensor handed to a vendor call
            return "x".join(str(int(d)) for d in v.shape) + "@" + self.sym(v.data_ptr())
        return repr(v)

    def add(self, name, args, kwargs, frame):
        parts = [self.sym(a) for a in args] + ["%s=%s" % (k, self.sym(kwargs[k])) for k in sorted(kwargs)]
        self.records.append("%s(%s)" % (name, ",".join(parts)))
        code = frame.f_code
        self.callers.append("%s:%d:%s" % (os.path.basename(code.co_filename), code.co_firstlineno, code.co_name))


class _Proxy:
    """Forwards every attribute of the extension module; calls are logged first."""

    def __init__(self, mod, rec):
        self.__dict__.update(_mod=mod, _rec=rec)

    def __getattr__(self, name):
        v = getattr(self._mod, name)
        if not callable(v):
            return v
        rec = self._rec

        def call(*args, **kwargs):
            rec.add(name, args, kwargs, sys._getframe(1))
            return v(*args, **kwargs)
        return call


def keep_alive():
    """A dispatch mode that holds on to every tensor an ATen op returns (autograd's worker threads inherit it):
    while it is active nothing is freed, so no address is handed out twice and one ``a<k>`` is one tensor,
    whatever the caching allocator held before the case."""
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from torch.utils._pytree import tree_map_only

    class KeepAlive(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.kept = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            tree_map_only(torch.Tensor, self.kept.append, out)
            return out

    return KeepAlive()


class _Vendor:
    """Stands in for a vendor call: logs, then forwards; every other attribute is the original's (torch itself
    looks up ``aten.convolution_backward.default``)."""

    def __init__(self, orig, rec, name):
        self.__dict__.update(_orig=orig, _rec=rec, _name=name)

    def __call__(self, *args, **kwargs):
        self._rec.add(self._name, args, kwargs, sys._getframe(1))
        return self._orig(*args, **kwargs)

    def __getattr__(self, name):
        return getattr(self._orig, name)


@contextlib.contextmanager
def recording(rec: Recorder, ext=None, vendor: bool = True):
    """Log into ``rec`` every call made through ``ext.get()`` (default: ``ops._ext``) and,
    with ``vendor``, through ``F.conv2d`` / ``aten.convolution_backward``; the originals are put back on exit."""
    if ext is None:
        from fluxmpi_amd.ops import _ext as ext
    get = ext.get

    def rec_get(*a, **k):
        mod = get(*a, **k)
        return None if mod is None else _Proxy(mod, rec)

    undo = [(ext, "get", get)]
    ext.get = rec_get
    try:
        if vendor:
            import torch
            conv2d, conv_bwd = torch.nn.functional.conv2d, torch.ops.aten.convolution_backward
            undo += [(torch.nn.functional, "conv2d", conv2d), (torch.ops.aten, "convolution_backward", conv_bwd)]
            torch.nn.functional.conv2d = _Vendor(conv2d, rec, "F.conv2d")
            torch.ops.aten.convolution_backward = _Vendor(conv_bwd, rec, "aten.convolution_backward")
        yield rec
    finally:
        for obj, name, orig in reversed(undo):
            setattr(obj, name, orig)


# ------------------------------------------------------------------------------------------ cases

@contextlib.contextmanager
def _isolated(other=(), wg=None, switches=(), wgrad="ours"):
    """Empty frozen choice tables (plus the case's entries), the case's module switches, an empty
    transposed-filter cache; everything as it was afterwards. ``other``: ``(input shape, Cout[, stride])``
    of the convolutions whose forward (and narrow-channel input gradient) goes to MIOpen + the statistics
    pass and whose weight gradient goes to our split-K kernel (``wgrad="miopen"``: stays on MIOpen)."""
    from fluxmpi_amd.ops import conv_choice as CC
    from fluxmpi_amd.ops import gemm as G
    tables = [getattr(CC, n) for n in CC._CHOICE_TABLES.values()]
    saved = [dict(t) for t in tables]
    filt, frozen = dict(G._FILT), CC.choices_frozen()
    pick = (wgrad, CC._WG_CONFIGS[0] if wgrad == "ours" else None)
    old = [(m, n, getattr(m, n)) for m, n, _ in switches]
    try:
        for t in tables:
            t.clear()
        G._FILT.clear()
        CC.freeze_choices(True)
        for key in other:
            if len(key) == 3:
                CC._DS_CHOICE[key] = False
                CC._WG_CHOICE[("ds",) + key] = pick
            else:
                CC._FWD1_CHOICE[key] = CC._FWD_CHOICE[key] = CC._S2_CHOICE[key] = CC._DGRAD_CHOICE[key] = False
                for kind in ("1x1", "3x3", "3x3s2"):
                    CC._WG_CHOICE[(kind,) + key] = pick
        CC._WG_CHOICE.update(wg or {})
        for m, n, v in switches:
            setattr(m, n, v)
        yield
    finally:
        for m, n, v in old:
            setattr(m, n, v)
        CC.freeze_choices(frozen)
        G._FILT.clear()
        G._FILT.update(filt)
        for t, s in zip(tables, saved):
            t.clear()
            t.update(s)


def _bf16(mod):
    import torch
    mod = mod.cuda().to(memory_format=torch.channels_last)
    for m in mod.modules():
        if not isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            for p in m.parameters(recurse=False):
                p.data = p.data.bfloat16()
    return mod.train()


def _x(*shape, grad=True, dtype=None):
    import torch
    x = torch.randn(*shape, device="cuda").to(dtype or torch.bfloat16)
    if len(shape) == 4:
        x = x.contiguous(memory_format=torch.channels_last)
    return x.requires_grad_(grad)


def _w(*shape):
    import torch
    return (torch.randn(*shape, device="cuda") * 0.1).bfloat16().contiguous(
        memory_format=torch.channels_last).requires_grad_()


def _backward(y):
    import torch
    g = torch.randn_like(y)
    (y.float() * g).sum().backward()
    torch.cuda.synchronize()


def _block(cin, width, stride=1, ds=False, impl="hybrid"):
    import torch.nn as nn
    from fluxmpi_amd.models.resnet import Bottleneck, _norm, conv1x1
    down = nn.Sequential(conv1x1(cin, 4 * width, stride, "miopen"), _norm(4 * width, "fused")) if ds else None
    return _bf16(Bottleneck(cin, width, stride, down, impl, "fused"))


def _run_block(cin, width, stride=1, ds=False, impl="hybrid", hw=14):
    def body():
        block = _block(cin, width, stride, ds, impl)  # alive over the backward: so are its buffers' addresses
        _backward(block(_x(2, cin, hw, hw)))
    return body


def _bn(ch, **kw):
    from fluxmpi_amd.ops.batchnorm import FusedBatchNorm2d
    return FusedBatchNorm2d(ch, **kw).cuda().train()


def _bn_case(relu=False, res=False, link=None, shape=(2, 64, 14, 14), sync=False, dtype=None, **kw):
    def body():
        from fluxmpi_amd.ops import batchnorm as B
        from fluxmpi_amd.ops.syncbn import SyncBatchNorm2d
        bn = SyncBatchNorm2d(shape[1], **kw).cuda().train() if sync else _bn(shape[1], **kw)
        r = _x(*shape, dtype=dtype) if res else None
        lk = None if link is None else B.GradLink(masked=link == "masked")
        _backward(bn(_x(*shape, dtype=dtype), relu=relu, residual=r, link=lk))
    return body


def _bn_eval(res):
    def body():
        import torch
        bn = _bn(64).eval()
        with torch.no_grad():
            bn(_x(2, 64, 14, 14, grad=False), relu=True, residual=_x(2, 64, 14, 14, grad=False) if res else None)
        torch.cuda.synchronize()
    return body


def _syncbn_ops():
    """The op-level protocol (one process playing a rank): both messages, the finalize, the apply, the dx."""
    import torch
    from fluxmpi_amd.ops import syncbn as S
    x, r, dy = (_x(2, 64, 14, 14, grad=False) for _ in range(3))
    w, b = torch.ones(64, device="cuda"), torch.zeros(64, device="cuda")
    rm, rv = torch.zeros(64, device="cuda"), torch.ones(64, device="cuda")
    nbt = torch.zeros((), device="cuda", dtype=torch.long)
    msg = S.forward_message(x)
    y, mask, sm, si = S.apply_from_message(x, msg, w, b, rm, rv, 0.1, 1e-5, True, r, nbt)
    bmsg, _, _ = S.backward_message(dy, x, mask, w, b, sm, si, True)
    S.dx_from_message(dy, x, mask, w, b, sm, si, bmsg, msg[128:], True, True)
    torch.cuda.synchronize()


def _bnlink_case(k, with_res, gradlink=False):
    def body():
        from fluxmpi_amd.ops import fused_block as fb
        ch = 128 if k == 1 else 64
        bn, link = _bn(ch), fb.BNStatsLink()
        c = _x(2, ch, 14, 14)
        r = _x(2, ch, 14, 14) if with_res else None
        y = bn(c, relu=True, residual=r, bnlink=link)
        if k == 1:
            z = fb.conv1x1_hybrid(y, _w(64, ch, 1, 1), None, link)
        else:
            gl = fb.GradLink() if gradlink else None
            z = fb.conv3x3(y, _w(64, 64, 3, 3), bnlink=link, gradlink=gl)
            if gl is not None:  # y's other consumer deposited its gradient of y
                gl.grad = _x(2, 64, 14, 14, grad=False)
        _backward(z)
    return body


def _conv1x1_case(n, hw, ci, co, ds_stride=None, link=True):
    def body():
        from fluxmpi_amd.ops import fused_block as fb
        x, w = _x(n, ci, hw, hw), _w(co, ci, 1, 1)
        if ds_stride is None:
            y = fb.conv1x1_hybrid(x, w)
        else:
            y = fb.conv1x1_downsample(x, w, ds_stride, fb.SideGradLink() if link else None)
        _backward(y)
    return body


def _conv1x1_stats_splitk():
    """Enough rows (8 x 28 x 28) for the register-staged weight gradient to split K: partials + the reduce."""
    from fluxmpi_amd.ops import fused_block as fb
    bn = _bn(64)
    _backward(fb.bn_from_stats(fb.conv1x1_stats(_x(8, 64, 28, 28), _w(64, 64, 1, 1)), bn, relu=True))


def _conv3x3_c48():
    """Channels that are no multiple of 32: the input gradient is a per-shape choice (here MIOpen), the
    gradient of x's other consumer arrives through a GradLink."""
    from fluxmpi_amd.ops import fused_block as fb
    gl = fb.GradLink()
    y = fb.conv3x3(_x(2, 48, 14, 14), _w(48, 48, 3, 3), gradlink=gl)
    gl.grad = _x(2, 48, 14, 14, grad=False)
    _backward(y)


def _raw(ch):
    def body():
        import torch
        from fluxmpi_amd.ops import fused_block as fb
        with torch.no_grad():
            x, w = _x(2, ch, 14, 14, grad=False), _w(ch, ch, 3, 3).detach()
            y = fb.conv3x3_fwd_raw(x, w)
            fb.conv3x3_dgrad_raw(_x(2, ch, 14, 14, grad=False), w, x.shape, residual=x)
        torch.cuda.synchronize()
        return y
    return body


def _pool():
    from fluxmpi_amd.ops import pool
    bn = _bn(64)
    _backward(pool.bn_relu_maxpool(_x(2, 64, 14, 14), bn))


def _stem():
    import torch
    from fluxmpi_amd.ops import stem
    conv = _bf16(torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False))
    x, bn = _x(1, 3, 224, 224, grad=False), _bn(64)
    assert stem.supported(x, conv.weight, conv, bn)
    _backward(stem.stem(x, conv, bn))


def cases():
    """``(name, body, _isolated arguments)`` of every case."""
    import torch
    from fluxmpi_amd.ops import conv_choice as CC
    from fluxmpi_amd.ops import fused_block as fb
    from fluxmpi_amd.ops import gemm as G
    s14, s7 = (2, 64, 14, 14), (2, 128, 7, 7)
    oa = [((2, 256, 14, 14), 64), (s14, 64), (s14, 256)]
    ob = [(s14, 64), (s14, 256), (s14, 256, 1)]
    oc = [((2, 256, 14, 14), 128), ((2, 128, 14, 14), 128), (s7, 512), ((2, 256, 14, 14), 512, 2)]
    out = []
    for impl in ("hybrid", "fused"):
        for tag, other in (("", {}), ("/other", None)):
            o = lambda keys: dict(other=keys) if other is None else {}
            out += [("a/%s%s" % (impl, tag), _run_block(256, 64, impl=impl), o(oa)),
                    ("b/%s%s" % (impl, tag), _run_block(64, 64, ds=True, impl=impl), o(ob)),
                    ("c/%s%s" % (impl, tag), _run_block(256, 128, 2, True, impl), o(oc))]
            if impl == "hybrid":
                out += [("a/hybrid/conv3bn3=0" + tag, _run_block(256, 64),
                         dict(switches=[(fb, "CONV3BN3", False)], **o(oa)))]
                out += [("b/hybrid/conv3ds=%d%s" % (v, tag), _run_block(64, 64, ds=True),
                         dict(switches=[(fb, "CONV3DS", v)], **o(ob))) for v in (0, 2)]
    out += [
        ("c/hybrid/s2_dgrad", _run_block(256, 128, 2, True), dict(switches=[(G, "S2_DGRAD", True)])),
        ("a/hybrid/w3n", _run_block(256, 64, hw=16), dict(wg={("3x3", (2, 64, 16, 16), 64): ("w3n", CC._W3N_CONFIGS[0])})),
        ("conv1x1/w256", _conv1x1_case(8, 28, 256, 256), dict(wg={("1x1", (8, 256, 28, 28), 256): ("w256", None)})),
        ("ds/w256", _conv1x1_case(8, 28, 256, 256, 1), dict(wg={("ds", (8, 256, 28, 28), 256, 1): ("w256", None)})),
        ("conv1x1_stats/splitk", _conv1x1_stats_splitk, {}),
        ("ds/s2/nolink", _conv1x1_case(2, 14, 256, 512, 2, link=False), {}),
        ("ds/s1/nolink", _conv1x1_case(2, 14, 64, 256, 1, link=False), {}),
        ("e/bnlink1x1", _bnlink_case(1, False), {}),
        ("e/bnlink1x1/res", _bnlink_case(1, True), {}),
        ("e/bnlink3x3", _bnlink_case(3, False), {}),
        ("e/bnlink3x3/res", _bnlink_case(3, True), {}),
        ("e/bnlink3x3/gradlink", _bnlink_case(3, False, True), {}),
        ("conv3x3/c48", _conv3x3_c48, dict(other=[((2, 48, 14, 14), 48)], wgrad="miopen")),
        ("raw/ours", _raw(64), {}),
        ("raw/miopen", _raw(48), dict(other=[((2, 48, 14, 14), 48)], wgrad="miopen")),
        ("f/bn", _bn_case(), {}),
        ("f/bn/relu", _bn_case(relu=True), {}),
        ("f/bn/relu+res", _bn_case(relu=True, res=True), {}),
        ("f/bn/res", _bn_case(res=True), {}),
        ("f/bn/link", _bn_case(relu=True, res=True, link="plain"), {}),
        ("f/bn/masked_link", _bn_case(relu=True, res=True, link="masked"), {}),
        ("f/bn/2d", _bn_case(relu=True, shape=(392, 64)), {}),
        ("f/bn/fp32", _bn_case(relu=True, res=True, dtype=torch.float32), {}),
        ("f/bn/no_affine", _bn_case(relu=True, affine=False, track_running_stats=False), {}),
        ("f/bn/eval", _bn_eval(False), {}),
        ("f/bn/eval+res", _bn_eval(True), {}),
        ("f/sync", _bn_case(relu=True, sync=True), {}),
        ("f/sync/masked_link", _bn_case(relu=True, res=True, link="masked", sync=True), {}),
        ("f/sync/link", _bn_case(relu=True, res=True, link="plain", sync=True), {}),
        ("f/sync/2d", _bn_case(shape=(392, 64), sync=True), {}),
        ("f/sync/no_affine", _bn_case(relu=True, res=True, sync=True, affine=False), {}),
        ("f/sync/ops", _syncbn_ops, {}),
        ("g/pool", _pool, {}),
        ("g/stem", _stem, {}),
    ]
    return out


def _aten_multiset(prof):
    rows = collections.Counter()
    for e in prof.key_averages(group_by_input_shape=True):
        if e.key.startswith("aten::"):
            rows["%s %s" % (e.key, json.dumps(e.input_shapes, separators=(",", ":")))] += e.count
    return dict(sorted(rows.items()))


def trace_all(aten: bool = False, only=None, coverage=None):
    """``{case: [records]}`` (``aten``: ``{case: {"op shapes": count}}``). A case that raises is recorded as
    ``{"error": ...}`` and ends the run (nothing more is started on a GPU that may have faulted). ``coverage``: a dict that receives ``{caller: sorted entries}`` per case."""
    import torch
    out = {}
    for name, body, iso in cases():
        if only and not any(name.startswith(o) for o in only):
            continue
        rec = Recorder()
        torch.manual_seed(0)
        try:
            with _isolated(**iso), recording(rec, vendor=not aten):
                if aten:
                    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU],
                                                record_shapes=True) as prof:
                        body()
                    out[name] = _aten_multiset(prof)
                else:
                    with keep_alive():
                        body()
                    out[name] = rec.records
            failed = False
        except Exception as e:
            out[name], failed = {"error": "%s: %s" % (type(e).__name__, e)}, True
        if coverage is not None:
            by = collections.defaultdict(set)
            for c, r in zip(rec.callers, rec.records):
                by[c].add(r.split("(", 1)[0])
            coverage[name] = {c: sorted(v) for c, v in sorted(by.items())}
        if failed:
            break
    return out


def dumps(result) -> str:
    """The committed form: one record per line, byte for byte reproducible."""
    return json.dumps(result, indent=0, separators=(",", ":")) + "\n"


def compare_aten(a: dict, b: dict):
    """Differences of two ``--aten`` outputs outside ``ATEN_EXCLUDED``: ``[(case, op, count a, count b)]``."""
    diff = []
    for case in sorted(set(a) | set(b)):
        ra, rb = a.get(case, {}), b.get(case, {})
        for k in sorted(set(ra) | set(rb)):
            if k.split(" ", 1)[0] not in ATEN_EXCLUDED and ra.get(k, 0) != rb.get(k, 0):
                diff.append((case, k, ra.get(k, 0), rb.get(k, 0)))
    return diff


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="write the JSON here (default: standard output)")
    ap.add_argument("--aten", action="store_true", help="the ATen side: per case the multiset of (op, input shapes)")
    ap.add_argument("--only", nargs="*", help="case name prefixes")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two outputs (no GPU needed) and exit")
    args = ap.parse_args()
    if args.compare:
        a, b = (json.load(open(p)) for p in args.compare)
        sample = next(iter(a.values()), None)
        if isinstance(sample, dict) and "error" not in sample:
            diff = compare_aten(a, b)
            for case in sorted(a):
                ex = collections.Counter()
                for side, r in (("a", a[case]), ("b", b.get(case, {}))):
                    ex[side] = sum(n for k, n in r.items() if k.split(" ", 1)[0] in ATEN_EXCLUDED)
                print("%-28s excluded (allocations, views): %d vs %d" % (case, ex["a"], ex["b"]))
            for d in diff:
                print("DIFF %s: %s: %d vs %d" % d)
        else:
            diff = [c for c in sorted(set(a) | set(b)) if a.get(c) != b.get(c)]
            for c in diff:
                print("DIFF", c)
        print("equal" if not diff else "%d differences" % len(diff))
        return 1 if diff else 0
    coverage = {}
    result = trace_all(args.aten, args.only, coverage)
    for case, by in coverage.items():
        r = result[case]
        print("== %s: %s" % (case, "%d records" % len(r) if isinstance(r, list) else
                              r["error"] if "error" in r else "%d ops" % sum(r.values())))
        for caller, entries in by.items():
            print("   %-44s %s" % (caller, " ".join(entries)))
    text = dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    bad = [c for c, r in result.items() if isinstance(r, dict) and "error" in r]
    for c in bad:
        print("ERROR %s: %s" % (c, result[c]["error"]), file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
