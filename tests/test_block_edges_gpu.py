"""Stage-wise per-element checks of one ResNet bottleneck on every route of ``Bottleneck.forward``
(``models/resnet.py``) through ``ops/fused_block.py``: a recorder keeps what every public entry point
took, returned and received as gradients, and the checker of ``block_edges.py`` (read its docstring for the
references and the derivation of every bound) holds each stage to its own bound, starting from the bf16
values the device stored for the stage's inputs.

Routes are forced, never the autotuner's pick: the ``*_forward_is_ours`` choices, ``conv_choice.WGRAD``
("ours": our filter-gradient kernels, held to the bound; "miopen": not held), ``BN2CONV3``, ``CONV3BN3``,
``CONV3DS``, ``DUAL_BN``, ``DS_FWD``, ``masked_links_ok`` and a block input without gradient. Every case
asserts the exact list of entry points seen, so a silent fall-back fails. ``conv3bn3_admits`` is patched
to drop ONLY its pixels-per-compute-unit term (a speed gate: nobody has timed the 128 -> 512 one-pass
kernel at few pixels), so that node is reached at 300 pixels; no dtype, layout, alignment or channel
predicate is patched. ``bn2conv3_ok`` has the same gate inside, unpatchable on its own: those routes run at
3 x 74 x 74 (stride 2: 3 x 148 x 148; 16428 pixels >= 64 x 256 compute units after conv2, not a multiple of
32), for the four kinds it admits (64- and 128-wide). The stride-2 one, whose input has 65712 pixels, is the
slowest case of the file: 2.3 s in the MI355X run of the table below, most of it the float64 references and
bounds. ``slabs=4``: the one-pass nodes with 4 workgroups for 10 tiles, so the persistent loop wraps. An arm
that a block kind cannot reach is skipped with the reason.

Exact case (``test_conv3_exact``): ternary a2, W3 and incoming gradient substituted at the recorder boundary
on a route that stores a2; c3, d_a2 and dW3 must equal the float64 results.

Worst |err| / bound per stage over the 139 GPU tests (MI355X, 2026-11-26): 136 single blocks, two two-block
tests whose blocks count separately (140 blocks walked), and the exact case, which has no ratio. A ratio
above 1 fails; every case prints its own as ``RATIO <kind> [<route>] <stage>: <ratio>``. A correctly rounded
bf16 store alone reaches 0.99 of its u |ref| term, so these are the ratios of tight bounds, met:

    stage          worst   blocks worst case
    conv1          0.988   140    64-64-s1-ds  [bn2conv3, big]          (forward, filter and block-input gradient)
    bn1            0.996   140    1024-512-s2-ds [impl=fused, dual=False]
    ds             0.991    55    64-64-s1-ds  [bn2conv3, conv3bn3=0, conv3ds=0, big]
    bn_ds          0.995     8    1024-512-s2-ds [dual=False]
    conv2          0.992   122    512-256-s2-ds [ours1=False, o3=True]
    bn2            0.995    91    1024-256-s1-id [default]
    bn2+conv3fwd   0.995     7    256-64-s1-id [bn2conv3, big]          (bn_relu_conv3)
    bn2+conv3      0.812    42    1024-512-s2-ds [impl=fused]           (bn_relu_conv1x1, composed bounds)
    conv3          0.993    62    1024-512-s2-ds [ours1=False, o3=True]
    bn3            0.996    54    256-64-s1-id [bn2conv3, conv3bn3=0, conv3ds=0, big]
    bn3+bn_ds      0.996    50    64-64-s1-ds  [bn2conv3, conv3bn3=0, conv3ds=0, big]   (dual_bn_relu)
    conv3+bn3      0.995    21    256-64-s1-id [bn2conv3, big]          (conv3_bn3_relu, composed bounds)
    conv3+ds+bn3   0.994    15    64-64-s1-ds  [default]                (conv3ds_bn_relu, composed bounds)
"""
import pytest
import torch

from . import block_edges as B

gpu = pytest.mark.gpu

ROUTES = [
    dict(),
    dict(ours1=False, ours3=False, ours3s2=False, ds_ours=False, wgrad="miopen"),
    dict(ours1=False),               # conv1 and conv3 on MIOpen, everything else ours: two statistics passes
    dict(ours1=False, o3=True),      # the per-shape choice differs: bn1 runs its own pass, bn3's sums are pending
    dict(o3=False),                  # ... and the other way round
    dict(ours3=False, ours3s2=False),  # only conv2 on MIOpen: bn2 runs its pass between two pending producers
    dict(conv3bn3=0, conv3ds=0),
    dict(conv3bn3=1),
    dict(conv3ds=2),
    dict(dual=False),
    dict(ds_fwd="force"),
    dict(ds_fwd="miopen"),
    dict(masked=False),
    dict(needs=False),
    dict(bn2conv3=True, big=True),
    dict(bn2conv3=True, big=True, conv3bn3=0, conv3ds=0),
    dict(slabs=4),
    dict(slabs=4, conv3ds=2),
    dict(impl="fused"),
    dict(impl="fused", ours3=False, ds_ours=False),
    dict(impl="fused", dual=False),
    dict(impl="fused", needs=False),
    dict(impl="fused", masked=False),
]


def unreachable(kind, kw):
    """Why the arm ``kw`` is no arm of its own for this block kind (None: it is one)."""
    cin, width, stride, ds = kind
    hy = kw.get("impl", "hybrid") == "hybrid"
    one_pass_id = hy and not ds and width in (64, 128)
    c3ds = hy and kind == B.KINDS[0]
    why = {
        "ours3": stride != 1 and "no stride-1 3x3",
        "ours3s2": not (stride == 2 and hy) and "no stride-2 3x3 on our kernels",
        "ds_ours": not ds and "no downsample", "ds_fwd": not ds and "no downsample", "dual": not ds and "no downsample",
        "conv3ds": not c3ds and "conv3ds_ok: only the 64 -> 64 -> 256 stride-1 downsample block",
        "conv3bn3": (not one_pass_id and "conv3bn3_ok: only 64 -> 256 and 128 -> 512 identity blocks")
        or (kw.get("conv3bn3") == 1 and width == 64 and "CONV3BN3=1 is CONV3BN3=2 for 64 -> 256"),
        "masked": ds and "no GradLink in a downsample block",
        "bn2conv3": not (hy and width in (64, 128)) and "bn2conv3_ok: only 64 -> 256 and 128 -> 512",
        "big": not (hy and width in (64, 128)) and "only with bn2conv3",
        "slabs": not (one_pass_id or c3ds) and "no one-pass node",
    }
    for k in ("bn2conv3", "big", "slabs") + (("conv3ds",) if "slabs" in kw else ()):  # the arm is about these
        if k in kw and why[k]:
            return f"{k}: {why[k]}"
    dead = [k for k in kw if why.get(k)]
    rest = {k: v for k, v in kw.items() if k not in dead}
    if dead and rest in ROUTES:  # without the switches that do nothing here it is another route of the matrix
        return "; ".join(f"{k}: {why[k]}" for k in dead) + f" (the arm of {rest or 'the default route'})"
    return None


def split(kw):
    kw = dict(kw)
    slabs = kw.pop("slabs", None)
    return B.route(**kw), slabs


CASES = [(k, kw, "uniform") for kw in ROUTES for k in B.KINDS] + \
        [(k, kw, "cancel") for kw in (dict(), dict(impl="fused")) for k in B.KINDS]
IDS = [f"{B.kind_id(k)}-{B.route_id(split(kw)[0])}{'-slabs' if 'slabs' in kw else ''}-{f}" for k, kw, f in CASES]


# ------------------------------------------------------------------------------- CPU: the oracle itself

@pytest.mark.parametrize("kind,kw,family", CASES, ids=IDS)
def test_oracle_accepts_emulation_cpu(kind, kw, family):
    """The checker passes on the float32 emulation of every block kind and route, and at most 1e-3 of
    any ReLU is undecided: the cap is met by the reference alone."""
    if unreachable(kind, kw):
        pytest.skip(unreachable(kind, kw))
    r, _ = split(kw)
    rec = B.emulate(kind, r, B.make_inputs(kind, family, r["big"]))
    w = B.Walk(kind, r).run(rec)
    assert not w.errs, "\n".join(w.errs)
    assert w.und and all(v <= B.N.UNDECIDED_CAP for v in w.und.values()), w.und


# defect -> (kind, route, the stage whose check must fail)
PLANTED = {
    "res_missing_last_tile": (B.KINDS[1], dict(), "conv1"),
    "res_twice": (B.KINDS[0], dict(conv3ds=0), "conv1"),
    "stats_swapped": (B.KINDS[2], dict(), "bn3+bn_ds"),
    "sums_swapped_bwd": (B.KINDS[2], dict(), "bn3+bn_ds"),
    "mask_shifted": (B.KINDS[3], dict(conv3bn3=0), "bn3"),
    "dbeta_32_63_zero": (B.KINDS[1], dict(), "conv3+bn3"),
    "biased_running_var": (B.KINDS[5], dict(), "bn3"),
    "c3_recomputed": (B.KINDS[1], dict(bn2conv3=True, big=True), "conv3+bn3"),
    "wgrad_slab_omitted": (B.KINDS[0], dict(), "conv3+ds+bn3"),
}


@pytest.mark.parametrize("defect", B.DEFECTS)
def test_planted_defects_fail_cpu(defect):
    """Every planted defect fails, first at the stage it was planted in, with an error naming that stage."""
    kind, kw, stage = PLANTED[defect]
    r = B.route(**kw)
    w = B.Walk(kind, r).run(B.emulate(kind, r, B.make_inputs(kind, "uniform", r["big"]), defect))
    assert w.errs, f"{defect}: not noticed"
    assert w.errs[0].startswith(stage + " "), f"{defect}: expected the first failure at {stage}:\n" + "\n".join(w.errs)


def test_plan_matches_defect_table_cpu():
    assert set(PLANTED) == set(B.DEFECTS)
    for defect, (kind, kw, stage) in PLANTED.items():
        assert stage in [st for _, st in B.plan(kind, B.route(**kw))], defect


# ------------------------------------------------------------------------------- GPU

def _block(kind, r, inp):
    from fluxmpi_amd.models.resnet import Bottleneck, _norm, conv1x1
    cin, width, stride, ds = kind
    cout = 4 * width
    down = torch.nn.Sequential(conv1x1(cin, cout, stride, "miopen"), _norm(cout, "fused")) if ds else None
    blk = Bottleneck(cin, width, stride, down, r["impl"]).cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)
    pairs = [(blk.bn1, "bn1"), (blk.bn2, "bn2"), (blk.bn3, "bn3")] + ([(down[1], "bn_ds")] if ds else [])
    with torch.no_grad():
        for bn, key in pairs:
            bn.float()
            bn.weight.copy_(inp[key]["w"])
            bn.bias.copy_(inp[key]["b"])
        for conv, key in [(blk.conv1, "w1"), (blk.conv2, "w2"), (blk.conv3, "w3")] + ([(down[0], "wds")] if ds else []):
            conv.weight.copy_(inp[key])
    return blk.train()


def _force(mp, r, slabs):
    from fluxmpi_amd.ops import conv_choice as cc
    from fluxmpi_amd.ops import fused_block as fb
    # conv1's filter has `width` output channels, conv3's four times that: the per-shape choice may differ
    mp.setattr(fb, "conv1x1_forward_is_ours", lambda x, w: r["ours1"] if w.shape[0] <= w.shape[1] else B.o3_of(r))
    mp.setattr(fb, "conv3x3_forward_is_ours", lambda x, w: r["ours3"])
    mp.setattr(fb, "conv3x3_s2_forward_is_ours", lambda x, w: r["ours3s2"])
    if r["ds_fwd"] == "ours":  # ("force" / "miopen": the function's own answer, no measurement)
        supported = fb.ds_forward_supported
        mp.setattr(fb, "ds_forward_is_ours", lambda x, w, s: r["ds_ours"] and supported(x, w, s))
    for name, v in (("DS_FWD", r["ds_fwd"]), ("BN2CONV3", r["bn2conv3"]), ("CONV3BN3", r["conv3bn3"]),
                    ("CONV3DS", r["conv3ds"]), ("DUAL_BN", r["dual"])):
        mp.setattr(fb, name, v)
    capable = fb.masked_links_ok  # (a capability of the GEMM engine: never forced on)
    mp.setattr(fb, "masked_links_ok", lambda: r["masked"] and capable())
    mp.setattr(cc, "WGRAD", r["wgrad"])
    mp.setattr(cc, "_WG_CHOICE", {})
    # the speed gate only (pixels >= 64 x compute units for 128 -> 512): shapes and the switch as in fused_block
    mp.setattr(fb, "conv3bn3_admits", lambda fs, pixels, cus: (tuple(fs) == (256, 64, 1, 1) and fb.CONV3BN3 >= 1)
               or (tuple(fs) == (512, 128, 1, 1) and fb.CONV3BN3 >= 2))
    if slabs:
        mp.setattr(fb, "conv3bn3_slabs", lambda rows, device, cout=256: slabs)
        mp.setattr(fb, "conv3ds_slabs", lambda rows, device: slabs)


def _nhwc(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _workspaces_clean():
    from fluxmpi_amd.ops import batchnorm as bnm
    torch.cuda.synchronize()
    return all(float(ws.abs().max()) == 0.0 for pool in (bnm._WS, bnm._LWS, bnm._DWS) for ws in pool.values())


def _run(blocks, x0, dy, needs):
    """One forward and one backward through ``blocks`` under the recorder; returns (record, links, the leaf)."""
    xl = _nhwc(x0).requires_grad_(needs)
    with B.Recorder() as rec:
        out = xl * 1 if needs else xl  # the block input is a non-leaf, as in a network
        for blk in blocks:
            out = blk(out)
        out.backward(_nhwc(dy))
        torch.cuda.synchronize()
        record = rec.finish()
    return record, rec.links, xl


@gpu
@pytest.mark.parametrize("kind,kw,family", CASES, ids=IDS)
def test_block_stagewise(gpu_ext, monkeypatch, kind, kw, family):
    if unreachable(kind, kw):
        pytest.skip(unreachable(kind, kw))
    r, slabs = split(kw)
    _force(monkeypatch, r, slabs)
    inp = B.make_inputs(kind, family, r["big"])
    record, links, xl = _run([_block(kind, r, inp)], inp["x"], inp["dy"], r["needs"])
    w = B.Walk(kind, r).run(record)
    errs = list(w.errs)
    if not r["needs"] and xl.grad is not None:
        errs.append("conv1 block-input: a gradient arrived at an input that needs none")
    errs += [f"link: a {type(l).__name__} was left unconsumed" for l in links if l.grad is not None]
    if not _workspaces_clean():
        errs.append("workspace: a statistics workspace was left non-zero after the block")
    assert not errs, "\n".join(errs)
    assert all(v <= B.N.UNDECIDED_CAP for v in w.und.values()), w.und


@gpu
@pytest.mark.parametrize("impl", ["hybrid", "fused"])
def test_two_consecutive_blocks(gpu_ext, monkeypatch, impl):
    """layer1.0 then layer1.1 as ``ResNet._make`` builds them: both checked stage-wise; the statistics
    workspaces are clean afterwards, and the identity block's link reaches the gradient of the first
    block's output (that gradient is the second block's block-input gradient, checked there, and the
    first block's backward starts from it)."""
    r = B.route(impl=impl)
    _force(monkeypatch, r, None)
    ka, kb = B.KINDS[0], B.KINDS[1]
    ia, ib = B.make_inputs(ka, "uniform"), B.make_inputs(kb, "uniform", seed=1)
    record, links, _ = _run([_block(ka, r, ia), _block(kb, r, ib)], ia["x"], ib["dy"], True)
    na = len(B.plan(ka, r))
    wa, wb = B.Walk(ka, r).run(record[:na]), B.Walk(kb, r).run(record[na:])
    errs = [f"block 0: {e}" for e in wa.errs] + [f"block 1: {e}" for e in wb.errs]
    errs += [f"link: a {type(l).__name__} was left unconsumed" for l in links if l.grad is not None]
    if not _workspaces_clean():
        errs.append("workspace: a statistics workspace was left non-zero after the blocks")
    assert not errs, "\n".join(errs)
    assert all(v <= B.N.UNDECIDED_CAP for w in (wa, wb) for v in w.und.values()), (wa.und, wb.und)


@gpu
def test_conv3_exact(gpu_ext, monkeypatch):
    """The 256 -> 64 -> 256 identity block with ``CONV3BN3=0`` stores a2 and runs conv3 as ``conv1x1_hybrid``.
    Between ``Bottleneck.forward`` and the recorder, conv3's a2 and W3 are replaced by ternary tensors and the
    gradient arriving at c3 by a ternary one: forward, input gradient and filter gradient are sums of at most
    75 terms +-1 and must equal the float64 results. (The block input takes no gradient: with a2 replaced,
    nothing upstream of conv3 is differentiated, and a GradLink would stay unconsumed.)"""
    from fluxmpi_amd.ops import fused_block as fb
    kind, r = B.KINDS[1], B.route(conv3bn3=0, needs=False)
    _force(monkeypatch, r, None)
    inp = B.make_inputs(kind, "uniform")
    n, _, h, _ = inp["x"].shape
    dy, a2, w3 = B.exact_operands(n * h * h, 4 * kind[1], kind[1])
    blk = _block(kind, r, inp)
    calls, shipped = [], fb.conv1x1_hybrid
    with B.Recorder() as rec:
        recorded = fb.conv1x1_hybrid

        def substitute(x, weight, *a, **k):
            calls.append(1)
            if len(calls) != 2:  # conv1
                return recorded(x, weight, *a, **k)
            xs = _nhwc(B.unrows(a2, n, h, h)).requires_grad_(True)
            ws = w3.view_as(weight).cuda().requires_grad_(True)
            c3 = recorded(xs, ws, *a, **k)
            out = c3.view_as(c3)
            out.register_hook(lambda g: _nhwc(B.unrows(dy, n, h, h)))  # replaces the gradient that reaches c3
            return out

        fb.conv1x1_hybrid = substitute  # (not monkeypatch: its undo would outlive the recorder's and re-install `recorded`)
        try:
            blk(_nhwc(inp["x"])).backward(_nhwc(inp["dy"]))
            torch.cuda.synchronize()
            record = rec.finish()
        finally:
            fb.conv1x1_hybrid = recorded
    assert fb.conv1x1_hybrid is shipped, "the entry point must be the shipped function again"
    assert [e["name"] for e in record] == [nm for nm, _ in B.plan(kind, r)]
    errs = []
    B.exact_conv3(record[-2]["t"], errs)
    assert not errs, "\n".join(errs)
