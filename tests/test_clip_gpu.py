"""Fused gradient clipping on the GPU: the deterministic multi-tensor sum of squares, the clip
arguments of the fused Adam / SGD kernels, the fused clip chains of ``optimisers`` and the DDP
engine's per-leaf (ClipNorm chain) and global (``clip_global_norm``) modes, eager and graphed."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# One call's leaves: 1, 7, 8 elements (below / at one vector), one chunk, one chunk + 1, several
# chunks + a tail, a leaf that starts one element into a larger buffer (not 16-byte aligned: the
# scalar path), one leaf without elements in the MIDDLE, 30 leaves in all (more than the 24 of one
# launch, so the call splits). Standard deviations vary so that some leaves clip and some do not.
SIZES = [1, 7, 8, 4096, 4097, 3 * 4096 + 5, 5000, 33, 100, 257, 1000, 2048, 4095, 63, 0, 64, 65, 511, 513, 9, 15, 16,
         17, 31, 129, 8191, 8193, 3, 5, 12]
UNALIGNED = 6  # index of the offset leaf
OMEGA = 10.0  # randn leaves: norm ~ sqrt(n) * std — below 10 for the small ones, above for the large
GS = 0.5


def _cpu_leaves(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * (0.5 + (i % 3)) for i, n in enumerate(SIZES)]


def _to_dev(leaves, dtype, offset_leaf=True):
    out = []
    for i, t in enumerate(leaves):
        if i == UNALIGNED and offset_leaf:
            buf = torch.zeros(t.numel() + 8, dtype=dtype, device="cuda")
            buf[1:1 + t.numel()].copy_(t.to(dtype))
            v = buf[1:1 + t.numel()]
            assert v.data_ptr() % 16 != 0
            out.append(v)
        else:
            out.append(t.to(dtype).cuda())
    return out


@pytest.fixture(scope="module")
def grads_cpu():
    return _cpu_leaves(0)


def _acc(dt):
    return torch.float64 if dt == torch.float64 else torch.float32


# ---------------------------------------------------------------- 1. sum of squares
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.float64])
def test_sumsq_matches_fp64_and_is_deterministic(gpu_ext, grads_cpu, dtype):
    from fluxmpi_amd.ops import optim
    gs = _to_dev(grads_cpu, dtype)
    assert len(gs) == 30 and gs[14].numel() == 0
    want = optim.sumsq_reference(gs)  # fp64 CPU sums of the values the device holds
    outs = []
    for _ in range(2):
        out = torch.full((len(gs),), -1.0, dtype=_acc(dtype), device="cuda")
        sc = torch.full((len(gs),), -1.0, dtype=_acc(dtype), device="cuda")
        optim.sumsq_(gs, out, scales=sc, omega=OMEGA, grad_scale=GS)
        outs.append((out, sc))
    torch.cuda.synchronize()
    rtol = 1e-12 if dtype == torch.float64 else 1e-5
    print("max rel err", float(((outs[0][0].double().cpu() - want).abs() / want.clamp_min(1e-300)).max()))
    torch.testing.assert_close(outs[0][0].double().cpu(), want, rtol=rtol, atol=0)
    wsc = optim.clip_scales_reference(want, OMEGA, GS)
    torch.testing.assert_close(outs[0][1].double().cpu(), wsc, rtol=rtol, atol=0)
    assert (wsc < 1).any() and (wsc == 1).sum() > 3
    assert outs[0][0][14] == 0 and outs[0][1][14] == 1  # the empty leaf
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_clip_total_accumulates(gpu_ext, grads_cpu):
    from fluxmpi_amd.ops import optim
    gs = _to_dev(grads_cpu, torch.float32)
    out = torch.empty(len(gs), device="cuda")
    optim.sumsq_(gs, out)
    slot = torch.full((3,), 7.0, device="cuda")
    optim.clip_total_(out, slot, omega=3.0, grad_scale=GS)
    total = float(optim.sumsq_reference(gs).sum())
    torch.testing.assert_close(slot.cpu().double(), torch.tensor([total, GS * total ** 0.5, 3.0 / (GS * total ** 0.5)],
                                                                  dtype=torch.float64), rtol=1e-5, atol=0)
    optim.clip_total_(out, slot, accumulate=True)
    torch.testing.assert_close(slot.cpu().double(), torch.tensor([2 * total, (2 * total) ** 0.5, 1.0],
                                                                  dtype=torch.float64), rtol=1e-5, atol=0)


# ---------------------------------------------------------------- 2. clip + update vs the oracle
COMBOS = [
    (torch.float32, torch.float32, torch.float32, False),
    (torch.bfloat16, torch.bfloat16, torch.bfloat16, False),
    (torch.bfloat16, torch.bfloat16, torch.float32, True),
    (torch.float32, torch.bfloat16, torch.float32, False),
    (torch.float64, torch.float64, torch.float64, False),
]
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)


def _tol(dt):
    return dict(rtol=1e-2, atol=1e-3) if dt in (torch.bfloat16, torch.float16) else dict(rtol=1e-5, atol=1e-6)


def _oracle_grads(gs, omega, gscale):
    """Per-leaf scales in fp64 on the CPU, applied to the gradients in fp32 (fp64 for fp64)."""
    from fluxmpi_amd.ops import optim
    sc = optim.clip_scales_reference(optim.sumsq_reference(gs), omega, gscale)
    ct = _acc(gs[0].dtype)
    return [g.cpu().to(ct) * sc[i].to(ct) for i, g in enumerate(gs)], sc


def _fused_scales(gs, omega, gscale):
    from fluxmpi_amd.ops import optim
    buf = torch.empty(2, len(gs), dtype=_acc(gs[0].dtype), device="cuda")
    optim.sumsq_(gs, buf[0], scales=buf[1], omega=omega, grad_scale=gscale)
    return buf[1]


def _compare(got, want, dts):
    for a, b, dt in zip(got, want, dts):
        torch.testing.assert_close(a.cpu().to(_acc(dt)), b.to(_acc(dt)), **_tol(dt))


@pytest.mark.parametrize("pd,gd,sd,master", COMBOS)
def test_fused_clipnorm_adam(gpu_ext, grads_cpu, pd, gd, sd, master):
    from fluxmpi_amd.ops import optim
    P = _cpu_leaves(1)
    p1, g1 = _to_dev(P, pd, offset_leaf=False), _to_dev(grads_cpu, gd)
    m1, v1 = [torch.zeros_like(t, dtype=sd) for t in p1], [torch.zeros_like(t, dtype=sd) for t in p1]
    w1 = [t.float() for t in p1] if master else None
    pc, mc, vc = [t.cpu().clone() for t in p1], [t.cpu().clone() for t in m1], [t.cpu().clone() for t in v1]
    wc = [t.cpu().clone() for t in w1] if master else None
    gc, sc = _oracle_grads(g1, OMEGA, GS)
    assert (sc < 1).any() and (sc == 1).any()
    for t in (1, 2):  # two steps: the second one starts from non-zero moments
        kw = dict(bc1=1 - 0.9 ** t, bc2=1 - 0.999 ** t, **ADAM)
        optim.adam_(p1, g1, m1, v1, masters=w1, grad_scale=GS, tscale=_fused_scales(g1, OMEGA, GS), **kw)
        optim.adam_reference_(pc, gc, mc, vc, masters=wc, grad_scale=GS, **kw)
    torch.cuda.synchronize()
    n = len(p1)
    _compare(m1 + v1 + p1, mc + vc + pc, [sd] * (2 * n) + [pd] * n)
    if master:
        _compare(w1, wc, [torch.float32] * n)


# Descent keeps no state, so it has no (bf16 parameter, fp32 state, master) layout to run in
@pytest.mark.parametrize("pd,gd,sd,master,mom", [(*c, 0.9) for c in COMBOS] + [(*c, 0.0) for c in COMBOS if not c[3]])
def test_fused_clipnorm_sgd(gpu_ext, grads_cpu, pd, gd, sd, master, mom):
    """Descent and Momentum: the scale shows directly in the parameter."""
    from fluxmpi_amd.ops import optim
    P = _cpu_leaves(2)
    p1, g1 = _to_dev(P, pd, offset_leaf=False), _to_dev(grads_cpu, gd)
    b1 = [torch.zeros_like(t, dtype=sd) for t in p1]
    w1 = [t.float() for t in p1] if master else None
    pc, bc = [t.cpu().clone() for t in p1], [t.cpu().clone() for t in b1]
    wc = [t.cpu().clone() for t in w1] if master else None
    gc, _ = _oracle_grads(g1, OMEGA, GS)
    for _ in range(2):
        optim.sgd_(p1, g1, b1, lr=0.1, momentum=mom, masters=w1, grad_scale=GS, tscale=_fused_scales(g1, OMEGA, GS))
        optim.sgd_reference_(pc, gc, bc, lr=0.1, momentum=mom, masters=wc, grad_scale=GS)
    torch.cuda.synchronize()
    n = len(p1)
    _compare(p1 + (b1 if mom else []), pc + (bc if mom else []), [pd] * n + [sd] * n)
    if master:
        _compare(w1, wc, [torch.float32] * n)


# ---------------------------------------------------------------- 3. exactness at scale 1
@pytest.mark.parametrize("pd,gd,sd,master", COMBOS[:3])
def test_scale_one_is_bit_identical(gpu_ext, grads_cpu, pd, gd, sd, master):
    from fluxmpi_amd.ops import optim
    g1 = _to_dev(grads_cpu, gd)
    big = 1e6  # above every leaf's norm, above max|g|
    ts = _fused_scales(g1, big, GS)
    assert bool((ts == 1).all())
    res = []
    for kw in ({}, {"tscale": ts}, {"clip_delta": big}, {"tscale": ts, "clip_delta": big}):
        out = []
        for kind in ("adam", "momentum"):
            p = _to_dev(_cpu_leaves(3), pd, offset_leaf=False)
            m, v = [torch.zeros_like(t, dtype=sd) for t in p], [torch.zeros_like(t, dtype=sd) for t in p]
            w = [t.float() for t in p] if master else None
            for t in (1, 2):
                if kind == "adam":
                    optim.adam_(p, g1, m, v, masters=w, grad_scale=GS, bc1=1 - 0.9 ** t, bc2=1 - 0.999 ** t, **ADAM,
                                **kw)
                else:
                    optim.sgd_(p, g1, m, lr=0.1, momentum=0.9, masters=w, grad_scale=GS, **kw)
            out += p + m + v + (w or [])
        res.append(out)
    torch.cuda.synchronize()
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)


# ---------------------------------------------------------------- 4. edge values
def test_zero_and_nan_leaves(gpu_ext, grads_cpu):
    from fluxmpi_amd.ops import optim
    G = [t.clone() for t in grads_cpu]
    G[3].zero_()  # an all-zero leaf: norm 0 -> scale 1, finite results
    G[5][77] = float("nan")  # one NaN: this leaf's scale, and with it its whole m, is NaN
    g1 = _to_dev(G, torch.float32)
    p1 = _to_dev(_cpu_leaves(4), torch.float32, offset_leaf=False)
    m1, v1 = [torch.zeros_like(t) for t in p1], [torch.zeros_like(t) for t in p1]
    pc, mc, vc = [t.cpu().clone() for t in p1], [t.cpu().clone() for t in m1], [t.cpu().clone() for t in v1]
    gc, sc = _oracle_grads(g1, OMEGA, GS)
    assert sc[3] == 1 and torch.isnan(sc[5])
    ts = _fused_scales(g1, OMEGA, GS)
    kw = dict(bc1=0.1, bc2=0.001, **ADAM)
    optim.adam_(p1, g1, m1, v1, grad_scale=GS, tscale=ts, **kw)
    optim.adam_reference_(pc, gc, mc, vc, grad_scale=GS, **kw)
    torch.cuda.synchronize()
    assert ts[3] == 1 and torch.isnan(ts[5])
    assert torch.isfinite(p1[3]).all() and torch.isfinite(m1[3]).all() and torch.isfinite(v1[3]).all()
    assert torch.isnan(m1[5]).all()
    keep = [i for i in range(len(p1)) if i != 5]
    _compare([x[i] for x in (m1, v1, p1) for i in keep], [x[i] for x in (mc, vc, pc) for i in keep],
             [torch.float32] * (3 * len(keep)))


@pytest.mark.parametrize("kind", ["adam", "descent", "momentum", "nesterov"])
def test_clipgrad_matches_clamp(gpu_ext, grads_cpu, kind):
    """A delta that clamps about half the elements == torch.clamp, then the reference update."""
    from fluxmpi_amd.ops import optim
    g1 = _to_dev(grads_cpu, torch.float32)
    delta = 0.4  # gradients: randn * {0.5, 1.5, 2.5} * GS
    frac = float(torch.cat([(g * GS).abs() > delta for g in g1]).float().mean())
    assert 0.3 < frac < 0.7, frac
    gc = [torch.clamp(g.cpu() * GS, -delta, delta) for g in g1]
    p1 = _to_dev(_cpu_leaves(5), torch.float32, offset_leaf=False)
    m1, v1 = [torch.zeros_like(t) for t in p1], [torch.zeros_like(t) for t in p1]
    pc, mc, vc = [t.cpu().clone() for t in p1], [t.cpu().clone() for t in m1], [t.cpu().clone() for t in v1]
    for t in (1, 2):
        if kind == "adam":
            kw = dict(bc1=1 - 0.9 ** t, bc2=1 - 0.999 ** t, **ADAM)
            optim.adam_(p1, g1, m1, v1, grad_scale=GS, clip_delta=delta, **kw)
            optim.adam_reference_(pc, gc, mc, vc, **kw)
        else:
            kw = dict(lr=0.1, momentum=0.0 if kind == "descent" else 0.9, nesterov=kind == "nesterov")
            optim.sgd_(p1, g1, m1, grad_scale=GS, clip_delta=delta, **kw)
            optim.sgd_reference_(pc, gc, mc, **kw)
    torch.cuda.synchronize()
    _compare(p1 + m1 + v1, pc + mc + vc, [torch.float32] * (3 * len(p1)))


def test_global_scale_sgd(gpu_ext, grads_cpu):
    """``dev_gscale`` of the SGD kernels: one device scalar from clip_total_ (global-norm clip)."""
    from fluxmpi_amd.ops import optim
    g1 = _to_dev(grads_cpu, torch.float32)
    out, slot = torch.empty(len(g1), device="cuda"), torch.zeros(3, device="cuda")
    optim.sumsq_(g1, out)
    optim.clip_total_(out, slot, omega=5.0, grad_scale=GS)
    nrm = GS * float(optim.sumsq_reference(g1).sum()) ** 0.5
    assert nrm > 5.0
    p1 = _to_dev(_cpu_leaves(6), torch.float32, offset_leaf=False)
    pc = [t.cpu().clone() for t in p1]
    optim.sgd_(p1, g1, None, lr=0.1, grad_scale=GS, dev_gscale=slot[2:3])
    optim.sgd_reference_(pc, [g.cpu() * (5.0 / nrm) for g in g1], None, lr=0.1, grad_scale=GS)
    torch.cuda.synchronize()
    _compare(p1, pc, [torch.float32] * len(p1))


# ---------------------------------------------------------------- 5. optimisers.update on GPU leaves
def _chain(name):
    from fluxmpi_amd import optimisers as O
    return {"clipnorm_adam": lambda: O.OptimiserChain(O.ClipNorm(0.5), O.Adam(1e-2)),
            "clipnorm_adamw": lambda: O.OptimiserChain(O.ClipNorm(0.5), O.AdamW(1e-2, decay=0.1)),
            "clipgrad_momentum": lambda: O.OptimiserChain(O.ClipGrad(0.01), O.Momentum())}[name]()


@pytest.mark.parametrize("name", ["clipnorm_adam", "clipnorm_adamw", "clipgrad_momentum"])
def test_optimisers_update_clip_chain_gpu_matches_cpu(gpu_ext, monkeypatch, name):
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.ops import optim
    torch.manual_seed(7)
    ps = {"w": torch.randn(300, 7), "b": torch.randn(7) * 0.01, "e": torch.randn(5000)}
    gs = {"w": torch.randn(300, 7), "b": torch.randn(7) * 0.001, "e": torch.randn(5000) * 0.003}
    st = O.setup(_chain(name), ps)
    psg = {k: v.cuda() for k, v in ps.items()}
    gsg = {k: v.cuda() for k, v in gs.items()}
    stg = O.setup(_chain(name), psg)
    for _ in range(3):
        st, ps = O.update(st, ps, gs)
    # the fused path must run on the GPU leaves: one update launch group per step with the clip
    # inside, and no per-leaf clip expression (the per-leaf fallback would pass the numerics too)
    calls = []
    fn = "sgd_" if name == "clipgrad_momentum" else "adam_"
    real = getattr(optim, fn)

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)

    def boom(*a, **kw):
        raise AssertionError("per-leaf clip ran on GPU leaves")

    monkeypatch.setattr(optim, fn, spy)
    monkeypatch.setattr(O.ClipNorm, "apply", boom)
    monkeypatch.setattr(O.ClipGrad, "apply", boom)
    for _ in range(3):
        stg, psg = O.update(stg, psg, gsg)
    assert len(calls) == 3
    if name == "clipgrad_momentum":
        assert all(abs(kw["clip_delta"] - 0.01) < 1e-8 for kw in calls)
    else:
        assert all(kw["tscale"].is_cuda and kw["tscale"].numel() == 3 for kw in calls)
        sc = calls[-1]["tscale"].cpu()
        assert (sc < 1).any() and (sc == 1).any()
    for k in ps:
        torch.testing.assert_close(psg[k].cpu(), ps[k], rtol=1e-5, atol=1e-6)
    s = stg["w"].state  # the chain's tuple of member states
    assert isinstance(s, tuple) and len(s) == 2 and s[0] is None
    if name == "clipnorm_adamw":
        assert len(s[1]) == 2 and s[1][1] is None and len(s[1][0]) == 3 and s[1][0][0].is_cuda
        assert s[1][0][2] == st["w"].state[1][0][2]
    elif name == "clipnorm_adam":
        assert len(s[1]) == 3 and s[1][2] == st["w"].state[1][2]
    else:
        torch.testing.assert_close(s[1].cpu(), st["w"].state[1], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- 6. engine, world of one
def _mlp(seed, dev="cuda"):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                               torch.nn.Linear(64, 1)).to(dev)


SMALL = dict(bucket_mb=0.004, first_bucket_mb=0.002)


@pytest.fixture
def flux():
    """An initialised runtime (the world-of-one RCCL communicator, shared with the rest of the
    session); the watchdog threads of the test's engines are stopped when it ends."""
    import fluxmpi_amd as FluxMPI
    from fluxmpi_amd.utils.debug import stop_all
    FluxMPI.Init()
    yield FluxMPI
    stop_all()


def _data(seed=21, n=16, target="sin"):
    """Inputs from a CPU generator (the same on every machine). With these models and data the
    per-leaf gradient norms at the first step lie between 0.06 and 0.95 and the global norm
    between 1.2 and 1.6, so the thresholds below (0.2 - 0.3 per leaf, 0.5 global) clip some
    leaves and not others, and the global clip is active."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 32, generator=g)
    y = x.sum(1, keepdim=True).sin() if target == "sin" else torch.randn(n, 1, generator=g)
    return x.cuda(), y.cuda()


def _grads_of(model, ps, x, y):
    for n, p in model.named_parameters():
        p.data.copy_(ps[n])
        p.grad = None
    ((model(x) - y) ** 2).mean().backward()
    return {n: p.grad.clone() for n, p in model.named_parameters()}


def _prescale_global(grads, w):
    nrm = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads.values())))
    s = min(1.0, w / nrm)
    return {n: (g.double() * s).to(g.dtype) for n, g in grads.items()}, nrm


def test_engine_clipnorm_chain_matches_functional(gpu_ext):
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    w = 0.3
    rule = lambda: O.OptimiserChain(O.ClipNorm(w), O.Adam(1e-2))  # noqa: E731
    m1, m2 = _mlp(0), _mlp(0)
    ddp = DDP(m1, rule(), **SMALL)
    assert len(ddp.buckets) > 1
    ps = {n: p.detach().clone() for n, p in m2.named_parameters()}
    st = O.setup(rule(), ps)
    x, y = _data()
    clipped = unclipped = 0
    for _ in range(5):
        ((ddp(x) - y) ** 2).mean().backward()
        ddp.step()
        sc = torch.cat([b.clip[1] for b in ddp.buckets])
        clipped += int((sc < 1).sum())
        unclipped += int((sc == 1).sum())
        grads = _grads_of(m2, ps, x, y)
        nrm = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads.values())))
        torch.testing.assert_close(float(ddp.grad_norm()), nrm, rtol=1e-5, atol=0)
        st, ps = O.update(st, ps, grads)
    assert clipped > 0 and unclipped > 0, (clipped, unclipped)
    for n, p in m1.named_parameters():
        torch.testing.assert_close(p.detach(), ps[n], rtol=1e-5, atol=1e-6)
    leaf = ddp.optimiser_state()["0.weight"]
    assert leaf.state[0] is None and len(leaf.state[1]) == 3 and leaf.state[1][0].shape == (64, 32)
    sd = ddp.state_dict()
    ddp.load_state_dict(sd)


def test_engine_clipnorm_overlap_opt_bitwise(gpu_ext, flux):
    """force_comm + overlap_opt (clip + update behind each bucket's allreduce on the RCCL stream)
    == the updates in step(): bf16 parameters, fp32 masters, several buckets."""
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    x, y = _data(22, 64)
    x = x.bfloat16()
    outs = []
    for ov in (False, True):
        m = _mlp(3).bfloat16()
        d = DDP(m, O.OptimiserChain(O.ClipNorm(0.2), O.Adam(1e-2)), force_comm=True, overlap_opt=ov, average=True,
                **SMALL)
        assert d.overlap_opt == ov and len(d.buckets) > 1
        for _ in range(4):
            ((d(x).float() - y) ** 2).mean().backward()
            d.step()
        torch.cuda.synchronize()
        sc = torch.cat([b.clip[1] for b in d.buckets])
        assert (sc < 1).any() and (sc == 1).any()
        outs.append([p.detach().clone() for p in m.parameters()] + [b.master.clone() for b in d.buckets]
                    + [d.grad_norm().clone()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("rule_name", ["adam", "clipgrad_momentum"])
def test_engine_clip_global_norm(gpu_ext, rule_name):
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    w = 0.5
    inner = (lambda: O.Adam(1e-2)) if rule_name == "adam" else (lambda: O.Momentum(0.05, 0.9))
    delta = 0.004
    rule = inner if rule_name == "adam" else (lambda: O.OptimiserChain(O.ClipGrad(delta), inner()))
    m1, m2 = _mlp(4), _mlp(4)
    ddp = DDP(m1, rule(), clip_global_norm=w, **SMALL)
    assert len(ddp.buckets) > 1 and not ddp.overlap_opt
    ps = {n: p.detach().clone() for n, p in m2.named_parameters()}
    st = O.setup(rule(), ps)  # ClipGrad after the global scale: the chain's own order
    x, y = _data()
    active = 0
    for _ in range(5):
        ((ddp(x) - y) ** 2).mean().backward()
        ddp.step()
        grads, nrm = _prescale_global(_grads_of(m2, ps, x, y), w)
        active += nrm > w
        gn = ddp.grad_norm()
        assert gn.is_cuda and gn.dim() == 0 and gn.dtype == torch.float32
        torch.testing.assert_close(float(gn), nrm, rtol=1e-5, atol=0)
        st, ps = O.update(st, ps, grads)
    assert active > 0
    for n, p in m1.named_parameters():
        torch.testing.assert_close(p.detach(), ps[n], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("mode", ["leaf", "global"])
def test_engine_clips_carried_sum(gpu_ext, flux, mode):
    """step(zero_grad=False), then backward + step: the clip sees S1 + S2."""
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    w = 0.3 if mode == "leaf" else 0.5
    m1, m2 = _mlp(5), _mlp(5)
    if mode == "leaf":
        ddp = DDP(m1, O.OptimiserChain(O.ClipNorm(w), O.Descent(0.1)), force_comm=True, **SMALL)
    else:
        ddp = DDP(m1, O.Descent(0.1), clip_global_norm=w, force_comm=True, **SMALL)
    x, y = _data()
    ps = {n: p.detach().clone() for n, p in m2.named_parameters()}

    def clip(grads):
        if mode == "global":
            return _prescale_global(grads, w)[0]
        return {n: (g.double() * min(1.0, w / float(g.double().norm()))).float() for n, g in grads.items()}

    ((ddp(x) - y) ** 2).mean().backward()
    ddp.step(zero_grad=False)
    s1 = _grads_of(m2, ps, x, y)
    ps = {n: ps[n] - 0.1 * g for n, g in clip(s1).items()}
    ((ddp(x) - y) ** 2).mean().backward()
    ddp.step()
    s2 = _grads_of(m2, ps, x, y)
    both = {n: s1[n] + s2[n] for n in s1}
    nrm = float(torch.sqrt(sum(g.double().pow(2).sum() for g in both.values())))
    torch.testing.assert_close(float(ddp.grad_norm()), nrm, rtol=1e-5, atol=0)
    ps = {n: ps[n] - 0.1 * g for n, g in clip(both).items()}
    for n, p in m1.named_parameters():
        torch.testing.assert_close(p.detach(), ps[n], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("mode", ["leaf", "global"])
def test_graphed_clipped_step_matches_eager(gpu_ext, mode):
    import torch.nn.functional as F
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    from fluxmpi_amd.parallel.graph import GraphedStep

    def make(m):
        if mode == "leaf":
            return DDP(m, O.OptimiserChain(O.ClipNorm(0.2), O.Adam(1e-2)), **SMALL)
        return DDP(m, O.Adam(1e-2), clip_global_norm=0.5, **SMALL)

    m1, m2 = _mlp(1), _mlp(1)
    d1, d2 = make(m1), make(m2)
    x, y = _data(23, 16, target="randn")

    def loss_fn(d, xx, yy):
        return F.mse_loss(d(xx), yy)

    g = GraphedStep(d1, loss_fn, x, y, warmup=2)
    for _ in range(2):
        loss_fn(d2, x, y).backward()
        d2.step()
    for _ in range(4):
        g(x, y)
        loss_fn(d2, x, y).backward()
        d2.step()
    torch.cuda.synchronize()
    assert float(d2.grad_norm()) > 0.5  # the clip is active
    torch.testing.assert_close(d1.grad_norm(), d2.grad_norm(), rtol=1e-5, atol=0)
    for p, q in zip(m1.parameters(), m2.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-5, atol=1e-6)


def test_engine_clip_argument_errors(gpu_ext):
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    with pytest.raises(ValueError):
        DDP(_mlp(6), O.Adam(), clip_global_norm=1.0, overlap_opt=True)
    with pytest.raises(ValueError):
        DDP(_mlp(6), O.OptimiserChain(O.ClipNorm(1.0), O.Adam()), clip_global_norm=1.0)
