"""The fused kernels of the rule set beyond Adam and SGD (``csrc/kernels/optim_rules.hip``) on the
GPU: every rule against ``ops.optim.rule_reference_`` over the dtype combinations, the clip
prologue, the functional API on GPU leaves and the DDP engine (eager, overlapped, graphed,
checkpointed)."""
import pytest
import torch

from tests.test_clip_gpu import COMBOS, SIZES, UNALIGNED, _acc, _tol

pytestmark = pytest.mark.gpu

KINDS = ["rmsprop", "adagrad", "lion", "adamax", "amsgrad", "nadam", "adabelief", "adadelta"]
NEW = KINDS[2:]
ALL_COMBOS = COMBOS + [(torch.float16, torch.float16, torch.float32, True)]
CANARY = 77.0
GRAD_ONLY = 4  # a second leaf whose gradient alone misses 16-byte alignment
HYPER = {
    "rmsprop": dict(lr=1e-3, rho=0.9, eps=1e-8),
    "adagrad": dict(lr=0.1, eps=1e-8),
    "lion": dict(lr=1e-3, beta1=0.9, beta2=0.99),
    "adamax": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8),
    "amsgrad": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8),
    "nadam": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8),
    "adabelief": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-16),
    "adadelta": dict(rho=0.9, eps=1e-7),
}


def _rules():
    from fluxmpi_amd import optimisers as O
    return {"rmsprop": O.RMSProp, "adagrad": O.AdaGrad, "lion": O.Lion, "adamax": O.AdaMax, "amsgrad": O.AMSGrad,
            "nadam": O.NAdam, "adabelief": O.AdaBelief, "adadelta": O.AdaDelta}


def _cpu_leaves(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * (0.5 + (i % 3)) * scale for i, n in enumerate(SIZES)]


_CACHE: dict = {}


def _leaves(seed, scale=1.0):
    """CPU leaves, computed once per (seed, scale) and never changed."""
    key = (seed, scale)
    if key not in _CACHE:
        _CACHE[key] = _cpu_leaves(seed, scale)
    return _CACHE[key]


class Guarded:
    """Device copies of CPU leaves, each in a buffer of its own with 8 extra elements holding a
    canary (and, for an offset leaf, one canary element in front)."""

    def __init__(self, leaves, dtype, offset=()):
        self.bufs, self.views, self.spans = [], [], []
        for i, t in enumerate(leaves):
            o = 1 if i in offset else 0
            buf = torch.full((t.numel() + 8 + o,), CANARY, dtype=dtype, device="cuda")
            buf[o:o + t.numel()].copy_(t.to(dtype))
            v = buf[o:o + t.numel()]
            if o and t.numel():
                assert v.data_ptr() % 16 != 0
            self.bufs.append(buf)
            self.views.append(v)
            self.spans.append((o, t.numel()))

    def check(self):
        for buf, (o, n) in zip(self.bufs, self.spans):
            assert bool((buf[:o] == CANARY).all()) and bool((buf[o + n:] == CANARY).all()), "write past a leaf"

    def update(self, leaves):
        for v, t in zip(self.views, leaves):
            v.copy_(t.to(v.dtype))


def _init_states(kind, ns, sd, n_leaves):
    """fp32 / fp64 states: the rule's own initial state (3 steps follow). bf16 / fp16 states: positive
    non-trivial values rounded to the state dtype, identical on both sides (one step follows)."""
    out = []
    for k in range(ns):
        if sd in (torch.float32, torch.float64):
            fill = HYPER[kind]["eps"] if kind in ("adagrad", "amsgrad") else 0.0
            out.append([torch.full((n,), fill, dtype=sd) for n in SIZES])
        else:
            out.append([t.abs().mul(0.1).to(sd) for t in _leaves(40 + k)])
    return out


@pytest.mark.parametrize("pd,gd,sd,master", ALL_COMBOS)
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_matches_reference(gpu_ext, kind, pd, gd, sd, master):
    from fluxmpi_amd.ops import optim
    _, ns, has_bt = optim.RULES[kind]
    hyper = HYPER[kind]
    off_all, off_g = (UNALIGNED,), (UNALIGNED, GRAD_ONLY)
    P = Guarded(_leaves(1), pd, off_all)
    G = Guarded(_leaves(0), gd, off_g)
    st_cpu = _init_states(kind, ns, sd, len(SIZES))
    S = [Guarded(s, sd, off_all) for s in st_cpu]
    W = Guarded([v.cpu().float() for v in P.views], torch.float32, off_all) if master else None
    assert len(P.views) == 30 and P.views[14].numel() == 0
    pc = [v.cpu().clone() for v in P.views]
    sc = [[t.clone() for t in s] for s in st_cpu]
    wc = [v.cpu().clone() for v in W.views] if master else None
    steps = 3 if sd in (torch.float32, torch.float64) else 1
    b1, b2 = hyper.get("beta1", 0.0), hyper.get("beta2", 0.0)
    excluded = total = 0
    for t in range(1, steps + 1):
        if t > 1:
            G.update(_leaves(10 + t))  # fresh gradients
        gc = [v.cpu().clone() for v in G.views]
        kw = dict(bt1=b1 ** t, bt2=b2 ** t, weight_decay=0.01, grad_scale=0.5, **hyper) if has_bt else \
            dict(weight_decay=0.01, grad_scale=0.5, **hyper)
        if kind == "lion":
            # elements whose sign argument is within rounding of zero are left out (see below)
            ct = _acc(pd)
            args = [sc[0][i].to(ct) * b1 + (1 - b1) * (gc[i].to(ct) * 0.5) for i in range(len(gc))]
            near = [a.abs() < 1e-5 for a in args] if t == 1 else [n | (a.abs() < 1e-5) for n, a in zip(near, args)]
        optim.rule_(kind, P.views, G.views, [s.views for s in S], masters=W.views if master else None, **kw)
        optim.rule_reference_(kind, pc, gc, sc, masters=wc, **kw)
    torch.cuda.synchronize()
    for guard in [P, G, *S] + ([W] if master else []):
        guard.check()

    def compare(got, want, dt, mask=None):
        for i, (a, b) in enumerate(zip(got, want)):
            a, b = a.cpu().to(_acc(dt)), b.to(_acc(dt))
            if mask is not None:
                a, b = a[~mask[i]], b[~mask[i]]
            torch.testing.assert_close(a, b, **_tol(dt))

    for s, c in zip(S, sc):
        compare(s.views, c, sd)
    mask = None
    if kind == "lion":
        # a sign flip moves the parameter by 2·lr: only elements whose argument is further from zero
        # than its rounding (about 1e-7 in fp32) are compared; they must be all but 0.1 %
        mask = near
        excluded, total = sum(int(n.sum()) for n in near), sum(SIZES)
        print(f"lion: {excluded} of {total} elements left out")
        assert excluded <= 1e-3 * total
    compare(P.views, pc, pd, mask)
    if master:
        compare(W.views, wc, torch.float32, mask)


# ---------------------------------------------------------------- clip prologue
def _run(kind, g_dev, seed=3, **kw):
    from fluxmpi_amd.ops import optim
    ns = optim.RULES[kind][1]
    p = [t.cuda() for t in _leaves(seed)]
    fill = HYPER[kind]["eps"] if kind == "amsgrad" else 0.0
    st = [[torch.full_like(t, fill) for t in p] for _ in range(ns)]
    for t in (1, 2):
        optim.rule_(kind, p, g_dev, st, bt1=0.9 ** t, bt2=0.999 ** t, **HYPER[kind], **kw)
    return p, st


def _run_ref(kind, g_cpu, seed=3, **kw):
    from fluxmpi_amd.ops import optim
    ns = optim.RULES[kind][1]
    p = [t.clone() for t in _leaves(seed)]
    fill = HYPER[kind]["eps"] if kind == "amsgrad" else 0.0
    st = [[torch.full_like(t, fill) for t in p] for _ in range(ns)]
    for t in (1, 2):
        optim.rule_reference_(kind, p, g_cpu, st, bt1=0.9 ** t, bt2=0.999 ** t, **HYPER[kind], **kw)
    return p, st


def _close(got, want, kind):
    gp, gs = got
    wp, ws = want
    torch.cuda.synchronize()
    for a, b in zip([t for s in gs for t in s], [t for s in ws for t in s]):
        torch.testing.assert_close(a.cpu(), b, **_tol(torch.float32))
    bad = sum(int((~torch.isclose(a.cpu(), b, **_tol(torch.float32))).sum()) for a, b in zip(gp, wp))
    # Lion: an argument within rounding of zero may take the other sign (see the kernel test)
    assert bad <= (1e-3 * sum(SIZES) if kind == "lion" else 0), bad


@pytest.mark.parametrize("kind", ["lion", "amsgrad"])
@pytest.mark.parametrize("arg", ["tscale", "clip_delta", "dev_gscale", "grad_scale"])
def test_clip_prologue(gpu_ext, kind, arg):
    """Each clip argument == the reference applied to gradients clipped beforehand."""
    g_cpu = _leaves(0)
    g_dev = [t.cuda() for t in g_cpu]
    if arg == "tscale":
        sc = torch.linspace(0.1, 1.0, len(SIZES))
        got = _run(kind, g_dev, tscale=sc.cuda())
        want = _run_ref(kind, [g * s for g, s in zip(g_cpu, sc)])
    elif arg == "clip_delta":
        frac = float(torch.cat([g.abs() > 0.8 for g in g_cpu]).float().mean())
        assert 0.3 < frac < 0.7, frac
        got = _run(kind, g_dev, clip_delta=0.8)
        want = _run_ref(kind, [torch.clamp(g, -0.8, 0.8) for g in g_cpu])
    elif arg == "dev_gscale":
        got = _run(kind, g_dev, dev_gscale=torch.tensor([0.25], device="cuda"))
        want = _run_ref(kind, [g * 0.25 for g in g_cpu])
    else:
        got = _run(kind, g_dev, grad_scale=0.25)
        want = _run_ref(kind, [g * 0.25 for g in g_cpu])
    _close(got, want, kind)
    plain = _run(kind, g_dev)
    torch.cuda.synchronize()
    # the argument did something (in the state: Lion's parameters do not see a positive scale)
    assert any(not torch.equal(a, b) for a, b in zip(plain[1][0], got[1][0]))


@pytest.mark.parametrize("kind", ["lion", "amsgrad"])
def test_unit_scales_are_bit_identical(gpu_ext, kind):
    g_dev = [t.cuda() for t in _leaves(0)]
    base = _run(kind, g_dev)
    for kw in ({"tscale": torch.ones(len(SIZES), device="cuda")}, {"dev_gscale": torch.ones(1, device="cuda")}):
        other = _run(kind, g_dev, **kw)
        torch.cuda.synchronize()
        for a, b in zip(base[0] + [t for s in base[1] for t in s], other[0] + [t for s in other[1] for t in s]):
            assert torch.equal(a, b)


def test_rule_argument_errors(gpu_ext):
    from fluxmpi_amd.ops import optim
    p, g = [torch.zeros(8, device="cuda")], [torch.zeros(8, device="cuda")]
    with pytest.raises(ValueError):
        optim.rule_("amsgrad", p, g, [[torch.zeros(8, device="cuda")]] * 2)  # three states needed
    with pytest.raises(TypeError):
        optim.rule_("lion", p, g, [[torch.zeros(4, device="cuda")]])  # a state shorter than its parameter
    with pytest.raises(TypeError):
        optim.rule_("lion", p, g, [[torch.zeros(8, device="cuda", dtype=torch.float64)]])  # no such kernel
    with pytest.raises(RuntimeError):
        gpu_ext.mt_rule(2, [p[0].data_ptr()], [g[0].data_ptr()], [], [], [], [], [8], 7, 7, 7, 1e-3, 0.9, 0.99, 0.0,
                        0.0, 0.0, 0.0, 1.0, 0, 0, 0, 0.0, 0)  # the native entry refuses a missing state list


# ---------------------------------------------------------------- optimisers.update on GPU leaves
def _functional_rule(name):
    from fluxmpi_amd import optimisers as O
    R = _rules()
    if name in R:
        return R[name](**({"eta": 1e-2} if name != "adadelta" else {}))
    inner = {"lion": lambda: O.Lion(1e-2), "nadam": lambda: O.NAdam(1e-2)}[name.split("_")[1]]
    return {"decay": lambda: O.OptimiserChain(inner(), O.WeightDecay(0.1)),
            "clipnorm": lambda: O.OptimiserChain(O.ClipNorm(0.5), inner()),
            "clipnormdecay": lambda: O.OptimiserChain(O.ClipNorm(0.5), O.OptimiserChain(inner(), O.WeightDecay(0.1))),
            "flat": lambda: O.OptimiserChain(O.ClipNorm(0.5), inner(), O.WeightDecay(0.1))}[name.split("_")[0]]()


FUNCTIONAL = NEW + [f"{c}_{r}" for r in ("lion", "nadam") for c in ("decay", "clipnorm", "clipnormdecay", "flat")]


@pytest.mark.parametrize("name", FUNCTIONAL)
def test_optimisers_update_gpu_matches_cpu(gpu_ext, monkeypatch, name):
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.ops import optim
    torch.manual_seed(7)
    ps = {"w": torch.randn(300, 7), "b": torch.randn(7) * 0.01, "e": torch.randn(5000)}
    gs = {"w": torch.randn(300, 7), "b": torch.randn(7) * 0.001, "e": torch.randn(5000) * 0.003}
    st = O.setup(_functional_rule(name), ps)
    psg = {k: v.cuda() for k, v in ps.items()}
    gsg = {k: v.cuda() for k, v in gs.items()}
    stg = O.setup(_functional_rule(name), psg)
    for _ in range(3):
        st, ps = O.update(st, ps, gs)
    calls = []
    real = optim.rule_

    def spy(*a, **kw):
        calls.append((a[0], kw))
        return real(*a, **kw)

    def boom(*a, **kw):
        raise AssertionError("a per-leaf rule ran on GPU leaves")

    monkeypatch.setattr(optim, "rule_", spy)
    for cls in (O.ClipNorm, O.WeightDecay, O.Lion, O.NAdam):
        monkeypatch.setattr(cls, "apply", boom)
    for _ in range(3):
        stg, psg = O.update(stg, psg, gsg)
    assert len(calls) == 3  # one fused launch group per step
    if "clipnorm" in name or "flat" in name:
        sc = calls[-1][1]["tscale"].cpu()
        assert sc.numel() == 3 and (sc < 1).any() and (sc == 1).any()
    if "decay" in name or "flat" in name:
        assert abs(calls[-1][1]["weight_decay"] - 0.1) < 1e-8
    lion = "lion" in name
    for k in ps:
        a, b = psg[k].cpu(), ps[k]
        if lion:  # a sign argument within rounding of zero: at most 0.1 % of the elements
            assert int((~torch.isclose(a, b, rtol=1e-5, atol=1e-6)).sum()) <= max(1, a.numel() // 1000)
        else:
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
    # the returned state has the table's layout
    s, sc_ = stg["w"].state, st["w"].state

    def same_layout(x, y):
        if isinstance(y, torch.Tensor):
            assert isinstance(x, torch.Tensor) and x.is_cuda and x.shape == y.shape
        elif isinstance(y, tuple) and y and all(isinstance(v, float) for v in y):
            assert x == y  # βt
        elif isinstance(y, tuple):
            assert isinstance(x, tuple) and len(x) == len(y)
            for u, v in zip(x, y):
                same_layout(u, v)
        else:
            assert x is None and y is None

    same_layout(s, sc_)
    flat_state = []

    def tensors(x, out):
        if isinstance(x, torch.Tensor):
            out.append(x)
        elif isinstance(x, tuple):
            for v in x:
                tensors(v, out)

    cpu_state = []
    tensors(s, flat_state)
    tensors(sc_, cpu_state)
    want_n = {"lion": 1, "adamax": 2, "amsgrad": 3, "nadam": 2, "adabelief": 2, "adadelta": 2}
    assert len(flat_state) == want_n[name.split("_")[-1]]
    if not lion:
        for a, b in zip(flat_state, cpu_state):
            torch.testing.assert_close(a.cpu(), b, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- engine, world of one
class TwoDtypes(torch.nn.Module):
    """A two-layer MLP with a bf16 first layer and an fp32 second: one bucket of each dtype."""

    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.a = torch.nn.Linear(32, 64).to(torch.bfloat16)
        self.b = torch.nn.Linear(64, 1)

    def forward(self, x):
        return self.b(torch.tanh(self.a(x.to(torch.bfloat16)).float()))


def _data(seed=21, n=16):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 32, generator=g)
    return x.cuda(), x.sum(1, keepdim=True).sin().cuda()


def _engine_rule(kind, lr=1e-2):
    return _rules()[kind](**({"eta": lr} if kind != "adadelta" else {}))


def _loss(d, x, y):
    return ((d(x) - y) ** 2).mean()


def _engine_state(d):
    out = [p.detach().clone() for p in d.module.parameters()]
    for b in d.buckets:
        out += [t.clone() for t in (b.master, b.exp_avg, b.exp_avg_sq, b.state3) if t is not None]
    return out


@pytest.fixture
def flux():
    import fluxmpi_amd as FluxMPI
    from fluxmpi_amd.utils.debug import stop_all
    FluxMPI.Init()
    yield FluxMPI
    stop_all()


@pytest.mark.parametrize("kind", KINDS)
def test_engine_matches_fused_functional_path(gpu_ext, kind):
    """DDP (a bf16 bucket with fp32 masters and states, an fp32 bucket) == ``ops.optim.rule_`` on the
    same gradients with host-side βt; ``optimiser_state()`` has the table's layout."""
    from fluxmpi_amd.ops import optim
    from fluxmpi_amd.parallel.ddp import DDP
    _, ns, has_bt = optim.RULES[kind]
    m1, m2 = TwoDtypes(0).cuda(), TwoDtypes(0).cuda()
    rule = _engine_rule(kind)
    ddp = DDP(m1, rule)
    assert sorted(str(b.dtype) for b in ddp.buckets) == ["torch.bfloat16", "torch.float32"]
    assert all((b.master is not None) == (b.dtype == torch.bfloat16) for b in ddp.buckets)
    ps = list(m2.parameters())
    fill = rule.epsilon if kind in ("adagrad", "amsgrad") else 0.0
    st = [[torch.full(p.shape, fill, device="cuda") for p in ps] for _ in range(ns)]
    ws = [p.detach().float() if p.dtype == torch.bfloat16 else None for p in ps]
    x, y = _data()
    bt = list(rule.beta) if has_bt else [0.0, 0.0]
    for _ in range(3):
        _loss(ddp, x, y).backward()
        ddp.step()
        for p in ps:
            p.grad = None
        _loss(m2, x, y).backward()
        with torch.no_grad():
            for low in (True, False):
                idx = [i for i, p in enumerate(ps) if (p.dtype == torch.bfloat16) == low]
                kw = dict(rule._hyper())
                if has_bt:
                    kw.update(bt1=float(torch.tensor(bt[0])), bt2=float(torch.tensor(bt[1])))
                optim.rule_(kind, [ps[i].data for i in idx], [ps[i].grad for i in idx],
                            [[s[i] for i in idx] for s in st], masters=[ws[i] for i in idx] if low else None, **kw)
        if has_bt:  # the engine's block is fp32 and advanced in fp32
            bt = [float(torch.tensor(bt[0]) * torch.tensor(rule.beta[0])), float(torch.tensor(bt[1]) * torch.tensor(rule.beta[1]))]
    torch.cuda.synchronize()
    frac = 1e-3 if kind == "lion" else 0.0  # Lion: a sign argument within rounding of zero
    for p, q in zip(m1.parameters(), m2.parameters()):
        tol = _tol(p.dtype)
        bad = int((~torch.isclose(p.detach().float(), q.detach().float(), **tol)).sum())
        assert bad <= max(1, int(frac * p.numel())) * (frac > 0), (kind, bad)
    leaf = ddp.optimiser_state()["a.weight"]
    s = leaf.state
    if ns == 1:
        assert isinstance(s, torch.Tensor) and s.shape == (64, 32) and s.dtype == torch.float32
    elif has_bt:
        assert len(s) == 3 and s[0].shape == (64, 32) and s[1].shape == (64, 32) and len(s[2]) == 2
        assert s[2] == pytest.approx((rule.beta[0] ** 4, rule.beta[1] ** 4), rel=1e-5)
    else:
        assert len(s) == ns and all(t.shape == (64, 32) for t in s)
    names = [n for n, _ in m2.named_parameters()]
    got = s if ns == 1 else s[0]
    torch.testing.assert_close(got, st[0][names.index("a.weight")], **_tol(torch.float32))


@pytest.mark.parametrize("kind", KINDS)
def test_engine_overlap_opt_is_bitwise_step(gpu_ext, flux, kind):
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    x, y = _data(22, 32)
    outs = []
    for ov in (False, True):
        m = TwoDtypes(3).cuda()
        d = DDP(m, O.OptimiserChain(O.ClipNorm(0.2), _engine_rule(kind)), force_comm=True, overlap_opt=ov, average=True)
        assert d.overlap_opt == ov and len(d.buckets) == 2
        for _ in range(3):
            _loss(d, x, y).backward()
            d.step()
        torch.cuda.synchronize()
        outs.append(_engine_state(d) + [d.grad_norm().clone()])
    assert len(outs[0]) == len(outs[1])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", KINDS)
def test_graphed_step_matches_eager_and_sees_set_lr(gpu_ext, kind):
    from fluxmpi_amd.parallel.ddp import DDP
    from fluxmpi_amd.parallel.graph import GraphedStep
    m1, m2 = TwoDtypes(1).cuda(), TwoDtypes(1).cuda()
    d1, d2 = DDP(m1, _engine_rule(kind)), DDP(m2, _engine_rule(kind))
    x, y = _data(23, 16)
    g = GraphedStep(d1, _loss, x, y, warmup=2)
    for _ in range(2):
        _loss(d2, x, y).backward()
        d2.step()
    for i in range(4):
        if i == 2:
            if kind == "adadelta":
                for d in (d1, d2):
                    with pytest.raises(ValueError):
                        d.set_lr(0.5)
            else:
                d1.set_lr(3e-2)
                d2.set_lr(3e-2)
        g(x, y)
        _loss(d2, x, y).backward()
        d2.step()
    torch.cuda.synchronize()
    frac = 1e-3 if kind == "lion" else 0.0
    for p, q in zip(m1.parameters(), m2.parameters()):
        bad = int((~torch.isclose(p.detach().float(), q.detach().float(), **_tol(p.dtype))).sum())
        assert bad <= max(1, int(frac * p.numel())) * (frac > 0), (kind, bad)
    if kind != "adadelta":
        # the replayed graph took the new learning rate: the same engine without it ends elsewhere
        m3 = TwoDtypes(1).cuda()
        d3 = DDP(m3, _engine_rule(kind))
        for _ in range(6):
            _loss(d3, x, y).backward()
            d3.step()
        torch.cuda.synchronize()
        assert not torch.allclose(m1.b.weight, m3.b.weight, rtol=1e-4, atol=1e-6)


def test_engine_clip_global_norm_with_lion(gpu_ext):
    """The global scale cannot change a sign, so it shows in Lion's momentum: m == the functional
    rule's m on gradients scaled beforehand; ``grad_norm()`` is the unclipped norm."""
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    from tests.test_clip_gpu import _grads_of, _mlp, _prescale_global
    w = 0.5
    m1, m2 = _mlp(4), _mlp(4)
    ddp = DDP(m1, O.Lion(1e-3), clip_global_norm=w, bucket_mb=0.004, first_bucket_mb=0.002)
    assert len(ddp.buckets) > 1
    ps = {n: p.detach().clone() for n, p in m2.named_parameters()}
    st = O.setup(O.Lion(1e-3), ps)
    x, y = _data()
    active = 0
    for _ in range(3):
        _loss(ddp, x, y).backward()
        ddp.step()
        # the reference follows the ENGINE's parameters, so a flipped sign cannot make the runs drift
        grads, nrm = _prescale_global(_grads_of(m2, ps, x, y), w)
        active += nrm > w
        torch.testing.assert_close(float(ddp.grad_norm()), nrm, rtol=1e-5, atol=0)
        st, _ = O.update(st, ps, grads)
        ps = {n: p.detach().clone() for n, p in m1.named_parameters()}
    assert active > 0
    state = ddp.optimiser_state()
    for n in ps:
        torch.testing.assert_close(state[n].state, st[n].state, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("kind", KINDS)
def test_engine_checkpoint_round_trip_is_bitwise(gpu_ext, kind):
    from fluxmpi_amd.parallel.ddp import DDP
    x, y = _data(24, 16)
    m1 = TwoDtypes(5).cuda()
    d1 = DDP(m1, _engine_rule(kind))
    for _ in range(2):
        _loss(d1, x, y).backward()
        d1.step()
    sd = d1.state_dict()
    assert all(("s3" in s) == (kind == "amsgrad") for s in sd["buckets"])
    assert all(set(s) - {"s3"} == {"master", "m", "v"} for s in sd["buckets"])
    m2 = TwoDtypes(6).cuda()
    d2 = DDP(m2, _engine_rule(kind))
    d2.load_state_dict(sd)
    for d in (d1, d2):
        for _ in range(2):
            _loss(d, x, y).backward()
            d.step()
    torch.cuda.synchronize()
    a, b = _engine_state(d1), _engine_state(d2)
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(d1.hyper, d2.hyper)


def test_engine_runs_rmsprop_and_lion_exists(gpu_ext):
    """What failed before the rule set was widened."""
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    assert issubclass(O.Lion, O.AbstractRule)
    m = TwoDtypes(7).cuda()
    before = m.b.weight.detach().clone()
    d = DDP(m, O.RMSProp(1e-3))
    x, y = _data()
    _loss(d, x, y).backward()
    d.step()
    torch.cuda.synchronize()
    assert not torch.equal(before, m.b.weight.detach()) and torch.isfinite(m.b.weight).all()
