"""The layer-wise kernels (``csrc/kernels/optim_layerwise.hip``: LARS and LAMB) on the GPU: against
``ops.optim.lars_reference_`` / ``lamb_reference_`` over the dtype combinations, the ratio table
against fp64 norms, the fixed-order fold, the functional API on GPU leaves and the DDP engine (eager,
overlapped, graphed, checkpointed, globally clipped)."""
import pytest
import torch

from tests.test_clip_gpu import SIZES, SMALL, UNALIGNED, _acc, _grads_of, _mlp, _prescale_global, _tol
from tests.test_clip_gpu import _data as _mlp_data
from tests.test_rules_gpu import ALL_COMBOS, CANARY, GRAD_ONLY, Guarded, _leaves

pytestmark = pytest.mark.gpu

LARS = dict(lr=0.1, momentum=0.9, trust=0.02, weight_decay=0.01, eps=1e-9)
LAMB = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.01)
GS = 0.5
EMPTY = SIZES.index(0)


def _ratio_tol(dt):
    return dict(rtol=1e-12 if dt == torch.float64 else 1e-5, atol=0)


def _h(dt, v):
    """The hyperparameter as a kernel of compute precision ``dt`` holds it."""
    return v if dt == torch.float64 else float(torch.tensor(v, dtype=torch.float32))


def _lars_ratio64(x, g, ct):
    """LARS' ratio from fp64 CPU norms of the values the device holds."""
    xn, gn = x.double().cpu().pow(2).sum().sqrt(), (g.double().cpu() * GS).pow(2).sum().sqrt()
    if not (xn > 0 and gn > 0):
        return torch.tensor(1.0, dtype=torch.float64)
    return _h(ct, LARS["trust"]) * xn / (gn + _h(ct, LARS["weight_decay"]) * xn + _h(ct, LARS["eps"]))


def _lamb_ratio64(x_before, m, v, bt1, bt2, ct):
    """LAMB's ratio from fp64 CPU norms: u formed in fp64 from the moments the kernel stored."""
    x, m, v = x_before.double().cpu(), m.double().cpu(), v.double().cpu()
    u = m / (1 - _h(ct, bt1)) / (torch.sqrt(v / (1 - _h(ct, bt2))) + _h(ct, LAMB["eps"])) + _h(ct, LAMB["weight_decay"]) * x
    xn, un = x.pow(2).sum().sqrt(), u.pow(2).sum().sqrt()
    return xn / un if (xn > 0 and un > 0) else torch.tensor(1.0, dtype=torch.float64)


def _states(rule, sd, sizes=SIZES):
    """fp32 / fp64 states start at zero (three steps follow); bf16 / fp16 states at positive values
    rounded to the state dtype, identical on both sides (one step follows)."""
    ns = 1 if rule == "lars" else 2
    if sd in (torch.float32, torch.float64):
        return [[torch.zeros(n, dtype=sd) for n in sizes] for _ in range(ns)]
    return [[t.abs().mul(0.1).to(sd) for t in _leaves(40 + k)] for k in range(ns)]


def _call(rule, optim, p, g, st, t, **kw):
    if rule == "lars":
        optim.lars_(p, g, st[0], grad_scale=GS, **LARS, **kw)
    else:
        optim.lamb_(p, g, st[0], st[1], grad_scale=GS, bt1=LAMB["beta1"] ** t, bt2=LAMB["beta2"] ** t, **LAMB, **kw)


def _call_ref(rule, optim, p, g, st, t, **kw):
    if rule == "lars":
        optim.lars_reference_(p, g, st[0], grad_scale=GS, **LARS, **kw)
    else:
        optim.lamb_reference_(p, g, st[0], st[1], grad_scale=GS, bt1=LAMB["beta1"] ** t, bt2=LAMB["beta2"] ** t,
                              **LAMB, **kw)


def _compare(got, want, dt):
    for a, b in zip(got, want):
        torch.testing.assert_close(a.cpu().to(_acc(dt)), b.to(_acc(dt)), **_tol(dt))


# ---------------------------------------------------------------- kernels vs the references
@pytest.mark.parametrize("pd,gd,sd,master", ALL_COMBOS)
@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_kernel_matches_reference(gpu_ext, rule, pd, gd, sd, master):
    """30 leaves (an empty one, single elements, chunk edges, two launches, a misaligned leaf, a leaf
    whose gradient alone is misaligned), fresh gradients each step, canaries around every buffer,
    the workspace and the ratio table included."""
    from fluxmpi_amd.ops import optim
    ct = _acc(pd)
    off_all, off_g = (UNALIGNED,), (UNALIGNED, GRAD_ONLY)
    P = Guarded(_leaves(1), pd, off_all)
    G = Guarded(_leaves(0), gd, off_g)
    st_cpu = _states(rule, sd)
    S = [Guarded(s, sd, off_all) for s in st_cpu]
    W = Guarded([v.cpu().float() for v in P.views], torch.float32, off_all) if master else None
    assert len(P.views) == 30 and P.views[EMPTY].numel() == 0
    need = optim.layerwise_workspace(P.views)
    assert need == 2 * sum((n + 4095) // 4096 for n in SIZES)
    work = torch.full((need + 8,), CANARY, dtype=ct, device="cuda")
    table = torch.full((len(SIZES) + 8,), CANARY, dtype=ct, device="cuda")
    pc = [v.cpu().clone() for v in P.views]
    sc = [[t.clone() for t in s] for s in st_cpu]
    wc = [v.cpu().clone() for v in W.views] if master else None
    want_q = torch.zeros(len(SIZES), dtype=ct)
    steps = 3 if sd in (torch.float32, torch.float64) else 1
    for t in range(1, steps + 1):
        if t > 1:
            G.update(_leaves(10 + t))  # fresh gradients
        gc = [v.cpu().clone() for v in G.views]
        x0 = [v.clone() for v in (W.views if master else P.views)]
        _call(rule, optim, P.views, G.views, [s.views for s in S], t, masters=W.views if master else None,
              ratios=table[:len(SIZES)], workspace=work[:need])
        _call_ref(rule, optim, pc, gc, sc, t, masters=wc, ratios=want_q)
        # the ratio table against fp64 norms, every step
        if rule == "lars":
            q64 = torch.stack([_lars_ratio64(x, g, ct) for x, g in zip(x0, G.views)])
        else:
            q64 = torch.stack([_lamb_ratio64(x, m, v, LAMB["beta1"] ** t, LAMB["beta2"] ** t, ct)
                               for x, m, v in zip(x0, S[0].views, S[1].views)])
        got_q = table[:len(SIZES)].double().cpu()
        print(f"step {t}: ratio max rel err {float(((got_q - q64).abs() / q64).max()):.3e}")
        torch.testing.assert_close(got_q, q64, **_ratio_tol(pd))
        assert got_q[EMPTY] == 1 and ((got_q > 0) & (got_q != 1)).sum() == len(SIZES) - 1
    torch.cuda.synchronize()
    for guard in [P, G, *S] + ([W] if master else []):
        guard.check()
    assert bool((work[need:] == CANARY).all()) and bool((table[len(SIZES):] == CANARY).all())
    for s, c in zip(S, sc):
        _compare(s.views, c, sd)
    _compare(P.views, pc, pd)
    if master:
        _compare(W.views, wc, torch.float32)


# 257 chunks + 3: the fold gives threads 0 and 1 two partials; 4097 chunks + 1: past the leaf size
# at which the fold becomes a launch of its own
@pytest.mark.parametrize("n", [257 * 4096 + 3, 4097 * 4096 + 1])
@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_large_leaf_fold(gpu_ext, rule, n):
    from fluxmpi_amd.ops import optim
    g = torch.Generator().manual_seed(n % 1000)
    sizes = [100, n, 4097]  # neighbours on both sides
    pc = [torch.randn(k, generator=g) for k in sizes]
    gc = [torch.randn(k, generator=g) * 0.3 for k in sizes]
    sc = _states(rule, torch.float32, sizes)
    p, gr = [t.cuda() for t in pc], [t.cuda() for t in gc]
    st = [[t.cuda() for t in s] for s in sc]
    q, want_q = torch.zeros(3, device="cuda"), torch.zeros(3)
    x0 = [t.clone() for t in p]
    _call(rule, optim, p, gr, st, 1, ratios=q)
    _call_ref(rule, optim, pc, gc, sc, 1, ratios=want_q)
    if rule == "lars":
        q64 = torch.stack([_lars_ratio64(x, g_, torch.float32) for x, g_ in zip(x0, gr)])
    else:
        q64 = torch.stack([_lamb_ratio64(x, m, v, LAMB["beta1"], LAMB["beta2"], torch.float32)
                           for x, m, v in zip(x0, st[0], st[1])])
    print("ratio rel err", ((q.double().cpu() - q64).abs() / q64).tolist())
    torch.testing.assert_close(q.double().cpu(), q64, rtol=1e-5, atol=0)
    _compare(p, pc, torch.float32)
    for s, c in zip(st, sc):
        _compare(s, c, torch.float32)


@pytest.mark.parametrize("pd,gd,sd,master", [ALL_COMBOS[0], ALL_COMBOS[2]])
@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_two_runs_are_bit_identical(gpu_ext, rule, pd, gd, sd, master):
    from fluxmpi_amd.ops import optim
    runs = []
    for _ in range(2):
        p = [t.to(pd).cuda() for t in _leaves(1)] + [_big().to(pd).cuda()]
        g = [t.to(gd).cuda() for t in _leaves(0)] + [(_big() * 0.3).to(gd).cuda()]
        st = [[torch.zeros_like(t, dtype=sd) for t in p] for _ in range(1 if rule == "lars" else 2)]
        w = [t.float() for t in p] if master else None
        q = torch.zeros(len(p), device="cuda")
        for t in (1, 2):
            _call(rule, optim, p, g, st, t, masters=w, ratios=q)
        torch.cuda.synchronize()
        runs.append(p + [t for s in st for t in s] + (w or []) + [q])
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _big():
    return _leaves_big()[0]


_BIG: list = []


def _leaves_big():
    """One 258-chunk leaf (more partials than fold threads), computed once."""
    if not _BIG:
        _BIG.append(torch.randn(257 * 4096 + 3, generator=torch.Generator().manual_seed(99)))
    return _BIG


@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_zero_leaves_inside_a_call(gpu_ext, rule):
    """An all-zero parameter and (LARS) an all-zero gradient leaf: q == 1, finite results, and the
    other leaves of the call come out as the same bits as without them."""
    from fluxmpi_amd.ops import optim
    ZP, ZG = 5, 11  # a several-chunk leaf and a small one

    def run(zero):
        P, G = [t.clone() for t in _leaves(1)], [t.clone() for t in _leaves(0)]
        if zero:
            P[ZP].zero_()
            G[ZG].zero_()
        p, g = [t.cuda() for t in P], [t.cuda() for t in G]
        st = [[torch.zeros_like(t) for t in p] for _ in range(1 if rule == "lars" else 2)]
        q = torch.zeros(len(p), device="cuda")
        _call(rule, optim, p, g, st, 1, ratios=q)
        torch.cuda.synchronize()
        return p, st, q

    p0, s0, q0 = run(False)
    p1, s1, q1 = run(True)
    assert q1[ZP] == 1 and q0[ZP] != 1
    if rule == "lars":
        assert q1[ZG] == 1 and q0[ZG] != 1
    else:  # LAMB with a zero gradient: u = decay·x, q = 1/decay
        torch.testing.assert_close(float(q1[ZG]), 1.0 / LAMB["weight_decay"], rtol=1e-5, atol=0)
    for i in (ZP, ZG):
        assert torch.isfinite(p1[i]).all() and all(torch.isfinite(s[i]).all() for s in s1)
    # LARS, zero parameter at q == 1: the plain momentum step from zero velocity, x = -lr·g
    if rule == "lars":
        torch.testing.assert_close(p1[ZP], -_h(torch.float32, LARS["lr"]) * GS * _leaves(0)[ZP].cuda(), rtol=1e-6, atol=0)
    for i in range(len(p0)):
        if i not in (ZP, ZG):
            assert torch.equal(p0[i], p1[i]) and torch.equal(q0[i], q1[i])
            assert all(torch.equal(a[i], b[i]) for a, b in zip(s0, s1))


def test_argument_errors(gpu_ext):
    from fluxmpi_amd.ops import optim
    p, g, v = [torch.zeros(8, 2, device="cuda")], [torch.zeros(8, 2, device="cuda")], [torch.zeros(8, 2, device="cuda")]
    with pytest.raises(TypeError):
        optim.lars_(p, g, v, workspace=torch.zeros(1, device="cuda"), **LARS)  # needs two entries
    with pytest.raises(TypeError):
        optim.lars_(p, g, v, ratios=torch.zeros(1, device="cuda", dtype=torch.float64), **LARS)
    with pytest.raises(ValueError):
        optim.lamb_(p, g, v, [], bt1=0.9, bt2=0.999, **LAMB)
    with pytest.raises(RuntimeError):
        gpu_ext.mt_rule(8, [p[0].data_ptr()], [g[0].data_ptr()], [v[0].data_ptr()], [], [], [], [16], 7, 7, 7, 0.1, 0.9,
                        0.02, 0.0, 0.0, 0.0, 0.0, 1.0, 0, 0, 0, 0.0, 0)  # no partials address, no ratio table


# ---------------------------------------------------------------- optimisers.update on GPU leaves
@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_optimisers_update_gpu_matches_cpu(gpu_ext, monkeypatch, name):
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.ops import optim
    mk = (lambda: O.LARS(0.1, 0.9, trust=0.02, decay=0.01)) if name == "lars" else (lambda: O.LAMB(1e-2))
    torch.manual_seed(7)
    ps = {"w": torch.randn(300, 7), "b": torch.randn(7) * 0.01, "k": torch.randn(80, 64), "z": torch.zeros(1, 1, 16)}
    gs = {"w": torch.randn(300, 7), "b": torch.randn(7) * 0.001, "k": torch.randn(80, 64) * 0.003,
          "z": torch.randn(1, 1, 16)}
    st = O.setup(mk(), ps)
    psg = {k: v.cuda() for k, v in ps.items()}
    gsg = {k: v.cuda() for k, v in gs.items()}
    stg = O.setup(mk(), psg)
    for _ in range(3):
        st, ps = O.update(st, ps, gs)
    calls = {"layer": 0, "base": 0}
    fn, base = ("lars_", "sgd_") if name == "lars" else ("lamb_", "adam_")
    real, real_base = getattr(optim, fn), getattr(optim, base)

    def spy(*a, **kw):
        calls["layer"] += 1
        assert len(a[0]) == 3  # the adapted leaves, in one call
        return real(*a, **kw)

    def spy_base(*a, **kw):
        calls["base"] += 1
        assert len(a[0]) == 1 and kw.get("weight_decay", 0.0) == 0.0  # the 1-D leaf: neither decayed nor adapted
        return real_base(*a, **kw)

    def boom(*a, **kw):
        raise AssertionError("the per-leaf rule ran on GPU leaves")

    monkeypatch.setattr(optim, fn, spy)
    monkeypatch.setattr(optim, base, spy_base)
    monkeypatch.setattr(O.LARS if name == "lars" else O.LAMB, "apply", boom)
    for _ in range(3):
        stg, psg = O.update(stg, psg, gsg)
    assert calls == {"layer": 3, "base": 3}
    for k in ps:
        torch.testing.assert_close(psg[k].cpu(), ps[k], rtol=1e-5, atol=1e-6)
    a, b = stg["w"].state, st["w"].state
    if name == "lars":
        torch.testing.assert_close(a.cpu(), b, rtol=1e-5, atol=1e-6)
    else:
        assert len(a) == 3 and a[2] == b[2]
        torch.testing.assert_close(a[0].cpu(), b[0], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(a[1].cpu(), b[1], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- engine, world of one
def _rule(name):
    from fluxmpi_amd import optimisers as O
    return O.LARS(0.05, 0.9, trust=0.02, decay=0.01) if name == "lars" else O.LAMB(1e-2, decay=0.01)


@pytest.fixture
def flux():
    import fluxmpi_amd as FluxMPI
    from fluxmpi_amd.utils.debug import stop_all
    FluxMPI.Init()
    yield FluxMPI
    stop_all()


def _engine_state(d):
    out = [p.detach().clone() for p in d.module.parameters()]
    for b in d.buckets:
        out += [t.clone() for t in (b.master, b.exp_avg, b.exp_avg_sq, b.ratios) if t is not None]
    return out


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_engine_matches_functional(gpu_ext, name):
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    m1, m2 = _mlp(0), _mlp(0)
    ddp = DDP(m1, _rule(name), **SMALL)
    assert ddp.kind == name and len(ddp.buckets) > 1
    ps = {n: p.detach().clone() for n, p in m2.named_parameters()}
    st = O.setup(_rule(name), ps)
    x, y = _mlp_data()
    for _ in range(3):
        ((ddp(x) - y) ** 2).mean().backward()
        ddp.step()
        st, ps = O.update(st, ps, _grads_of(m2, ps, x, y))
    got = dict(m1.named_parameters())
    # one adapted and one 1-D leaf on their own, then the rest
    assert got["0.weight"].ndim == 2 and got["0.bias"].ndim == 1
    torch.testing.assert_close(got["0.weight"].detach(), ps["0.weight"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(got["0.bias"].detach(), ps["0.bias"], rtol=1e-5, atol=1e-6)
    for n, p in got.items():
        torch.testing.assert_close(p.detach(), ps[n], rtol=1e-5, atol=1e-6)
    tr = ddp.trust_ratios()
    assert sorted(tr) == ["0.weight", "2.weight", "4.weight"]  # exactly the adapted leaves
    assert all(t.is_cuda and t.dim() == 0 and t.dtype == torch.float32 and 0 < float(t) != 1 for t in tr.values())
    leaf = ddp.optimiser_state()["0.weight"]
    if name == "lamb":  # Adam's layout
        assert len(leaf.state) == 3 and leaf.state[0].shape == (64, 32) and len(leaf.state[2]) == 2
        torch.testing.assert_close(leaf.state[0], st["0.weight"].state[0], rtol=1e-5, atol=1e-6)
    else:  # Momentum's
        torch.testing.assert_close(leaf.state, st["0.weight"].state, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_engine_overlap_opt_is_bitwise_step(gpu_ext, flux, name):
    """force_comm + overlap_opt (stats, apply and the 1-D launch behind each bucket's allreduce) ==
    the updates in step(): bf16 parameters, fp32 masters, several buckets."""
    from fluxmpi_amd.parallel.ddp import DDP
    x, y = _mlp_data(22, 64)
    x = x.bfloat16()
    outs = []
    for ov in (False, True):
        m = _mlp(3).bfloat16()
        d = DDP(m, _rule(name), force_comm=True, overlap_opt=ov, average=True, **SMALL)
        assert d.overlap_opt == ov and len(d.buckets) > 1 and all(b.master is not None for b in d.buckets)
        for _ in range(4):
            ((d(x).float() - y) ** 2).mean().backward()
            d.step()
        torch.cuda.synchronize()
        outs.append(_engine_state(d))
    assert len(outs[0]) == len(outs[1])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_graphed_step_matches_eager(gpu_ext, name):
    import torch.nn.functional as F
    from fluxmpi_amd.parallel.ddp import DDP
    from fluxmpi_amd.parallel.graph import GraphedStep
    m1, m2 = _mlp(1), _mlp(1)
    d1, d2 = DDP(m1, _rule(name), **SMALL), DDP(m2, _rule(name), **SMALL)
    x, y = _mlp_data(23, 16, target="randn")

    def loss_fn(d, xx, yy):
        return F.mse_loss(d(xx), yy)

    g = GraphedStep(d1, loss_fn, x, y, warmup=2)
    for _ in range(2):
        loss_fn(d2, x, y).backward()
        d2.step()
    for k in range(4):
        if k == 2:  # the learning rate lives on the device: the captured step sees the change
            before = [p.detach().clone() for p in m1.parameters()]
            d1.set_lr(0.5 * d1._inner.eta)
            d2.set_lr(0.5 * d2._inner.eta)
        g(x, y)
        loss_fn(d2, x, y).backward()
        d2.step()
    torch.cuda.synchronize()
    for p, q in zip(m1.parameters(), m2.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-5, atol=1e-6)
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, m1.parameters()))
    t1, t2 = d1.trust_ratios(), d2.trust_ratios()
    for n in t2:
        torch.testing.assert_close(t1[n], t2[n], rtol=1e-5, atol=0)


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_state_dict_round_trip_continues_bitwise(gpu_ext, name):
    from fluxmpi_amd.parallel.ddp import DDP
    x, y = _mlp_data()
    m1 = _mlp(2)
    d1 = DDP(m1, _rule(name), **SMALL)
    for _ in range(2):
        ((d1(x) - y) ** 2).mean().backward()
        d1.step()
    sd = d1.state_dict()
    assert all(set(s) == {"master", "m", "v"} for s in sd["buckets"])  # Momentum's / Adam's keys
    m2 = _mlp(9)  # other weights: everything must come from the checkpoint
    d2 = DDP(m2, _rule(name), **SMALL)
    d2.load_state_dict(sd)
    for d in (d1, d2):
        for _ in range(2):
            ((d(x) - y) ** 2).mean().backward()
            d.step()
    torch.cuda.synchronize()
    for a, b in zip(_engine_state(d1), _engine_state(d2)):
        assert torch.equal(a, b)


def test_engine_lamb_clip_global_norm(gpu_ext):
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    w = 0.5
    m1, m2 = _mlp(4), _mlp(4)
    ddp = DDP(m1, _rule("lamb"), clip_global_norm=w, **SMALL)
    assert len(ddp.buckets) > 1 and not ddp.overlap_opt
    ps = {n: p.detach().clone() for n, p in m2.named_parameters()}
    st = O.setup(_rule("lamb"), ps)
    x, y = _mlp_data()
    active = 0
    for _ in range(3):
        ((ddp(x) - y) ** 2).mean().backward()
        ddp.step()
        grads, nrm = _prescale_global(_grads_of(m2, ps, x, y), w)
        active += nrm > w
        torch.testing.assert_close(float(ddp.grad_norm()), nrm, rtol=1e-5, atol=0)
        st, ps = O.update(st, ps, grads)
    assert active > 0
    for n, p in m1.named_parameters():
        torch.testing.assert_close(p.detach(), ps[n], rtol=1e-5, atol=1e-6)


def test_engine_lars_refuses_clip_global_norm(gpu_ext):
    from fluxmpi_amd.parallel.ddp import DDP
    with pytest.raises(ValueError, match="LARS"):
        DDP(_mlp(6), _rule("lars"), clip_global_norm=1.0, **SMALL)
