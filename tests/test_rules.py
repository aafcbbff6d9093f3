"""The rule set beyond Adam and SGD on the CPU: state layouts, one hand-computed step per rule,
AdaDelta against torch.optim, ``ops.optim.rule_reference_`` against the per-leaf rules, the fused
plans of the chains, and ``DistributedOptimizer`` over gloo."""
import math

import pytest
import torch


def _rules():
    from fluxmpi_amd import optimisers as O
    return {"rmsprop": O.RMSProp, "adagrad": O.AdaGrad, "lion": O.Lion, "adamax": O.AdaMax, "amsgrad": O.AMSGrad,
            "nadam": O.NAdam, "adabelief": O.AdaBelief, "adadelta": O.AdaDelta}


KINDS = ["rmsprop", "adagrad", "lion", "adamax", "amsgrad", "nadam", "adabelief", "adadelta"]
NEW = KINDS[2:]


def test_new_rules_exist_with_defaults():
    from fluxmpi_amd import optimisers as O
    assert (O.Lion().eta, O.Lion().beta) == (1e-3, (0.9, 0.999))
    for cls in (O.AdaMax, O.AMSGrad, O.NAdam):
        assert (cls().eta, cls().beta, cls().epsilon) == (1e-3, (0.9, 0.999), 1e-8)
    assert (O.AdaBelief().eta, O.AdaBelief().beta, O.AdaBelief().epsilon) == (1e-3, (0.9, 0.999), 1e-16)
    assert (O.AdaDelta().rho, O.AdaDelta().epsilon) == (0.9, 1e-7) and not hasattr(O.AdaDelta(), "eta")
    for name in ("Lion", "AdaMax", "AMSGrad", "NAdam", "AdaBelief", "AdaDelta"):
        assert name in O.__all__


def test_init_layouts_and_fill_values():
    x = torch.randn(3, 2)
    R = _rules()
    z = torch.zeros_like(x)
    bt = (float(torch.tensor(0.9)), float(torch.tensor(0.999)))  # β rounded to fp32
    assert torch.equal(R["rmsprop"]().init(x), z)
    assert torch.equal(R["adagrad"](epsilon=1e-3).init(x), torch.full_like(x, 1e-3))
    assert torch.equal(R["lion"]().init(x), z)
    for k in ("adamax", "nadam", "adabelief"):
        s = R[k]().init(x)
        assert len(s) == 3 and torch.equal(s[0], z) and torch.equal(s[1], z) and s[2] == bt
        assert s[0] is not s[1]
    s = R["amsgrad"](epsilon=1e-3).init(x)
    assert len(s) == 3 and all(torch.equal(t, torch.full_like(x, 1e-3)) for t in s)
    assert len({t.data_ptr() for t in s}) == 3
    s = R["adadelta"]().init(x)
    assert len(s) == 2 and torch.equal(s[0], z) and torch.equal(s[1], z) and s[0] is not s[1]


def _hand_step(kind, g):
    """Two steps of the table from its initial state, in Python floats (fp64): returns the dx'."""
    b1, b2, eta = 0.9, 0.999, 1e-3
    out = []
    if kind == "rmsprop":
        acc = 0.0
        for _ in range(2):
            acc = 0.9 * acc + 0.1 * g * g
            out.append(g * eta / (math.sqrt(acc) + 1e-8))
    elif kind == "adagrad":
        acc = 1e-8
        for _ in range(2):
            acc += g * g
            out.append(g * 0.1 / (math.sqrt(acc) + 1e-8))
    elif kind == "lion":
        m = 0.0
        for _ in range(2):
            a = b1 * m + (1 - b1) * g
            out.append(eta * ((a > 0) - (a < 0)))
            m = b2 * m + (1 - b2) * g
    elif kind == "adamax":
        m = u = 0.0
        bt1 = b1
        for _ in range(2):
            m = b1 * m + (1 - b1) * g
            u = max(b2 * u, abs(g))
            out.append(eta / (1 - bt1) * m / (u + 1e-8))
            bt1 *= b1
    elif kind == "amsgrad":
        m = v = vh = 1e-8
        for _ in range(2):
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
            vh = max(vh, v)
            out.append(eta * m / (math.sqrt(vh) + 1e-8))
    elif kind == "nadam":
        m = v = 0.0
        bt1, bt2 = b1, b2
        for _ in range(2):
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
            out.append((b1 * m / (1 - b1 * bt1) + (1 - b1) * g / (1 - bt1)) / (math.sqrt(v * b2 / (1 - bt2)) + 1e-8) * eta)
            bt1, bt2 = bt1 * b1, bt2 * b2
    elif kind == "adabelief":
        m = s = 0.0
        bt1, bt2 = b1, b2
        for _ in range(2):
            m = b1 * m + (1 - b1) * g
            s = b2 * s + (1 - b2) * (g - m) ** 2 + 1e-16
            out.append(eta * m / (1 - bt1) / (math.sqrt(s / (1 - bt2)) + 1e-16))
            bt1, bt2 = bt1 * b1, bt2 * b2
    else:
        acc = d = 0.0
        for _ in range(2):
            acc = 0.9 * acc + 0.1 * g * g
            dx = g * math.sqrt(d + 1e-7) / math.sqrt(acc + 1e-7)
            d = 0.9 * d + 0.1 * dx * dx
            out.append(dx)
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("g", [0.5, -0.25])
def test_hand_computed_scalar_steps(kind, g):
    rule = _rules()[kind]()
    x = torch.tensor([1.0], dtype=torch.float64)
    st = rule.init(x)
    for want in _hand_step(kind, g):
        st, dx = rule.apply(st, x, torch.tensor([g], dtype=torch.float64))
        assert float(dx) == pytest.approx(want, rel=1e-12, abs=0)
    if kind in ("adamax", "nadam", "adabelief"):
        assert st[2] == pytest.approx((0.9 ** 3, 0.999 ** 3), rel=1e-12)


def test_lion_sign_of_zero_is_zero():
    from fluxmpi_amd import optimisers as O
    x = torch.ones(3)
    m, dx = O.Lion(0.5).apply(torch.zeros(3), x, torch.tensor([0.0, 2.0, -2.0]))
    assert dx.tolist() == [0.0, 0.5, -0.5]


def test_adadelta_matches_torch_optim():
    """An independent oracle: torch.optim.Adadelta(lr=1) is the same recurrence."""
    from fluxmpi_amd import optimisers as O
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(40, dtype=torch.float64, generator=g)
    grads = [torch.randn(40, dtype=torch.float64, generator=g) for _ in range(5)]
    p = torch.nn.Parameter(x0.clone())
    opt = torch.optim.Adadelta([p], lr=1.0, rho=0.9, eps=1e-7)
    ps = {"x": x0.clone()}
    st = O.setup(O.AdaDelta(0.9, 1e-7), ps)
    for gr in grads:
        p.grad = gr.clone()
        opt.step()
        st, ps = O.update(st, ps, {"x": gr})
    torch.testing.assert_close(ps["x"], p.detach(), rtol=1e-12, atol=0)
    torch.testing.assert_close(st["x"].state[0], opt.state[p]["square_avg"], rtol=1e-12, atol=0)
    torch.testing.assert_close(st["x"].state[1], opt.state[p]["acc_delta"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", KINDS)
def test_rule_reference_equals_per_leaf_apply(kind, dtype):
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.ops import optim
    gen = torch.Generator().manual_seed(5)
    rule = _rules()[kind]()
    x = torch.randn(200, dtype=dtype, generator=gen)
    xr = x.clone()
    st = rule.init(x)
    sr = [t.clone() for t in rule._tensors(rule.init(x))]
    has_bt = optim.RULES[kind][2]
    for _ in range(3):
        g = torch.randn(200, dtype=dtype, generator=gen)
        bt = st[2] if has_bt else (0.0, 0.0)
        st, dx = rule.apply(st, x, g)
        x = x - dx
        optim.rule_reference_(kind, [xr], [g], [[t] for t in sr], bt1=bt[0], bt2=bt[1], **rule._hyper(x))
    tol = dict(rtol=1e-12, atol=1e-15) if dtype == torch.float64 else dict(rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(xr, x, **tol)
    for a, b in zip(sr, rule._tensors(st)):
        torch.testing.assert_close(a, b, **tol)


def test_rule_reference_cpu_entry_point_and_errors():
    """``rule_`` on CPU tensors is the reference, with ``dev_hyper`` read on the host."""
    from fluxmpi_amd.ops import optim
    x, g = torch.randn(10), torch.randn(10)
    a, b = [x.clone()], [x.clone()]
    sa, sb = [[torch.zeros(10)], [torch.zeros(10)]], [[torch.zeros(10)], [torch.zeros(10)]]
    kw = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1, grad_scale=0.5, clip_delta=0.3)
    optim.rule_("nadam", a, [g], sa, dev_hyper=torch.tensor([1e-2, 0.81, 0.998]), **kw)
    optim.rule_reference_("nadam", b, [g], sb, lr=1e-2, bt1=float(torch.tensor(0.81)), bt2=float(torch.tensor(0.998)), **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(sa[1][0], sb[1][0]) and not torch.equal(a[0], x)
    with pytest.raises(ValueError):
        optim.rule_("radam", a, [g], sa)
    with pytest.raises(ValueError):
        optim.rule_("amsgrad", a, [g], sa)  # needs three state lists


def test_fused_plan_recognises_the_new_chains():
    from fluxmpi_amd import optimisers as O
    R = _rules()
    for k in NEW:
        r = R[k]()
        assert O.OptimiserChain(r, O.WeightDecay(0.1)).fused_plan()[1].opts[0] is r
        for clip in (O.ClipNorm(1.0), O.ClipGrad(0.5)):
            assert O.OptimiserChain(clip, r).fused_plan() == (clip, r, 1)
            nested = O.OptimiserChain(clip, O.OptimiserChain(r, O.WeightDecay(0.1))).fused_plan()
            assert nested[0] is clip and nested[1].opts[0] is r and nested[2] == 1
            flat = O.OptimiserChain(clip, r, O.WeightDecay(0.1)).fused_plan()
            assert flat[0] is clip and flat[1].opts[0] is r and flat[1].opts[1].gamma == 0.1 and flat[2] is None
        assert O.OptimiserChain(O.ClipNorm(1.0, p=1), r).fused_plan() is None
        assert O.OptimiserChain(r, O.ClipNorm(1.0)).fused_plan() is None
    # RMSProp / AdaGrad: fused in the DDP engine only; the functional chains keep the per-leaf path
    for k in ("rmsprop", "adagrad"):
        r = R[k]()
        assert O.OptimiserChain(O.ClipNorm(1.0), r).fused_plan() is None
        assert O.OptimiserChain(r, O.WeightDecay(0.1)).fused_plan() is None
        assert O.OptimiserChain(O.ClipNorm(1.0), r).fused_plan(engine=True)[1] is r
        assert O.OptimiserChain(r, O.WeightDecay(0.1)).fused_plan(engine=True)[1].opts[0] is r


@pytest.mark.parametrize("spelling", ["nested", "flat"])
def test_update_through_clip_lion_decay_chain_equals_members(spelling):
    """``update`` / ``update_`` through the fused plan == the chain applied member by member."""
    from fluxmpi_amd import optimisers as O
    torch.manual_seed(6)
    ps = {"w": torch.randn(40, 7), "b": torch.randn(7) * 0.01}
    gs = {k: torch.randn_like(v) * (0.01 if k == "b" else 1.0) for k, v in ps.items()}

    def chain():
        if spelling == "nested":
            return O.OptimiserChain(O.ClipNorm(1.0), O.OptimiserChain(O.Lion(), O.WeightDecay(0.1)))
        return O.OptimiserChain(O.ClipNorm(1.0), O.Lion(), O.WeightDecay(0.1))

    assert chain().fused_plan() is not None
    st = O.setup(chain(), ps)
    st2, ps2 = O.setup(chain(), ps), {k: v.clone() for k, v in ps.items()}
    want = {k: v.clone() for k, v in ps.items()}
    ref = chain()
    rst = {k: ref.init(v) for k, v in ps.items()}
    p = ps
    for _ in range(3):
        st, p = O.update(st, p, gs)
        O.update_(st2, ps2, gs)
        for k in want:
            rst[k], dx = O.OptimiserChain.apply(ref, rst[k], want[k], gs[k])  # member by member
            want[k] = want[k] - dx
    for k in want:
        torch.testing.assert_close(p[k], want[k], rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(ps2[k], want[k], rtol=1e-6, atol=1e-7)
    s = st["w"].state  # the chain's tuple of member states
    if spelling == "nested":
        assert len(s) == 2 and s[0] is None and len(s[1]) == 2 and s[1][1] is None
        torch.testing.assert_close(s[1][0], rst["w"][1][0], rtol=1e-6, atol=1e-7)
    else:
        assert len(s) == 3 and s[0] is None and s[2] is None
        torch.testing.assert_close(s[1], rst["w"][1], rtol=1e-6, atol=1e-7)


def test_adjust_freeze_repr_and_checkpoint_of_new_states(tmp_path):
    from fluxmpi_amd import optimisers as O
    ps = {"w": torch.randn(4, 3)}
    gs = {"w": torch.randn(4, 3)}
    for k in NEW:
        rule = O.OptimiserChain(_rules()[k](), O.WeightDecay(0.1))
        st = O.setup(rule, ps)
        assert "tensor(4, 3)" in repr(st["w"]) and type(rule.opts[0]).__name__ in repr(st["w"])
        O.adjust_(st, 0.5, gamma=0.2)
        assert rule.opts[1].gamma == 0.2
        if k != "adadelta":
            assert rule.opts[0].eta == 0.5
        else:
            O.adjust_(st, rho=0.8)
            assert rule.opts[0].rho == 0.8 and not hasattr(rule.opts[0], "eta")
        O.freeze_(st)
        _, p1 = O.update(st, ps, gs)
        assert torch.equal(p1["w"], ps["w"])
        O.thaw_(st)
        st1, p1 = O.update(st, ps, gs)
        assert not torch.equal(p1["w"], ps["w"])
        f = tmp_path / f"{k}.pt"
        torch.save({"state": st1}, f)
        back = torch.load(f, weights_only=False)["state"]
        a, b = back["w"].state[0], st1["w"].state[0]
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y


def test_engine_runs_every_rule_on_cpu_like_the_functional_rule():
    """DDP (CPU tensors: the reference path) == the per-leaf rule, bare and behind ClipNorm with
    WeightDecay; AdaGrad / AMSGrad start at ϵ; AdaDelta has no learning rate to set."""
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP

    def mlp():
        torch.manual_seed(2)
        return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1))

    g = torch.Generator().manual_seed(9)
    x, y = torch.randn(16, 8, generator=g), torch.randn(16, 1, generator=g)
    for k in KINDS:
        for wrap in (lambda r: r, lambda r: O.OptimiserChain(O.ClipNorm(0.3), O.OptimiserChain(r, O.WeightDecay(0.1)))):
            m1, m2 = mlp(), mlp()
            ddp = DDP(m1, wrap(_rules()[k]()))
            ps = {n: p.detach().clone() for n, p in m2.named_parameters()}
            rule = wrap(_rules()[k]())
            st = O.setup(rule, ps)
            for _ in range(3):
                ((ddp(x) - y) ** 2).mean().backward()
                ddp.step()
                for n, p in m2.named_parameters():
                    p.data.copy_(ps[n])
                    p.grad = None
                ((m2(x) - y) ** 2).mean().backward()
                st, ps = O.update(st, ps, {n: p.grad.clone() for n, p in m2.named_parameters()})
            for n, p in m1.named_parameters():
                torch.testing.assert_close(p.detach(), ps[n], rtol=1e-5, atol=1e-6)
            if k == "adadelta":
                with pytest.raises(ValueError):
                    ddp.set_lr(0.1)
            else:
                ddp.set_lr(0.25)
                assert float(ddp.hyper[0]) == 0.25


def worker_lion():
    """DistributedOptimizer(Lion): every rank applies the sign of the SUMMED gradient's blend."""
    import fluxmpi_amd as FluxMPI
    from fluxmpi_amd import optimisers as O

    FluxMPI.Init()
    W, r = FluxMPI.total_workers(), FluxMPI.local_rank()
    g = torch.Generator().manual_seed(13)
    ps = {"w": torch.randn(20, 3, generator=g), "b": torch.randn(3, generator=g)}
    per_rank = [{"w": torch.randn(20, 3, generator=g), "b": torch.randn(3, generator=g)} for _ in range(W)]
    st = O.setup(FluxMPI.DistributedOptimizer(O.Lion(1e-2)), ps)
    single = O.setup(O.Lion(1e-2), ps)
    summed = {k: sum(pr[k] for pr in per_rank) for k in ps}
    p_d, p_s = ps, ps
    for _ in range(3):
        st, p_d = O.update(st, p_d, {k: v.clone() for k, v in per_rank[r].items()})
        single, p_s = O.update(single, p_s, summed)
    for k in ps:
        torch.testing.assert_close(p_d[k], p_s[k], rtol=1e-6, atol=1e-7)
        assert not torch.equal(p_d[k], ps[k])
        every = FluxMPI.allreduce_gradients({"x": p_d[k].clone()}, on_gpu=False)["x"]
        assert W == 2 and torch.equal(every, p_d[k] * 2)  # identical on both ranks
    FluxMPI.Finalize()


def test_distributed_optimizer_lion(spmd):
    spmd("tests.test_rules:worker_lion", nprocs=2)
