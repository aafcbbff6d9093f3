"""LARS and LAMB (``optimisers.LARS`` / ``optimisers.LAMB``) on the CPU: the per-leaf rules against
formulas written out here in fp64, the 1-D leaves against Momentum / Adam, the edge ratios, the tree
API, and the DDP engine against the functional API and across two gloo ranks."""
import math

import pytest
import torch

from tests.test_ddp import _data, _mlp

LARS_KW = dict(eta=0.1, rho=0.9, trust=0.02, decay=1e-2, epsilon=1e-9)
LAMB_KW = dict(eta=1e-2, beta=(0.9, 0.999), epsilon=1e-6, decay=0.01)


def _r(dtype, v):
    """The hyperparameter as the rule holds it for a leaf of ``dtype`` (fp32 leaves round it to fp32)."""
    return float(torch.tensor(v, dtype=torch.float32)) if dtype == torch.float32 else v


def _lars_fp64(x, vel, g, dtype, eta, rho, trust, decay, epsilon):
    eta, rho, trust, decay, epsilon = (_r(dtype, v) for v in (eta, rho, trust, decay, epsilon))
    xn, gn = math.sqrt(float((x * x).sum())), math.sqrt(float((g * g).sum()))
    q = trust * xn / (gn + decay * xn + epsilon) if xn > 0 and gn > 0 else 1.0
    vel = rho * vel + eta * q * (g + decay * x)
    return x - vel, vel, q


def _lamb_fp64(x, m, v, g, t, dtype, eta, beta, epsilon, decay):
    eta, b1, b2, epsilon, decay = (_r(dtype, v_) for v_ in (eta, beta[0], beta[1], epsilon, decay))
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    u = m / (1 - b1 ** t) / (torch.sqrt(v / (1 - b2 ** t)) + epsilon) + decay * x
    xn, un = math.sqrt(float((x * x).sum())), math.sqrt(float((u * u).sum()))
    q = xn / un if xn > 0 and un > 0 else 1.0
    return x - eta * q * u, m, v, q


def _leaf_and_grads(dtype, seed=0, shape=(37, 11)):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64).to(dtype),
            [torch.randn(shape, generator=g, dtype=torch.float64).to(dtype) * 0.3 for _ in range(3)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_lars_apply_matches_fp64_formula(dtype):
    from fluxmpi_amd import optimisers as O
    x, grads = _leaf_and_grads(dtype)
    rule = O.LARS(**LARS_KW)
    st = rule.init(x)
    xr, vr = x.double(), torch.zeros_like(x, dtype=torch.float64)
    tol = dict(rtol=1e-12, atol=1e-12) if dtype == torch.float64 else dict(rtol=1e-5, atol=1e-6)
    for g in grads:
        st, d = rule.apply(st, x, g)
        x = x - d
        xr, vr, q = _lars_fp64(xr, vr, g.double(), dtype, **LARS_KW)
        assert 0 < q < 1
    torch.testing.assert_close(x.double(), xr, **tol)
    torch.testing.assert_close(st.double(), vr, **tol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_lamb_apply_matches_fp64_formula(dtype):
    from fluxmpi_amd import optimisers as O
    x, grads = _leaf_and_grads(dtype, seed=1)
    rule = O.LAMB(**LAMB_KW)
    st = rule.init(x)
    xr = x.double()
    mr, vr = torch.zeros_like(xr), torch.zeros_like(xr)
    tol = dict(rtol=1e-12, atol=1e-12) if dtype == torch.float64 else dict(rtol=1e-5, atol=1e-6)
    for t, g in enumerate(grads, 1):
        st, d = rule.apply(st, x, g)
        x = x - d
        xr, mr, vr, q = _lamb_fp64(xr, mr, vr, g.double(), t, dtype, **LAMB_KW)
        assert q > 0 and q != 1
    torch.testing.assert_close(x.double(), xr, **tol)
    torch.testing.assert_close(st[0].double(), mr, **tol)
    torch.testing.assert_close(st[1].double(), vr, **tol)
    b1, b2 = _r(dtype, 0.9), _r(dtype, 0.999)
    torch.testing.assert_close(torch.tensor(st[2], dtype=torch.float64), torch.tensor([b1 ** 4, b2 ** 4],
                                                                                     dtype=torch.float64),
                               rtol=1e-6 if dtype == torch.float32 else 1e-12, atol=0)


def _three_steps(rule, x, grads):
    st = rule.init(x)
    for g in grads:
        st, d = rule.apply(st, x, g)
        x = x - d
    return x, st


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_1d_leaf_is_the_base_rule_bitwise(name):
    from fluxmpi_amd import optimisers as O
    x, grads = _leaf_and_grads(torch.float32, seed=2, shape=(53,))
    if name == "lars":
        mine, base = O.LARS(**LARS_KW), O.Momentum(LARS_KW["eta"], LARS_KW["rho"])
        adapt = O.LARS(adapt_1d=True, **LARS_KW)
    else:
        mine, base = O.LAMB(**LAMB_KW), O.Adam(LAMB_KW["eta"], LAMB_KW["beta"], LAMB_KW["epsilon"])
        adapt = O.LAMB(adapt_1d=True, **LAMB_KW)
    x1, s1 = _three_steps(mine, x.clone(), grads)
    x2, s2 = _three_steps(base, x.clone(), grads)
    x3, _ = _three_steps(adapt, x.clone(), grads)
    assert torch.equal(x1, x2)
    if name == "lars":
        assert torch.equal(s1, s2)
    else:
        assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1]) and s1[2] == s2[2]
    assert not torch.allclose(x1, x3, rtol=1e-4, atol=1e-5)
    # a 0-dim leaf is 1-D too
    s = torch.tensor(0.7)
    a, _ = _three_steps(mine, s.clone(), [torch.tensor(0.1)] * 3)
    b, _ = _three_steps(base, s.clone(), [torch.tensor(0.1)] * 3)
    assert torch.equal(a, b)


def test_zero_leaves_have_ratio_one():
    """An all-zero parameter (ViT's cls token at the start) or, under LARS, an all-zero gradient:
    q == 1, i.e. the plain momentum / Adam-with-decay step."""
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.ops import optim
    g = torch.Generator().manual_seed(3)
    z, gr = torch.zeros(6, 5), torch.randn(6, 5, generator=g)
    # LARS, zero parameter: vel = eta * g
    st, d = O.LARS(**LARS_KW).apply(torch.zeros(6, 5), z, gr)
    torch.testing.assert_close(d, _r(torch.float32, LARS_KW["eta"]) * gr, rtol=1e-6, atol=0)
    # LARS, zero gradient: vel = eta * decay * x
    x = torch.randn(6, 5, generator=g)
    st, d = O.LARS(**LARS_KW).apply(torch.zeros(6, 5), x, torch.zeros(6, 5))
    torch.testing.assert_close(d, _r(torch.float32, LARS_KW["eta"]) * _r(torch.float32, LARS_KW["decay"]) * x,
                               rtol=1e-6, atol=0)
    # LAMB, zero parameter: Adam's first step, m/(1-b1) / (sqrt(v/(1-b2)) + eps) * eta
    rule = O.LAMB(**LAMB_KW)
    _, d = rule.apply(rule.init(z), z, gr)
    adam = O.Adam(LAMB_KW["eta"], LAMB_KW["beta"], LAMB_KW["epsilon"])
    _, da = adam.apply(adam.init(z), z, gr)
    torch.testing.assert_close(d, da, rtol=1e-6, atol=0)
    # the same through the multi-tensor references, which report the ratios
    ps, gs = [z.clone(), x.clone(), x.clone()], [gr.clone(), torch.zeros(6, 5), gr.clone()]
    q = torch.full((3,), -1.0)
    optim.lars_([p.clone() for p in ps], gs, [torch.zeros(6, 5) for _ in ps], lr=0.1, momentum=0.9, trust=0.02,
                weight_decay=0.01, eps=0.0, ratios=q)
    assert q[0] == 1 and q[1] == 1 and 0 < q[2] < 1
    q = torch.full((3,), -1.0)
    optim.lamb_([p.clone() for p in ps], gs, [torch.zeros(6, 5) for _ in ps], [torch.zeros(6, 5) for _ in ps],
                lr=0.01, beta1=0.9, beta2=0.999, eps=1e-6, bt1=0.9, bt2=0.999, weight_decay=0.01, ratios=q)
    assert q[0] == 1 and q[1] != 1 and q[2] != 1 and (q > 0).all()


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_setup_update_on_a_nested_tree(name):
    from fluxmpi_amd import optimisers as O
    g = torch.Generator().manual_seed(4)
    mk = (lambda: O.LARS(**LARS_KW)) if name == "lars" else (lambda: O.LAMB(**LAMB_KW))
    model = {"enc": {"w": torch.randn(9, 4, generator=g), "b": torch.randn(4, generator=g)},
             "head": [torch.randn(4, 3, generator=g), torch.randn(3, generator=g)]}
    grads = {"enc": {"w": torch.randn(9, 4, generator=g), "b": torch.randn(4, generator=g)},
             "head": [torch.randn(4, 3, generator=g), torch.randn(3, generator=g)]}
    st = O.setup(mk(), model)
    assert isinstance(st["enc"]["w"], O.Leaf) and isinstance(st["head"][1], O.Leaf)
    st2, m2 = O.update(st, model, grads)
    rule = mk()
    for x, gr, got, leaf in ((model["enc"]["w"], grads["enc"]["w"], m2["enc"]["w"], st2["enc"]["w"]),
                             (model["enc"]["b"], grads["enc"]["b"], m2["enc"]["b"], st2["enc"]["b"]),
                             (model["head"][0], grads["head"][0], m2["head"][0], st2["head"][0]),
                             (model["head"][1], grads["head"][1], m2["head"][1], st2["head"][1])):
        s, d = rule.apply(rule.init(x), x, gr)
        assert torch.equal(got, x - d)
        if name == "lamb":
            assert leaf.state[2] == s[2] and torch.equal(leaf.state[0], s[0])
        else:
            assert torch.equal(leaf.state, s)
    # update is out of place: the inputs are untouched
    assert not torch.equal(m2["enc"]["w"], model["enc"]["w"])
    assert float(st["enc"]["w"].state.abs().sum() if name == "lars" else st["enc"]["w"].state[0].abs().sum()) == 0


def test_adjust():
    from fluxmpi_amd import optimisers as O
    st = O.setup(O.LARS(**LARS_KW), {"w": torch.ones(2, 2)})
    O.adjust_(st, 0.5, trust=0.1, decay=0.0, rho=0.8)
    r = st["w"].rule
    assert (r.eta, r.trust, r.decay, r.rho) == (0.5, 0.1, 0.0, 0.8)
    st = O.setup(O.LAMB(**LAMB_KW), {"w": torch.ones(2, 2)})
    O.adjust_(st, 0.25, decay=0.3, beta=(0.8, 0.9), adapt_1d=True)
    r = st["w"].rule
    assert (r.eta, r.decay, r.beta, r.adapt_1d) == (0.25, 0.3, (0.8, 0.9), True)


def test_exports_and_chains():
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    assert "LARS" in O.__all__ and "LAMB" in O.__all__
    # behind a clip the functional API takes the per-leaf path; the engine has no fused form
    chain = O.OptimiserChain(O.ClipNorm(0.1), O.LAMB(**LAMB_KW))
    assert chain.fused_plan() is None and chain.fused_plan(engine=True) is None
    with pytest.raises(TypeError, match="no fused kernel"):
        DDP(_mlp(0), chain)
    with pytest.raises(TypeError, match="no fused kernel"):
        DDP(_mlp(0), O.OptimiserChain(O.ClipGrad(0.1), O.LARS(**LARS_KW)))
    with pytest.raises(ValueError):
        DDP(_mlp(0), O.LARS(**LARS_KW), clip_global_norm=1.0)


@pytest.mark.parametrize("grad_mode", ["steal", "view"])
@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_ddp_world1_matches_functional(name, grad_mode):
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    mk = (lambda: O.LARS(**LARS_KW)) if name == "lars" else (lambda: O.LAMB(**LAMB_KW))
    m1, m2 = _mlp(0), _mlp(0)
    ddp = DDP(m1, mk(), bucket_mb=0.001, first_bucket_mb=0.0005, grad_mode=grad_mode)  # several tiny buckets
    assert len(ddp.buckets) > 1
    ps = {n: p.detach().clone() for n, p in m2.named_parameters()}
    st = O.setup(mk(), ps)
    x, y = _data(0)
    for _ in range(3):
        ((ddp(x) - y) ** 2).mean().backward()
        ddp.step()
        for n, p in m2.named_parameters():
            p.data.copy_(ps[n])
            p.grad = None
        ((m2(x) - y) ** 2).mean().backward()
        st, ps = O.update(st, ps, {n: p.grad for n, p in m2.named_parameters()})
    for n, p in m1.named_parameters():
        torch.testing.assert_close(p.detach(), ps[n], rtol=1e-5, atol=1e-6)
    tr = ddp.trust_ratios()
    assert sorted(tr) == sorted(n for n, p in m1.named_parameters() if p.ndim > 1)
    assert all(t.dim() == 0 and float(t) > 0 and float(t) != 1 for t in tr.values())
    leaf = ddp.optimiser_state()["0.weight"]
    if name == "lamb":
        torch.testing.assert_close(leaf.state[0], st["0.weight"].state[0], rtol=1e-4, atol=1e-6)
        assert len(leaf.state) == 3 and len(leaf.state[2]) == 2
    else:
        torch.testing.assert_close(leaf.state, st["0.weight"].state, rtol=1e-4, atol=1e-6)
    sd = ddp.state_dict()
    assert set(sd["buckets"][0]) == {"master", "m", "v"}
    ddp.load_state_dict(sd)


def worker_lamb_ranks_agree():
    """Two ranks, different data: after three LAMB steps the parameters and the trust ratios are the
    same bits on every rank (each rank forms the ratios on its own replica, in a fixed order)."""
    import fluxmpi_amd as FluxMPI
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP

    FluxMPI.Init()
    r, W = FluxMPI.local_rank(), FluxMPI.total_workers()
    model = _mlp(1000 + r)
    ddp = DDP(model, O.LAMB(**LAMB_KW), bucket_mb=0.001, first_bucket_mb=0.0005, overlap=True)
    x, y = _data(r)
    for _ in range(3):
        ((ddp(x) - y) ** 2).mean().backward()
        ddp.step()
    for p in model.parameters():
        g = FluxMPI.allgather(p.detach().clone())
        assert all(torch.equal(g[0], g[i]) for i in range(W))
    tr = ddp.trust_ratios()
    assert len(tr) == 3
    q = torch.stack([tr[n] for n in sorted(tr)])
    assert bool((q > 0).all()) and bool((q != 1).all())
    g = FluxMPI.allgather(q.clone())
    assert all(torch.equal(g[0], g[i]) for i in range(W))
    FluxMPI.Finalize()


def test_lamb_two_ranks_bit_identical(spmd):
    spmd("tests.test_layerwise:worker_lamb_ranks_agree", nprocs=2)
