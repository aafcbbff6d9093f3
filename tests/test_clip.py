"""Gradient clipping on the CPU paths: the ``ops.optim`` fallbacks, the fused clip chains of
``optimisers`` on CPU leaves (which keep the per-leaf path), the DDP engine with a ClipNorm chain
and with ``clip_global_norm``, and ``DistributedOptimizer`` over gloo (the clip sees the SUMMED
gradient)."""
import pytest
import torch


def _leaves(seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).to(dtype) for n in (1, 7, 300, 0, 4097)]


def test_sumsq_cpu_matches_torch():
    from fluxmpi_amd.ops import optim
    gs = _leaves()
    out, sc = torch.empty(len(gs)), torch.empty(len(gs))
    optim.sumsq_(gs, out, scales=sc, omega=2.0, grad_scale=0.5)
    want = torch.stack([(g * g).sum() for g in gs])
    torch.testing.assert_close(out, want, rtol=1e-6, atol=0)
    torch.testing.assert_close(sc, torch.clamp(2.0 / (0.5 * want.sqrt()), max=1.0), rtol=1e-6, atol=0)
    assert sc[3] == 1.0  # the empty leaf: norm 0 -> scale 1, no NaN
    torch.testing.assert_close(optim.sumsq_reference(gs).float(), want, rtol=1e-6, atol=0)
    slot = torch.zeros(3)
    optim.clip_total_(out, slot, omega=1.0, grad_scale=0.5)
    optim.clip_total_(out, slot, accumulate=True, omega=1.0, grad_scale=0.5)
    nrm = 0.5 * (2 * want.sum()).sqrt()
    torch.testing.assert_close(slot, torch.stack([2 * want.sum(), nrm, torch.clamp(1.0 / nrm, max=1.0)]))
    optim.clip_total_(out, slot)  # omega 0: no clip, the sum starts afresh
    assert slot[2] == 1.0 and torch.allclose(slot[0], want.sum())


def test_sumsq_edge_values_cpu():
    from fluxmpi_amd.ops import optim
    gs = [torch.zeros(5), torch.tensor([1.0, float("nan")]), torch.tensor([float("inf"), 1.0])]
    out, sc = torch.empty(3), torch.empty(3)
    optim.sumsq_(gs, out, scales=sc, omega=1.0)
    assert sc[0] == 1.0 and torch.isnan(sc[1]) and sc[2] == 0.0


@pytest.mark.parametrize("kind", ["adam", "descent", "momentum", "nesterov"])
def test_clip_keywords_cpu(kind):
    """tscale / clip_delta / dev_gscale on CPU tensors == the same call on pre-clipped gradients."""
    from fluxmpi_amd.ops import optim
    P = [t for t in _leaves(1) if t.numel()]
    G = [t for t in _leaves(2) if t.numel()]
    ts = torch.tensor([0.5, 1.0, 0.25, 0.125])
    dg = torch.tensor([0.75])
    delta = 0.3
    pre = [torch.clamp(g * 0.5 * 0.75 * s, -delta, delta) for g, s in zip(G, ts)]
    outs = []
    for clipped in (True, False):
        p = [t.clone() for t in P]
        m = [torch.zeros_like(t) for t in P]
        v = [torch.zeros_like(t) for t in P]
        kw = dict(grad_scale=0.5, tscale=ts, clip_delta=delta, dev_gscale=dg) if clipped else {}
        g = G if clipped else pre
        for _ in range(2):
            if kind == "adam":
                optim.adam_(p, g, m, v, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, bc1=0.1, bc2=0.001,
                            weight_decay=0.01, **kw)
            else:
                optim.sgd_(p, g, m, lr=0.1, momentum=0.0 if kind == "descent" else 0.9, nesterov=kind == "nesterov",
                           **kw)
        outs.append(p + m + v)
    for a, b in zip(*outs):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)


def _chains():
    from fluxmpi_amd import optimisers as O
    return {"clipnorm_adam": lambda: O.OptimiserChain(O.ClipNorm(0.5), O.Adam(1e-2)),
            "clipnorm_adamw": lambda: O.OptimiserChain(O.ClipNorm(0.5), O.AdamW(1e-2, decay=0.1)),
            "clipgrad_momentum": lambda: O.OptimiserChain(O.ClipGrad(0.01), O.Momentum())}


def _manual_step(name, x, g, st, t):
    """One hand-written step of chain ``name`` on one leaf; st: dict of moments. Returns new x."""
    if name.startswith("clipnorm"):
        g = g * torch.clamp(0.5 / torch.linalg.vector_norm(g), max=1.0)
    else:
        g = torch.clamp(g, -0.01, 0.01)
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731
    if name == "clipgrad_momentum":
        st["v"] = f32(0.9) * st["v"] + f32(0.01) * g
        return x - st["v"]
    b1, b2 = f32(0.9), f32(0.999)
    st["m"] = b1 * st["m"] + (1 - b1) * g
    st["v"] = b2 * st["v"] + (1 - b2) * g * g
    dx = st["m"] / (1 - f32(b1 ** t)) / (torch.sqrt(st["v"] / (1 - f32(b2 ** t))) + f32(1e-8)) * f32(1e-2)
    if name == "clipnorm_adamw":
        dx = dx + f32(0.1) * x
    return x - dx


@pytest.mark.parametrize("name", ["clipnorm_adam", "clipnorm_adamw", "clipgrad_momentum"])
def test_clip_chains_cpu_match_manual_loop(name):
    from fluxmpi_amd import optimisers as O
    torch.manual_seed(3)
    ps = {"w": torch.randn(40, 7), "b": torch.randn(7) * 0.01, "s": torch.randn(1)}
    gs = {k: torch.randn_like(v) * (0.001 if k == "b" else 1.0) for k, v in ps.items()}
    rule = _chains()[name]()
    st = O.setup(rule, ps)
    want = {k: v.clone() for k, v in ps.items()}
    mom = {k: {"m": torch.zeros_like(v), "v": torch.zeros_like(v)} for k, v in ps.items()}
    for t in range(1, 4):
        st, ps = O.update(st, ps, gs)
        for k in want:
            want[k] = _manual_step(name, want[k], gs[k], mom[k], t)
    for k in ps:
        torch.testing.assert_close(ps[k], want[k], rtol=1e-5, atol=1e-6)
    # the chain's tuple-of-member-states layout
    s = st["w"].state
    assert isinstance(s, tuple) and len(s) == 2 and s[0] is None
    if name == "clipnorm_adamw":
        assert isinstance(s[1], tuple) and len(s[1]) == 2 and len(s[1][0]) == 3 and s[1][1] is None
    elif name == "clipnorm_adam":
        assert len(s[1]) == 3
    else:
        assert isinstance(s[1], torch.Tensor)


def test_flat_three_rule_chain_and_fallbacks_cpu():
    """(ClipNorm, Adam, WeightDecay) spelled flat equals the nested form; p != 2 and a clip behind
    the update rule keep the generic per-leaf path (and its results)."""
    from fluxmpi_amd import optimisers as O
    torch.manual_seed(4)
    ps = {"w": torch.randn(30, 5), "b": torch.randn(5)}
    gs = {k: torch.randn_like(v) for k, v in ps.items()}
    flat = O.OptimiserChain(O.ClipNorm(0.5), O.Adam(1e-2), O.WeightDecay(0.1))
    nested = O.OptimiserChain(O.ClipNorm(0.5), O.AdamW(1e-2, decay=0.1))
    assert flat.fused_plan() is not None and nested.fused_plan() is not None
    sf, sn, pf, pn = O.setup(flat, ps), O.setup(nested, ps), ps, ps
    for _ in range(3):
        sf, pf = O.update(sf, pf, gs)
        sn, pn = O.update(sn, pn, gs)
    for k in ps:
        torch.testing.assert_close(pf[k], pn[k], rtol=1e-6, atol=1e-7)
    assert len(sf["w"].state) == 3 and sf["w"].state[0] is None and sf["w"].state[2] is None
    assert O.OptimiserChain(O.ClipNorm(0.5, p=1), O.Adam()).fused_plan() is None
    assert O.OptimiserChain(O.Adam(), O.ClipNorm(0.5)).fused_plan() is None
    assert O.OptimiserChain(O.ClipNorm(0.5), O.RMSProp()).fused_plan() is None


def _mlp(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(), torch.nn.Linear(16, 16), torch.nn.Tanh(),
                               torch.nn.Linear(16, 1))


def _functional_steps(model, rule, x, y, steps, pre=None):
    """``steps`` functional updates of a copy of ``model``'s parameters; ``pre(grads)`` rescales."""
    from fluxmpi_amd import optimisers as O
    ps = {n: p.detach().clone() for n, p in model.named_parameters()}
    st = O.setup(rule, ps)
    norms = []
    for _ in range(steps):
        for n, p in model.named_parameters():
            p.data.copy_(ps[n])
            p.grad = None
        ((model(x) - y) ** 2).mean().backward()
        grads = {n: p.grad.clone() for n, p in model.named_parameters()}
        if pre is not None:
            norms.append(pre(grads))
        st, ps = O.update(st, ps, grads)
    return ps, norms


def _global_prescale(w):
    def pre(grads):
        nrm = torch.sqrt(sum(g.double().pow(2).sum() for g in grads.values()))
        s = min(1.0, w / float(nrm))
        for g in grads.values():
            g.mul_(s)
        return float(nrm)
    return pre


@pytest.mark.parametrize("grad_mode,overlap_opt", [("steal", False), ("view", False), ("steal", True)])
def test_ddp_cpu_clipnorm_chain_matches_functional(grad_mode, overlap_opt):
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    w = 0.05
    m1, m2 = _mlp(5), _mlp(5)
    d = DDP(m1, O.OptimiserChain(O.ClipNorm(w), O.Adam(1e-2)), bucket_mb=0.001, first_bucket_mb=0.0005,
            grad_mode=grad_mode, overlap=True, overlap_opt=overlap_opt)
    assert len(d.buckets) > 1 and d.overlap_opt == overlap_opt
    x = torch.randn(16, 8)
    y = x.sum(1, keepdim=True).sin()
    for _ in range(4):
        ((d(x) - y) ** 2).mean().backward()
        d.step()
    scales = torch.cat([b.clip[1] for b in d.buckets])
    assert (scales < 1).any() and (scales == 1).any()
    ps, _ = _functional_steps(m2, O.OptimiserChain(O.ClipNorm(w), O.Adam(1e-2)), x, y, 4)
    for n, p in m1.named_parameters():
        torch.testing.assert_close(p.detach(), ps[n], rtol=1e-5, atol=1e-6)
    st = d.optimiser_state()
    leaf = st["0.weight"]
    assert leaf.state[0] is None and len(leaf.state[1]) == 3 and leaf.state[1][0].shape == (16, 8)
    assert d.grad_norm().dim() == 0 and d.grad_norm().dtype == torch.float32


def test_ddp_cpu_clip_global_norm_matches_functional():
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    w = 0.1
    m1, m2 = _mlp(6), _mlp(6)
    d = DDP(m1, O.Momentum(0.05, 0.9), bucket_mb=0.001, first_bucket_mb=0.0005, clip_global_norm=w)
    x = torch.randn(16, 8)
    y = x.sum(1, keepdim=True).sin()
    got = []
    for _ in range(4):
        ((d(x) - y) ** 2).mean().backward()
        d.step()
        got.append(float(d.grad_norm()))
    ps, norms = _functional_steps(m2, O.Momentum(0.05, 0.9), x, y, 4, pre=_global_prescale(w))
    assert max(norms) > w  # the clip is active
    for n, p in m1.named_parameters():
        torch.testing.assert_close(p.detach(), ps[n], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(torch.tensor(got), torch.tensor(norms), rtol=1e-5, atol=0)


def test_ddp_clip_argument_errors():
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    with pytest.raises(ValueError):
        DDP(_mlp(7), O.Adam(), clip_global_norm=1.0, overlap_opt=True)
    with pytest.raises(ValueError):
        DDP(_mlp(7), O.OptimiserChain(O.ClipNorm(1.0), O.Adam()), clip_global_norm=1.0)
    with pytest.raises(RuntimeError):
        DDP(_mlp(7), O.Adam()).grad_norm()
    with pytest.raises(TypeError):
        DDP(_mlp(7), O.OptimiserChain(O.ClipNorm(1.0, p=1), O.Adam()))
    d = DDP(_mlp(7), O.OptimiserChain(O.ClipGrad(0.1), O.Descent(0.1)), clip_global_norm=1.0)  # allowed
    assert d.overlap_opt is False


def worker_clip():
    """DistributedOptimizer(OptimiserChain(ClipNorm, Adam)): the clip sees the summed gradient."""
    import fluxmpi_amd as FluxMPI
    from fluxmpi_amd import optimisers as O

    FluxMPI.Init()
    W, r = FluxMPI.total_workers(), FluxMPI.local_rank()
    g = torch.Generator().manual_seed(11)
    ps = {"w": torch.randn(20, 3, generator=g), "b": torch.randn(3, generator=g)}
    per_rank = [{"w": torch.randn(20, 3, generator=g), "b": torch.randn(3, generator=g) * 0.01} for _ in range(W)]
    w = 0.5
    chain = lambda: O.OptimiserChain(O.ClipNorm(w), O.Adam(1e-2))  # noqa: E731
    st = O.setup(FluxMPI.DistributedOptimizer(chain()), ps)
    single = O.setup(chain(), ps)
    summed = {k: sum(pr[k] for pr in per_rank) for k in ps}
    norms = {k: float(torch.linalg.vector_norm(v)) for k, v in summed.items()}
    assert norms["w"] > w > norms["b"], norms  # one leaf clips, the other does not
    p_d, p_s = ps, ps
    for _ in range(3):
        st, p_d = O.update(st, p_d, {k: v.clone() for k, v in per_rank[r].items()})
        single, p_s = O.update(single, p_s, summed)
    for k in ps:
        torch.testing.assert_close(p_d[k], p_s[k], rtol=1e-5, atol=1e-6)
        # every rank ends with identical parameters: with two ranks, a + b == 2 a means b == a
        every = FluxMPI.allreduce_gradients({"x": p_d[k].clone()}, on_gpu=False)["x"]
        assert W == 2 and torch.equal(every, p_d[k] * 2)
    FluxMPI.Finalize()


def test_distributed_optimizer_clips_summed_gradient(spmd):
    spmd("tests.test_clip:worker_clip", nprocs=2)
