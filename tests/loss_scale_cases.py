"""Engine-level loss-scaling cases shared by ``test_loss_scale.py`` (CPU engine, reference path) and
``test_loss_scale_gpu.py`` (fused kernels): the same bodies, run on either device.

The gradients are handed to the engine directly (``p.grad = g``), from a CPU generator, so both
twins of a case see exactly the bits the case intends: ``g`` on one side, ``1024 * g`` (exact in
bf16 and fp32) on the other.
"""
import torch

SMALL = dict(bucket_mb=0.004, first_bucket_mb=0.002)  # several buckets for the 64-128-10 MLP


def mlp(seed, dev, dtype=torch.float32):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Linear(64, 128), torch.nn.Tanh(), torch.nn.Linear(128, 10))
    return m.to(dev).to(dtype)


def rule_of(name):
    from fluxmpi_amd import optimisers as O
    return {"adam": lambda: O.Adam(1e-2),
            "momentum": lambda: O.Momentum(0.05, 0.9),
            "clipnorm": lambda: O.OptimiserChain(O.ClipNorm(0.3), O.Adam(1e-2)),
            "global": lambda: O.Adam(1e-2),
            "lamb": lambda: O.LAMB(1e-2)}[name]()


def engine(name, dev, dtype, seed=0, **kw):
    from fluxmpi_amd.parallel.ddp import DDP
    if name == "global":
        kw["clip_global_norm"] = 0.5
    d = DDP(mlp(seed, dev, dtype), rule_of(name), **SMALL, **kw)
    assert len(d.buckets) > 1
    return d


def step_grads(d, step, mult=1.0):
    """Gradients of step ``step`` (a CPU generator: the same on every machine), times ``mult``. Leaf
    norms are 0.16 - 4.5, so the ClipNorm(0.3) chain clips three leaves of four and the global clip at
    0.5 is active."""
    g = torch.Generator().manual_seed(1000 + step)
    out = []
    for p in d.module.parameters():
        t = (torch.randn(p.shape, generator=g) * 0.05).to(p.dtype)
        out.append((t.float() * mult).to(p.dtype).to(p.device))
    return out


def give(d, grads):
    for p, g in zip(d.module.parameters(), grads):
        p.grad = g.clone()


def state(d):
    """Every tensor a step may write: parameters, masters, state buffers, beta^t, trust ratios."""
    out = [p.detach().clone() for p in d.module.parameters()] + [d.hyper.clone()]
    for b in d.buckets:
        out += [t.clone() for t in (b.master, b.exp_avg, b.exp_avg_sq, b.state3, b.ratios) if t is not None]
    return out


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def case_exact_unscaling(name, dev, dtype):
    """p.grad = g against loss_scale=1024 and p.grad = 1024 g: bit-identical after three steps."""
    a, b = engine(name, dev, dtype), engine(name, dev, dtype, loss_scale=1024.0)
    for t in range(3):
        give(a, step_grads(a, t))
        give(b, step_grads(b, t, 1024.0))
        a.step()
        b.step()
        if name in ("clipnorm", "global"):
            assert float(a.grad_norm()) > 0.5 and torch.equal(a.grad_norm(), b.grad_norm())
    assert same(state(a), state(b))
    assert float(b.loss_scale()) == 1024.0 and int(b.skipped_steps()) == 0 and int(b.step_skipped()) == 0
    if name == "clipnorm":
        sc = torch.cat([bk.clip[1] for bk in b.buckets])
        assert (sc < 1).any()  # the scales refer to the unscaled gradient: 1024 g would clip every leaf to 0.3/1024
        assert torch.equal(sc, torch.cat([bk.clip[1] for bk in a.buckets]))
    moved = [not torch.equal(p, q) for p, q in zip(b.module.parameters(), mlp(0, dev, dtype).parameters())]
    assert all(moved)


def case_skip(name, dev, dtype, bad=float("inf")):
    """One clean step, one with a single non-finite element, one clean step again."""
    from fluxmpi_amd import LossScale
    ls = LossScale(init=1024.0, interval=1000)
    d = engine(name, dev, dtype, loss_scale=ls)
    give(d, step_grads(d, 0, 1024.0))
    d.step()
    assert int(d.step_skipped()) == 0 and int(d.skipped_steps()) == 0 and float(d.loss_scale()) == 1024.0
    before = state(d)
    grads = step_grads(d, 1, 1024.0)
    grads[-2].view(-1)[3] = bad  # one element of one leaf
    give(d, grads)
    d.step()
    assert same(before, state(d)), "a skipped step wrote something"
    assert int(d.step_skipped()) == 1 and int(d.skipped_steps()) == 1 and float(d.loss_scale()) == 512.0
    # the next clean step equals the step a fresh twin takes from the same state
    twin = engine(name, dev, dtype, seed=5, loss_scale=LossScale(init=1024.0, interval=1000))
    twin.load_state_dict(d.state_dict())
    assert float(twin.loss_scale()) == 512.0 and int(twin.skipped_steps()) == 1
    for e in (d, twin):
        give(e, step_grads(e, 2, 512.0))
        e.step()
    assert same(state(d), state(twin)) and not same(before, state(d))
    assert int(d.step_skipped()) == 0 and int(d.skipped_steps()) == 1 and float(d.loss_scale()) == 512.0


def case_errors(dev):
    import pytest
    from fluxmpi_amd import LossScale
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    m = lambda: mlp(0, dev)  # noqa: E731
    with pytest.raises(ValueError):
        DDP(m(), O.Adam(), loss_scale="dynamic", overlap_opt=True)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            DDP(m(), O.Adam(), loss_scale=bad)
    with pytest.raises(ValueError):
        DDP(m(), O.Adam(), loss_scale="static")
    with pytest.raises(TypeError):
        DDP(m(), O.Adam(), loss_scale=True)
    for kw in (dict(init=0.0), dict(init=-1.0), dict(backoff=2.0, growth=0.5), dict(backoff=1.5), dict(backoff=0.0),
               dict(growth=0.5), dict(interval=0), dict(interval=2.5), dict(min_scale=0.0), dict(init=2.0 ** 30),
               dict(min_scale=8.0, max_scale=4.0, init=4.0), dict(init=float("nan"))):
        with pytest.raises(ValueError):
            LossScale(**kw)
    d = DDP(m(), O.Adam(), loss_scale="dynamic")
    assert d.overlap_opt is False and float(d.loss_scale()) == 2.0 ** 16
    give(d, step_grads(d, 0))
    with pytest.raises(RuntimeError):
        d.step(zero_grad=False)
    plain = DDP(m(), O.Adam())
    for read in (plain.loss_scale, plain.skipped_steps, plain.step_skipped):
        with pytest.raises(RuntimeError):
            read()
    x = torch.ones(3, device=dev)
    assert plain.scale_loss(x) is x  # no scale: the loss as it is
    # the accessors are 0-dim views on the engine's device, and scale_loss is a device product
    for t, dt in ((d.loss_scale(), torch.float32), (d.skipped_steps(), torch.int32), (d.step_skipped(), torch.int32)):
        assert t.dim() == 0 and t.dtype == dt and t.device.type == torch.device(dev).type
    assert torch.equal(d.scale_loss(x), x * 65536.0)
    assert d.scale_loss(x.half()).dtype == torch.float32  # 2^16 is beyond fp16
