"""Dynamic loss scaling and the non-finite step skip on the CPU engine (the reference path of
``ops.optim``): exact unscaling, the skip, the scaler's rule, the errors, the checkpoint state and
two ranks over gloo that must reach one decision from one rank's inf."""
import pytest
import torch

from tests import loss_scale_cases as LS


# ---------------------------------------------------------------- ops: the references
def test_check_finite_reference_is_per_element_and_sticky():
    from fluxmpi_amd.ops import optim
    flag = torch.zeros(1, dtype=torch.int32)
    big = [torch.tensor([1e20, -1e20, 0.0, 1e-45]), torch.zeros(0), torch.tensor([3e38], dtype=torch.bfloat16)]
    optim.check_finite_(big, flag)
    assert int(flag) == 0  # finite, though every square is inf
    out = torch.zeros(3)
    optim.sumsq_(big[:2], out, flag=flag)
    assert torch.isinf(out[0]) and int(flag) == 0
    for bad in (float("inf"), float("-inf"), float("nan")):
        flag.zero_()
        optim.check_finite_([torch.ones(5), torch.tensor([1.0, bad])], flag)
        assert int(flag) == 1
        optim.check_finite_([torch.ones(5)], flag)
        assert int(flag) == 1  # sticky
        flag.zero_()
        optim.sumsq_([torch.ones(5), torch.tensor([1.0, bad])], out, flag=flag)
        assert int(flag) == 1


def test_sumsq_dev_pre_and_clip_total_reference():
    from fluxmpi_amd.ops import optim
    g = torch.Generator().manual_seed(0)
    gs = [torch.randn(n, generator=g) for n in (5, 100, 1)]
    pre = torch.tensor([2.0 ** -10])
    a, b = torch.zeros(2, 3), torch.zeros(2, 3)
    optim.sumsq_(gs, a[0], scales=a[1], omega=1.0, grad_scale=0.5)
    optim.sumsq_([t * 1024 for t in gs], b[0], scales=b[1], omega=1.0, grad_scale=0.5, dev_pre=pre)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0] * 2.0 ** 20, b[0])
    sa, sb = torch.zeros(3), torch.zeros(3)
    optim.clip_total_(a[0], sa, omega=1.0, grad_scale=0.5)
    optim.clip_total_(b[0], sb, omega=1.0, grad_scale=0.5, dev_pre=pre)
    assert torch.equal(sa[1], sb[1]) and torch.equal(sa[2] * 2.0 ** -10, sb[2]) and float(sa[2]) < 1
    optim.clip_total_(b[0], sb, dev_pre=pre)
    assert float(sb[2]) == 2.0 ** -10  # no clip: the inverse scale alone


def scaler_script(update, dev="cpu"):
    """A scripted flag sequence with interval 3 against hand-written expectations: (flag, scale,
    tracker, skipped, last) after each update. Shared with the GPU test."""
    from fluxmpi_amd.ops import optim
    kw = dict(growth=2.0, backoff=0.5, interval=3, min_scale=4.0, max_scale=64.0)
    blk = optim.loss_scale_block(16.0, dev)
    f = blk.view(torch.float32)
    script = [(0, 16, 1, 0, 0), (0, 16, 2, 0, 0), (0, 32, 0, 0, 0),   # grows after three clean steps
              (0, 32, 1, 0, 0), (1, 16, 0, 1, 1),                      # halves, tracker reset
              (0, 16, 1, 1, 0), (1, 8, 0, 2, 1), (1, 4, 0, 3, 1), (1, 4, 0, 4, 1),  # stops at min_scale
              (0, 4, 1, 4, 0), (0, 4, 2, 4, 0), (0, 8, 0, 4, 0),
              (0, 8, 1, 4, 0), (0, 8, 2, 4, 0), (0, 16, 0, 4, 0),
              (0, 16, 1, 4, 0), (0, 16, 2, 4, 0), (0, 32, 0, 4, 0),
              (0, 32, 1, 4, 0), (0, 32, 2, 4, 0), (0, 64, 0, 4, 0),
              (0, 64, 1, 4, 0), (0, 64, 2, 4, 0), (0, 64, 0, 4, 0)]   # stops at max_scale
    for flag, scale, tracker, skipped, last in script:
        blk[optim.LS_FLAG] = flag
        update(blk, **kw)
        got = blk.cpu()
        gf = got.view(torch.float32)
        assert float(gf[optim.LS_SCALE]) == scale and float(gf[optim.LS_SCALE] * gf[optim.LS_INV]) == 1.0
        assert [int(got[i]) for i in (optim.LS_TRACKER, optim.LS_SKIPPED, optim.LS_LAST, optim.LS_FLAG)] == \
            [tracker, skipped, last, 0], (flag, got.tolist())
    # a static scale: growth = backoff = 1
    blk = optim.loss_scale_block(1024.0, dev)
    for flag in (0, 1, 0):
        blk[optim.LS_FLAG] = flag
        update(blk, growth=1.0, backoff=1.0, interval=1, min_scale=1024.0, max_scale=1024.0)
        assert float(blk.view(torch.float32)[optim.LS_SCALE]) == 1024.0 and int(blk[optim.LS_LAST]) == flag
    assert int(blk[optim.LS_SKIPPED]) == 1
    return f


def test_loss_scale_update_reference_follows_the_script():
    from fluxmpi_amd.ops import optim
    scaler_script(optim.loss_scale_update_)


@pytest.mark.parametrize("fn", ["adam", "sgd", "rule", "lars", "lamb", "advance"])
def test_references_honour_dev_skip(fn):
    from fluxmpi_amd.ops import optim
    g = torch.Generator().manual_seed(1)
    mk = lambda: [torch.randn(n, generator=g) for n in (7, 33)]  # noqa: E731
    p, gr, s1, s2 = mk(), mk(), [t.abs() for t in mk()], [t.abs() for t in mk()]
    q = torch.full((2,), 7.0)
    hyper = torch.tensor([1e-2, 0.9, 0.999])

    def call(skip):
        kw = dict(dev_skip=skip)
        if fn == "adam":
            optim.adam_(p, gr, s1, s2, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, bc1=0.1, bc2=0.001, **kw)
        elif fn == "sgd":
            optim.sgd_(p, gr, s1, lr=1e-2, momentum=0.9, **kw)
        elif fn == "rule":
            optim.rule_("adamax", p, gr, [s1, s2], lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, bt1=0.9, bt2=0.999, **kw)
        elif fn == "lars":
            optim.lars_(p, gr, s1, lr=0.1, momentum=0.9, trust=0.02, ratios=q, **kw)
        elif fn == "lamb":
            optim.lamb_(p, gr, s1, s2, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-6, bt1=0.9, bt2=0.999, ratios=q, **kw)
        else:
            optim.adam_advance_(hyper, 0.9, 0.999, **kw)

    every = lambda: [t.clone() for t in p + s1 + s2 + [q, hyper]]  # noqa: E731
    before = every()
    call(torch.ones(1, dtype=torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(before, every()))
    call(torch.zeros(1, dtype=torch.int32))
    assert not all(torch.equal(a, b) for a, b in zip(before, every()))
    with pytest.raises(TypeError):
        call(torch.ones(1))  # the predicate is an int32


# ---------------------------------------------------------------- engine
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["adam", "momentum", "clipnorm", "global", "lamb"])
def test_cpu_engine_exact_unscaling(name, dtype):
    LS.case_exact_unscaling(name, "cpu", dtype)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("name", ["adam", "momentum", "clipnorm", "global", "lamb"])
def test_cpu_engine_skips_a_non_finite_step(name, bad):
    LS.case_skip(name, "cpu", torch.float32, bad)


def test_cpu_engine_errors():
    LS.case_errors("cpu")


def test_a_finite_gradient_whose_square_overflows_is_not_skipped():
    """loss_scale=1.0, the plain guard of a bf16 / fp32 model: 1e20 is a finite gradient."""
    d = LS.engine("momentum", "cpu", torch.float32, loss_scale=1.0)
    before = LS.state(d)
    grads = LS.step_grads(d, 0)
    grads[0].view(-1)[0] = 1e20
    LS.give(d, grads)
    d.step()
    assert int(d.step_skipped()) == 0 and not LS.same(before, LS.state(d))


def test_no_sync_accumulation_between_two_steps():
    """Two backwards at ONE scale summed by autograd (the scale only changes in step())."""
    a, b = LS.engine("adam", "cpu", torch.float32), LS.engine("adam", "cpu", torch.float32, loss_scale=1024.0)
    x = torch.randn(2, 8, 64, generator=torch.Generator().manual_seed(3))
    for d in (a, b):
        with d.no_sync():
            d.scale_loss(d(x[0]).pow(2).mean()).backward()
        d.scale_loss(d(x[1]).pow(2).mean()).backward()
        d.step()
    assert LS.same(LS.state(a), LS.state(b))


def test_state_dict_round_trip_and_a_checkpoint_without_scaler_state():
    from fluxmpi_amd import LossScale
    ls = lambda: LossScale(init=256.0, interval=2)  # noqa: E731
    d = LS.engine("adam", "cpu", torch.float32, loss_scale=ls())
    for t, bad in enumerate((False, True, False)):
        grads = LS.step_grads(d, t, float(d.loss_scale()))
        if bad:
            grads[0].view(-1)[0] = float("nan")
        LS.give(d, grads)
        d.step()
    sd = d.state_dict()
    assert sd["loss_scale"] == {"scale": 128.0, "growth_tracker": 1, "skipped": 1}
    e = LS.engine("adam", "cpu", torch.float32, seed=9, loss_scale=ls())
    view = e.loss_scale()
    e.load_state_dict(sd)
    assert float(view) == 128.0 and int(e.skipped_steps()) == 1  # loaded in place: earlier views follow
    for eng in (d, e):
        LS.give(eng, LS.step_grads(eng, 7, 128.0))
        eng.step()
    assert LS.same(LS.state(d), LS.state(e)) and float(e.loss_scale()) == 256.0  # tracker 1 -> 2: grown
    # a checkpoint written without loss scaling loads with the constructor's values
    plain = LS.engine("adam", "cpu", torch.float32).state_dict()
    assert "loss_scale" not in plain
    e.load_state_dict(plain)
    assert float(e.loss_scale()) == 256.0 and int(e.skipped_steps()) == 0 and int(e.step_skipped()) == 0
    # and an engine without loss scaling loads one that has the state
    LS.engine("adam", "cpu", torch.float32).load_state_dict(sd)


# ---------------------------------------------------------------- two ranks over gloo
def worker_two_ranks():
    """Step 2: only rank 1's LOCAL gradient holds an inf. The reduced gradient is non-finite on both
    ranks, both skip, nothing moves, the scale halves on both; step 3 applies on both."""
    import fluxmpi_amd as FluxMPI
    from fluxmpi_amd import LossScale
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP

    FluxMPI.Init()
    W, r = FluxMPI.total_workers(), FluxMPI.local_rank()
    assert W == 2
    d = DDP(LS.mlp(0, "cpu"), O.Adam(1e-2), loss_scale=LossScale(init=1024.0, interval=1000), overlap=False,
            **LS.SMALL)
    assert d.communicate and len(d.buckets) > 1

    def agree(t):
        """Bit-identical on both ranks: with two ranks a + b == 2 a means b == a."""
        s = FluxMPI.allreduce_gradients({"x": t.detach().clone().float()}, on_gpu=False)["x"]
        return torch.equal(s, t.detach().float() * 2)

    x = torch.randn(W, 8, 64, generator=torch.Generator().manual_seed(5))[r]  # each rank its own batch
    for step in (1, 2, 3):
        d.scale_loss(d(x).pow(2).mean()).backward()
        if step == 2 and r == 1:
            next(d.module.parameters()).grad.view(-1)[0] = float("inf")
        before = LS.state(d)
        d.step()
        skipped = step == 2
        assert int(d.step_skipped()) == int(skipped) and int(d.skipped_steps()) == int(step >= 2)
        assert LS.same(before, LS.state(d)) == skipped, step
        assert float(d.loss_scale()) == (1024.0 if step == 1 else 512.0)
        assert agree(d.loss_scale().reshape(1))
        assert all(agree(p) for p in d.module.parameters())
    FluxMPI.Finalize()


def test_two_ranks_reach_one_decision(spmd):
    spmd("tests.test_loss_scale:worker_two_ranks", nprocs=2)
