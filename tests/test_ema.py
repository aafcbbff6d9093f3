"""Exponential moving average of the weights on the CPU (the reference path of ``ops.optim``): the
references themselves, the engine's bookkeeping (``DDP(ema=...)``: readers, ``ema_state_dict``,
``ema_weights``, checkpoints, errors), the functional API and two ranks over gloo that must keep one
average. The helpers are shared with ``test_ema_gpu.py``."""
import numpy as np
import pytest
import torch

from tests import loss_scale_cases as LS


# ---------------------------------------------------------------- shared helpers
def ct_of(dtype):
    return torch.float64 if dtype == torch.float64 else torch.float32


def assert_within_bound(got, e0, x, omd, what=""):
    """|got - (e0 + omd (x - e0)) in fp64| <= 2.5 eps max(|e0|, |x|) per element: the three roundings
    of the expression in the compute type, u M (1 + 4 omd) with u = eps / 2 and omd <= 1."""
    eps = torch.finfo(got.dtype).eps
    e64, x64 = e0.detach().cpu().double(), x.detach().cpu().double()
    ref = e64 + float(omd) * (x64 - e64)
    bound = 2.5 * eps * torch.maximum(e64.abs(), x64.abs())
    err = (got.detach().cpu().double() - ref).abs()
    assert bool((err <= bound).all()), (what, float((err - bound).max()))


def mlp(seed, dev, dtype=torch.float32, hidden=128):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Linear(64, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, 10))
    return m.to(dev).to(dtype)


def rule_of(name):
    from fluxmpi_amd import optimisers as O
    return {"adam": lambda: O.Adam(1e-2), "momentum": lambda: O.Momentum(0.05, 0.9), "lamb": lambda: O.LAMB(1e-2),
            "clipnorm_adam": lambda: O.OptimiserChain(O.ClipNorm(0.3), O.Adam(1e-2))}[name]()


def engine(name, dev, dtype, seed=0, hidden=128, **kw):
    from fluxmpi_amd.parallel.ddp import DDP
    d = DDP(mlp(seed, dev, dtype, hidden), rule_of(name), **LS.SMALL, **kw)
    assert len(d.buckets) > 1
    return d


def sources(d):
    """{name: view of what the average follows}: the fp32 master, else the parameter."""
    from fluxmpi_amd.parallel.ddp import _strided_view
    return {n: _strided_view(b.master if b.master is not None else b.flat_param, p, o)
            for b in d.buckets for n, p, o in zip(b.names, b.params, b.offsets)}


def omd_of(d):
    """1 - d_t of the coming EMA update, in fp32 as the block holds it."""
    return (1.0 - d.ema_decay()).cpu()


def ema_bits(d):
    return [b.ema.clone() for b in d.buckets] + [d._ema_block.clone()]


def train_step(d, t, mult=1.0):
    LS.give(d, LS.step_grads(d, t, mult))
    d.step()


def advance_script(advance, dev, ulps=0):
    """25 optimiser steps, step 13 skipped, against hand-written (n, k, hold) and d_t: with ``a`` the
    applied steps so far, n = a // every, k = a % every, hold = (k + 1 < every); d_t from n."""
    from fluxmpi_amd.ops import optim
    one = np.float32(1.0)
    for every, decay in ((1, 0.7), (3, 0.3)):  # the warmup ramp (1 + n) / (10 + n) crosses either decay on the way
        for warmup in (True, False):
            blk = optim.ema_block(decay, warmup, every, dev)
            skip = torch.zeros(1, dtype=torch.int32, device=dev)
            applied, crossed = 0, set()

            def check():
                n, k = applied // every, applied % every
                got = blk.cpu()
                assert [int(got[i]) for i in (optim.EMA_UPDATES, optim.EMA_SINCE, optim.EMA_HOLD)] == \
                    [n, k, int(k + 1 < every)], (every, warmup, applied, got.tolist())
                ramp = np.float32(1 + n) / np.float32(10 + n)
                d = min(np.float32(decay), ramp) if warmup else np.float32(decay)
                crossed.add(bool(warmup and ramp < np.float32(decay)))
                f = got.view(torch.float32).numpy()
                for have, want in ((f[optim.EMA_DECAY], d), (f[optim.EMA_OMD], one - d)):
                    assert abs(np.float64(have) - np.float64(want)) <= ulps * np.spacing(np.float32(want)), \
                        (every, warmup, applied, have, want)

            check()  # the fresh block holds the first step's values
            for step in range(1, 26):
                skip.fill_(1 if step == 13 else 0)
                before = blk.clone()
                advance(blk, decay=decay, warmup=warmup, every=every, dev_skip=skip)
                if step == 13:
                    assert torch.equal(before, blk)
                else:
                    applied += 1
                check()
            assert crossed == ({True, False} if warmup else {False})
    with pytest.raises(TypeError):
        advance(torch.zeros(8, device=dev), decay=0.5, warmup=True, every=1)
    with pytest.raises(ValueError):
        advance(optim.ema_block(0.5, True, 1, dev), decay=0.5, warmup=True, every=0)


# ---------------------------------------------------------------- ops: the references
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_ema_reference_against_fp64(dtype):
    from fluxmpi_amd.ops import optim
    g = torch.Generator().manual_seed(0)
    ct = ct_of(dtype)
    xs = [torch.randn(n, generator=g).to(dtype) for n in (1, 33, 0, 4097)]
    for decay in (0.9999, 0.9, 0.0):
        es = [torch.randn(x.numel(), generator=g, dtype=torch.float64).to(ct) for x in xs]
        e0 = [e.clone() for e in es]
        optim.ema_reference_(es, xs, decay=decay)
        omd = float(torch.tensor(1.0 - decay, dtype=torch.float64).to(ct))
        for e, a, x in zip(es, e0, xs):
            assert e.dtype == ct
            assert_within_bound(e, a, x, omd, (dtype, decay))
    # x == e keeps the bits whatever omd is; the block's omd wins over the host's; hold and skip call it off
    same = [x.to(ct) for x in xs]
    optim.ema_reference_(same, xs, decay=0.123)
    assert all(torch.equal(a, x.to(ct)) for a, x in zip(same, xs))
    blk = optim.ema_block(0.75, False, 1, "cpu")
    a, b = [torch.zeros(33, dtype=ct)], [torch.zeros(33, dtype=ct)]
    optim.ema_reference_(a, [xs[1]], decay=0.0, dev_block=blk)
    optim.ema_reference_(b, [xs[1]], decay=0.75)
    assert torch.equal(a[0], b[0]) and torch.equal(a[0], 0.25 * xs[1].to(ct))
    blk[optim.EMA_HOLD] = 1
    optim.ema_reference_(a, [xs[1]], dev_block=blk)
    optim.ema_(a, [xs[1]], decay=0.5, dev_skip=torch.ones(1, dtype=torch.int32))
    assert torch.equal(a[0], b[0])
    with pytest.raises(TypeError):
        optim.ema_([torch.zeros(33, dtype=torch.float64 if ct == torch.float32 else torch.float32)], [xs[1]], decay=0.5)
    with pytest.raises(TypeError):
        optim.ema_([torch.zeros(32, dtype=ct)], [xs[1]], decay=0.5)


def test_ema_advance_reference_follows_the_script():
    from fluxmpi_amd.ops import optim
    advance_script(optim.ema_advance_, "cpu")
    advance_script(optim.ema_advance_reference_, "cpu")
    with pytest.raises(ValueError):
        optim.ema_block(1.0, True, 1, "cpu")


# ---------------------------------------------------------------- engine
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["adam", "momentum"])
def test_cpu_engine_keeps_the_average(name, dtype):
    from fluxmpi_amd import EMA
    d = engine(name, "cpu", dtype, ema=EMA(decay=0.99))
    assert (d.buckets[0].master is not None) == (dtype == torch.bfloat16)
    mine = {n: x.detach().float().clone() for n, x in sources(d).items()}
    assert all(torch.equal(v, mine[n]) for n, v in d.ema_parameters().items())
    for t in range(3):
        omd = omd_of(d)
        assert float(omd) == float(np.float32(1) - min(np.float32(0.99), np.float32(1 + t) / np.float32(10 + t)))
        train_step(d, t)
        for n, x in sources(d).items():
            mine[n].add_(omd * (x.detach().float() - mine[n]))  # the reference path's expression: same bits
        got = d.ema_parameters()
        assert set(got) == {n for n, _ in d.module.named_parameters()}
        for n, p in d.module.named_parameters():
            assert got[n].shape == p.shape and got[n].dtype == torch.float32 and torch.equal(got[n], mine[n]), (t, n)
        assert int(d.ema_updates()) == t + 1
    assert not any(torch.equal(mine[n], x.float()) for n, x in sources(d).items())
    for r in (d.ema_decay(), d.ema_updates()):
        assert r.dim() == 0
    # the exported state dict: the module's keys and dtypes, the averages cast to them
    sd, live = d.ema_state_dict(), d.module.state_dict()
    assert list(sd) == list(live)
    for k in live:
        assert sd[k].dtype == live[k].dtype and sd[k].data_ptr() != live[k].data_ptr()
        assert torch.equal(sd[k], mine[k].to(dtype))


def test_ema_state_dict_leaves_buffers_and_frozen_parameters_alone():
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.BatchNorm1d(8), torch.nn.Linear(8, 2))
    m[2].bias.requires_grad_(False)
    d = DDP(m, O.Momentum(0.1, 0.9), ema=0.5)
    assert d._ema.decay == 0.5 and d._ema.warmup and d._ema.every == 1
    d(torch.randn(4, 8)).sum().backward()
    d.step()
    sd = d.ema_state_dict()
    assert list(sd) == list(m.state_dict())
    for k in ("1.running_mean", "1.running_var", "1.num_batches_tracked", "2.bias"):
        assert torch.equal(sd[k], m.state_dict()[k]) and sd[k].dtype == m.state_dict()[k].dtype
    assert float(m.state_dict()["1.running_mean"].abs().sum()) > 0
    assert not torch.equal(sd["0.weight"], m.state_dict()["0.weight"])
    assert set(d.ema_parameters()) == {"0.weight", "0.bias", "1.weight", "1.bias", "2.weight"}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ema_weights_round_trip(dtype):
    d, twin = engine("adam", "cpu", dtype, ema=0.9), engine("adam", "cpu", dtype, ema=0.9)
    for e in (d, twin):
        train_step(e, 0)
    before, avg = LS.state(d), ema_bits(d)
    with d.ema_weights() as m:
        assert m is d.module
        for n, p in d.module.named_parameters():
            assert torch.equal(p, d.ema_parameters()[n].to(dtype)) and p.dtype == dtype
        assert not LS.same([p.detach() for p in d.module.parameters()], before[:4])
        LS.give(d, LS.step_grads(d, 1))
        with pytest.raises(RuntimeError):
            d.step()
        with pytest.raises(RuntimeError):
            with d.ema_weights():
                pass
    assert LS.same(before, LS.state(d)) and LS.same(avg, ema_bits(d))
    for e in (d, twin):  # the step after the context: the step of an engine that never entered it
        train_step(e, 1)
    assert LS.same(LS.state(d), LS.state(twin)) and LS.same(ema_bits(d), ema_bits(twin))
    assert not LS.same(before, LS.state(d))


def test_outside_edits_do_not_reset_the_average():
    d = engine("adam", "cpu", torch.bfloat16, ema=0.9)
    train_step(d, 0)
    avg = ema_bits(d)
    with torch.no_grad():
        next(d.module.parameters()).mul_(2.0)
    d._sync_masters()
    assert LS.same(avg, ema_bits(d))


def test_errors_and_an_engine_without_ema():
    from fluxmpi_amd import EMA
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    for kw in (dict(decay=1.0), dict(decay=-0.1), dict(decay=float("nan")), dict(every=0), dict(every=1.5)):
        with pytest.raises(ValueError):
            EMA(**kw)
    for bad in (1.0, -0.5, 2):
        with pytest.raises(ValueError):
            DDP(mlp(0, "cpu"), O.Adam(), ema=bad)
    assert EMA() == EMA(decay=0.9999, warmup=True, every=1)
    plain = DDP(mlp(0, "cpu"), O.Adam())
    assert plain._ema_block is None and all(b.ema is None for b in plain.buckets)
    assert "ema" not in plain.state_dict()
    for read in (plain.ema_parameters, plain.ema_decay, plain.ema_updates, plain.ema_state_dict):
        with pytest.raises(RuntimeError):
            read()
    with pytest.raises(RuntimeError):
        with plain.ema_weights():
            pass


def test_every_and_step_without_zero_grad():
    from fluxmpi_amd import EMA
    d = engine("momentum", "cpu", torch.float32, ema=EMA(decay=0.5, warmup=False, every=2))
    moved = []
    for t in range(4):
        before = ema_bits(d)[:-1]
        LS.give(d, LS.step_grads(d, t))
        d.step(zero_grad=t != 1)
        moved.append(not LS.same(before, ema_bits(d)[:-1]))
    assert moved == [False, True, False, True] and int(d.ema_updates()) == 2


# ---------------------------------------------------------------- checkpoints
def test_state_dict_round_trip_and_a_checkpoint_without_an_average():
    from fluxmpi_amd import EMA
    mk = lambda seed: engine("adam", "cpu", torch.bfloat16, seed=seed, ema=EMA(decay=0.9, every=2))  # noqa: E731
    d = mk(0)
    for t in range(3):
        train_step(d, t)
    sd = d.state_dict()
    assert sd["ema"]["num_updates"] == 1 and sd["ema"]["since"] == 1 and len(sd["ema"]["buckets"]) == len(d.buckets)
    assert all(t.device.type == "cpu" and t.dtype == torch.float32 for t in sd["ema"]["buckets"])
    e = mk(9)
    views, n = e.ema_parameters(), e.ema_updates()
    e.load_state_dict(sd)
    assert int(n) == 1 and LS.same(ema_bits(d), ema_bits(e))  # loaded in place: earlier views follow
    assert all(torch.equal(views[k], v) for k, v in d.ema_parameters().items())
    for eng in (d, e):
        train_step(eng, 7)
    assert LS.same(LS.state(d), LS.state(e)) and LS.same(ema_bits(d), ema_bits(e)) and int(e.ema_updates()) == 2
    # a checkpoint written without an average: the average starts from the loaded masters, n = 0
    plain = engine("adam", "cpu", torch.bfloat16, seed=3)
    train_step(plain, 0)
    psd = plain.state_dict()
    assert "ema" not in psd
    e.load_state_dict(psd)
    assert int(e.ema_updates()) == 0 and float(e.ema_decay()) == float(np.float32(0.1))
    for b, pb in zip(e.buckets, plain.buckets):
        assert torch.equal(b.ema, pb.master) and torch.equal(b.master, pb.master)
    # and an engine without an average loads a checkpoint that has one
    engine("adam", "cpu", torch.bfloat16).load_state_dict(sd)


# ---------------------------------------------------------------- functional API
def test_functional_api_on_a_nested_tree():
    from fluxmpi_amd import FlatParams
    from fluxmpi_amd import optimisers as O
    g = torch.Generator().manual_seed(2)
    tied = torch.randn(5, 3, generator=g)
    ps = {"a": [torch.randn(7, generator=g), torch.randn(4, 3, 2, 2, generator=g).to(torch.bfloat16)
                .contiguous(memory_format=torch.channels_last)],
          "b": {"c": torch.randn(9, generator=g, dtype=torch.float64), "tied": tied},
          "t": tied, "n": 3, "i": torch.arange(4)}
    ema = O.ema_setup(ps)
    assert ema["a"][0].dtype == torch.float32 and ema["a"][1].dtype == torch.float32
    assert ema["a"][1].stride() == ps["a"][1].stride() and ema["b"]["c"].dtype == torch.float64
    assert ema["n"] is None and ema["i"] is None and ema["t"] is ema["b"]["tied"]
    assert torch.equal(ema["a"][1], ps["a"][1].float()) and ema["a"][0].data_ptr() != ps["a"][0].data_ptr()
    e0 = [t.clone() for t in (ema["a"][0], ema["a"][1], ema["b"]["c"], ema["t"])]
    new = {"a": [ps["a"][0] + 1, (ps["a"][1].float() * 0.5).to(torch.bfloat16)],
           "b": {"c": ps["b"]["c"] - 2, "tied": tied}, "t": tied, "n": 3, "i": ps["i"]}
    new["b"]["tied"] = new["t"] = tied * 3
    assert O.ema_update(ema, new, 0.9) is ema
    for e, a, x, dt in zip((ema["a"][0], ema["a"][1], ema["b"]["c"], ema["t"]), e0,
                           (new["a"][0], new["a"][1], new["b"]["c"], new["t"]),
                           (torch.float32, torch.float32, torch.float64, torch.float32)):
        assert_within_bound(e, a, x, float(torch.tensor(1.0 - 0.9, dtype=torch.float64).to(dt)))
        assert not torch.equal(e, a)
    # num_updates: the warmed-up decay min(decay, (1 + n) / (10 + n)) on the host
    a, b = O.ema_setup(ps), O.ema_setup(ps)
    O.ema_update(a, new, 0.9, num_updates=0)
    O.ema_update(b, new, 0.1)
    assert torch.equal(a["a"][0], b["a"][0])
    O.ema_update(a, new, 0.9, num_updates=1000)
    O.ema_update(b, new, 0.9)
    assert torch.equal(a["a"][0], b["a"][0])
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            O.ema_update(a, new, bad)
    # FlatParams: one flat leaf
    fp = FlatParams({"w": torch.randn(6, generator=g), "v": {"u": torch.randn(2, 2, generator=g)}})
    fe = O.ema_setup(fp)
    assert isinstance(fe, FlatParams) and fe.data.data_ptr() != fp.data.data_ptr() and torch.equal(fe.v.u, fp.v.u)
    old = fp.data.clone()
    fp.data.add_(1.0)
    O.ema_update(fe, fp, 0.75)
    assert torch.equal(fe.data, old + 0.25 * (fp.data - old)) and not torch.equal(fe.data, old)
    # a module: its named parameters
    m = mlp(0, "cpu")
    me = O.ema_setup(m)
    assert list(me) == [n for n, _ in m.named_parameters()]
    with torch.no_grad():
        m[0].bias.add_(1.0)
    O.ema_update(me, m, 0.5)
    assert torch.allclose(me["0.bias"], m[0].bias - 0.5) and torch.equal(me["0.weight"], m[0].weight)


# ---------------------------------------------------------------- two ranks over gloo
def worker_two_ranks():
    """Each rank its own batch; on step 2 only rank 1's LOCAL gradient holds an inf, both ranks skip.
    After four steps the averages and the update count have equal bits on both ranks: n == 3."""
    import fluxmpi_amd as FluxMPI
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP

    FluxMPI.Init()
    W, r = FluxMPI.total_workers(), FluxMPI.local_rank()
    assert W == 2
    d = DDP(mlp(r, "cpu"), O.Adam(1e-2), loss_scale="dynamic", ema=0.99, overlap=False, **LS.SMALL)  # seeds differ
    assert d.communicate and len(d.buckets) > 1

    def agree(t):
        """Bit-identical on both ranks: with two ranks a + b == 2 a means b == a."""
        s = FluxMPI.allreduce_gradients({"x": t.detach().clone().double()}, on_gpu=False)["x"]
        return torch.equal(s, t.detach().double() * 2)

    assert all(agree(v) for v in d.ema_parameters().values())  # the root's average, broadcast
    x = torch.randn(W, 8, 64, generator=torch.Generator().manual_seed(5))[r]
    for step in (1, 2, 3, 4):
        d.scale_loss(d(x).pow(2).mean()).backward()
        if step == 2 and r == 1:
            next(d.module.parameters()).grad.view(-1)[0] = float("inf")
        before = ema_bits(d)
        d.step()
        assert LS.same(before, ema_bits(d)) == (step == 2), step
    assert int(d.ema_updates()) == 3 and int(d.skipped_steps()) == 1
    assert agree(d.ema_updates().reshape(1)) and agree(d.ema_decay().reshape(1))
    assert all(agree(v) for v in d.ema_parameters().values())
    assert not any(torch.equal(v, p) for v, p in zip(d.ema_parameters().values(), d.module.parameters()))
    FluxMPI.Finalize()


def test_two_ranks_keep_one_average(spmd):
    spmd("tests.test_ema:worker_two_ranks", nprocs=2)
