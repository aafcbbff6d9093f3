"""The fused weight-EMA kernels (``csrc/kernels/optim_ema.hip``) and ``DDP(ema=...)`` on the GPU.

Elementwise: ``mt_ema`` over the 30-leaf set of the update kernels' tests (an empty leaf, 4097 and
100 elements, a multi-chunk leaf, leaves whose EMA and / or source miss 16-byte alignment, a second
launch group) against fp64 within the derived bound ``2.5 eps max(|e|, |x|)``, and exact cases. Then
the skip / hold predicates, ``ema_advance`` against the CPU test's script, and the engine."""
import pytest
import torch

from tests import loss_scale_cases as LS
from tests import test_ema as TE
from tests.test_clip_gpu import SIZES, UNALIGNED
from tests.test_rules_gpu import Guarded, _leaves

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64]
E_OFF = (UNALIGNED, 8)   # leaves whose EMA starts one element into its buffer (8: the 100-element leaf)
X_OFF = (UNALIGNED, 4)   # ... and whose source does (4: 4097 elements, the source alone)


def _pair(dtype, e_seed=1, x_seed=0):
    ct = TE.ct_of(dtype)
    E, X = Guarded(_leaves(e_seed), ct, E_OFF), Guarded(_leaves(x_seed), dtype, X_OFF)
    assert len(E.views) == 30 and E.views[14].numel() == 0 and SIZES[4] == 4097 and SIZES[8] == 100
    return E, X


# ---------------------------------------------------------------- 1. kernel against the reference
@pytest.mark.parametrize("omd", [1e-4, 0.1, 1.0])
@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_within_the_bound(gpu_ext, dtype, omd):
    from fluxmpi_amd.ops import optim
    ct = TE.ct_of(dtype)
    E, X = _pair(dtype)
    e0 = [v.cpu().clone() for v in E.views]
    x0 = [v.cpu().clone() for v in X.views]
    decay = 1.0 - omd
    optim.ema_(E.views, X.views, decay=decay)
    torch.cuda.synchronize()
    E.check()
    X.check()
    omd_c = torch.tensor(1.0 - decay, dtype=torch.float64).to(ct)  # as the launcher hands it to the kernel
    ref = [t.clone() for t in e0]
    optim.ema_reference_(ref, x0, decay=decay)
    moved = 0
    for i, (v, a, x) in enumerate(zip(E.views, e0, x0)):
        assert torch.equal(X.views[i].cpu(), x), "the source was written"
        got = v.cpu()
        TE.assert_within_bound(got, a, x, float(omd_c), (dtype, omd, i))
        if dtype == torch.float64:  # fp64: a reference in fp64, the same expression, the same bound
            err = (got - ref[i]).abs()
            assert bool((err <= 2.5 * torch.finfo(ct).eps * torch.maximum(a.abs(), x.abs())).all()), i
        moved += int((got != a).sum())
    assert moved > 0.9 * sum(SIZES) * (omd > 1e-3)


# ---------------------------------------------------------------- 2. exact cases
@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_source_keeps_the_bits(gpu_ext, dtype):
    from fluxmpi_amd.ops import optim
    ct = TE.ct_of(dtype)
    X = Guarded(_leaves(3), dtype, X_OFF)
    E = Guarded([v.cpu().to(ct) for v in X.views], ct, E_OFF)
    before = [v.clone() for v in E.views]
    for decay in (0.9999, 0.37, 0.0):
        optim.ema_(E.views, X.views, decay=decay)
    assert all(torch.equal(a, b) for a, b in zip(before, E.views))
    E.check()


@pytest.mark.parametrize("omd", [0.5, 0.25])
@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_values_give_the_exact_rational(gpu_ext, dtype, omd):
    from fluxmpi_amd.ops import optim
    ct = TE.ct_of(dtype)
    g = torch.Generator().manual_seed(7)
    ints = lambda: [torch.randint(-64, 65, (n,), generator=g).double() for n in SIZES]  # noqa: E731
    e0, x0 = ints(), ints()
    E, X = Guarded(e0, ct, E_OFF), Guarded(x0, dtype, X_OFF)
    optim.ema_(E.views, X.views, decay=1.0 - omd)
    for v, a, x in zip(E.views, e0, x0):
        assert torch.equal(v.cpu().double(), a + omd * (x - a))  # multiples of 1/4 below 2^7: exact in every format
    E.check()


def test_device_block_overrides_the_host_value(gpu_ext):
    from fluxmpi_amd.ops import optim
    E1, X = _pair(torch.bfloat16)
    E2, _ = _pair(torch.bfloat16)
    blk = optim.ema_block(0.75, False, 1, "cuda")
    optim.ema_(E1.views, X.views, decay=0.0, dev_block=blk)  # the host says omd = 1, the block 0.25
    optim.ema_(E2.views, X.views, decay=0.75)
    assert all(torch.equal(a, b) for a, b in zip(E1.views, E2.views))
    assert not torch.equal(E1.views[3], X.views[3].float())


def test_wrong_ema_dtype_raises(gpu_ext):
    from fluxmpi_amd.ops import optim
    x = torch.zeros(16, device="cuda", dtype=torch.bfloat16)
    for bad in (torch.bfloat16, torch.float64, torch.float16):
        with pytest.raises(TypeError):
            optim.ema_([torch.zeros(16, device="cuda", dtype=bad)], [x], decay=0.5)
    with pytest.raises(TypeError):
        optim.ema_([torch.zeros(16, device="cuda")], [x.double()], decay=0.5)
    with pytest.raises(TypeError):
        optim.ema_([torch.zeros(15, device="cuda")], [x], decay=0.5)
    with pytest.raises(TypeError):
        optim.ema_([torch.zeros(16, device="cuda")], [x], dev_block=torch.zeros(8, device="cuda"))
    with pytest.raises(ValueError):
        optim.ema_([torch.zeros(16, device="cuda")], [x])


# ---------------------------------------------------------------- 3. skip and hold
@pytest.mark.parametrize("which", ["skip", "hold"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float64])
def test_skip_and_hold_touch_nothing(gpu_ext, dtype, which):
    from fluxmpi_amd.ops import optim
    E, X = _pair(dtype)
    X.views[5].fill_(float("nan"))  # nothing of it may reach the result
    before = [v.clone() for v in E.views]
    blk = optim.ema_block(0.5, False, 2 if which == "hold" else 1, "cuda")
    skip = torch.full((1,), int(which == "skip"), dtype=torch.int32, device="cuda")
    assert int(blk[optim.EMA_HOLD]) == int(which == "hold")
    optim.ema_(E.views, X.views, dev_block=blk, dev_skip=skip)
    if which == "skip":
        optim.ema_(E.views, X.views, decay=0.5, dev_skip=skip)
    assert all(torch.equal(a, b) for a, b in zip(before, E.views))
    blk[optim.EMA_HOLD] = 0
    skip.zero_()
    optim.ema_(E.views, X.views, dev_block=blk, dev_skip=skip)  # and the same call, neither set, runs
    assert bool(torch.isnan(E.views[5]).all()) and not torch.equal(before[3], E.views[3])
    E.check()


def test_ema_advance_follows_the_script_on_the_device(gpu_ext):
    from fluxmpi_amd.ops import optim
    TE.advance_script(optim.ema_advance_, "cuda", ulps=1)


# ---------------------------------------------------------------- 4. engine
def _engine(name, dtype=torch.bfloat16, seed=0, **kw):
    return TE.engine(name, "cuda", dtype, seed=seed, hidden=96, **kw)


@pytest.mark.parametrize("name", ["adam", "momentum", "lamb", "clipnorm_adam"])
def test_engine_follows_the_masters(gpu_ext, name):
    from fluxmpi_amd.ops import optim
    d = _engine(name, ema=0.99)
    assert all(b.master is not None and b.ema.dtype == torch.float32 for b in d.buckets)
    mine = {n: x.detach().cpu().clone() for n, x in TE.sources(d).items()}
    for t in range(3):
        omd = float(d._ema_block.view(torch.float32)[optim.EMA_OMD])  # read before the step
        TE.train_step(d, t)
        got, src = d.ema_parameters(), TE.sources(d)
        for n in mine:
            x = src[n].detach().cpu()
            TE.assert_within_bound(got[n].cpu(), mine[n], x, omd, (name, t, n))
            optim.ema_reference_([mine[n]], [x], decay=1.0 - omd)  # the test's own running value
            assert not torch.equal(mine[n], x)
    assert int(d.ema_updates()) == 3 and abs(float(d.ema_decay()) - 4.0 / 13.0) < 1e-6
    sd = d.ema_state_dict()
    assert all(sd[k].dtype == torch.bfloat16 and sd[k].is_cuda for k in sd)
    assert all(torch.equal(sd[n], got[n].to(torch.bfloat16)) for n in got)


def test_loss_scale_skip_leaves_the_average(gpu_ext):
    d = _engine("adam", loss_scale="dynamic", ema=0.99)
    TE.train_step(d, 0, float(d.loss_scale()))
    before, n, dt = TE.ema_bits(d), int(d.ema_updates()), float(d.ema_decay())
    grads = LS.step_grads(d, 1, float(d.loss_scale()))
    grads[-2].view(-1)[3] = float("inf")
    LS.give(d, grads)
    d.step()
    assert int(d.step_skipped()) == 1
    assert LS.same(before, TE.ema_bits(d)) and int(d.ema_updates()) == n == 1 and float(d.ema_decay()) == dt
    TE.train_step(d, 2, float(d.loss_scale()))
    assert int(d.step_skipped()) == 0 and int(d.ema_updates()) == 2 and float(d.ema_decay()) != dt
    assert not any(torch.equal(a, b) for a, b in zip(before, TE.ema_bits(d)))


def test_every_two_moves_on_even_steps(gpu_ext):
    from fluxmpi_amd import EMA
    d = _engine("momentum", ema=EMA(decay=0.9, warmup=False, every=2))
    moved = []
    for t in range(4):
        before = TE.ema_bits(d)[:-1]
        TE.train_step(d, t)
        moved.append(not LS.same(before, TE.ema_bits(d)[:-1]))
    assert moved == [False, True, False, True] and int(d.ema_updates()) == 2


def _data(dtype):
    g = torch.Generator().manual_seed(11)
    return torch.randn(8, 64, generator=g).cuda().to(dtype), torch.randn(8, 10, generator=g).cuda()


def _loss(d, x, y):
    return torch.nn.functional.mse_loss(d(x).float(), y)


def test_overlap_opt_equals_step(gpu_ext):
    a, b = _engine("adam", ema=0.9, overlap_opt=False), _engine("adam", ema=0.9, overlap_opt=True)
    assert b.overlap_opt and b._opt_stream is not None and not a.overlap_opt
    x, y = _data(torch.bfloat16)
    for _ in range(3):
        for d in (a, b):
            _loss(d, x, y).backward()
            d.step()
    torch.cuda.synchronize()
    assert LS.same(LS.state(a), LS.state(b)) and LS.same(TE.ema_bits(a), TE.ema_bits(b))
    assert int(b.ema_updates()) == 3


def test_graphed_step_equals_eager(gpu_ext):
    from fluxmpi_amd import EMA
    from fluxmpi_amd.parallel.graph import GraphedStep
    mk = lambda: _engine("adam", ema=EMA(decay=0.99, every=2), loss_scale=1024.0)  # noqa: E731
    d1, d2 = mk(), mk()
    x, y = _data(torch.bfloat16)
    loss_fn = lambda d, xx, yy: d.scale_loss(_loss(d, xx, yy))  # noqa: E731
    g = GraphedStep(d1, loss_fn, x, y, warmup=2)
    for _ in range(2):
        loss_fn(d2, x, y).backward()
        d2.step()
    for i in range(3):
        g(x, y)
        loss_fn(d2, x, y).backward()
        d2.step()
        torch.cuda.synchronize()
        assert LS.same(LS.state(d1), LS.state(d2)) and LS.same(TE.ema_bits(d1), TE.ema_bits(d2)), i
    assert int(d1.ema_updates()) == 2 and int(d1._ema_block[3]) == 1


def test_ema_weights_on_the_gpu(gpu_ext):
    d, twin = _engine("adam", ema=0.9), _engine("adam", ema=0.9)
    for e in (d, twin):
        TE.train_step(e, 0)
    before, avg = LS.state(d), TE.ema_bits(d)
    with d.ema_weights():
        for n, p in d.module.named_parameters():
            assert torch.equal(p, d.ema_parameters()[n].to(torch.bfloat16))
        out = d(_data(torch.bfloat16)[0])  # evaluation with the averaged weights
        assert out.shape == (8, 10)
        with pytest.raises(RuntimeError):
            d.step()
    assert LS.same(before, LS.state(d)) and LS.same(avg, TE.ema_bits(d))
    for e in (d, twin):
        TE.train_step(e, 1)
    assert LS.same(LS.state(d), LS.state(twin)) and LS.same(TE.ema_bits(d), TE.ema_bits(twin))


def test_without_masters_the_source_is_the_parameter(gpu_ext):
    from fluxmpi_amd.ops import optim
    d = _engine("adam", dtype=torch.float32, master_weights=False, ema=0.5)
    assert all(b.master is None for b in d.buckets)
    mine = {n: p.detach().cpu().clone() for n, p in d.module.named_parameters()}
    for t in range(2):
        omd = float(d._ema_block.view(torch.float32)[optim.EMA_OMD])
        TE.train_step(d, t)
        for n, p in d.module.named_parameters():
            x = p.detach().cpu()
            TE.assert_within_bound(d.ema_parameters()[n].cpu(), mine[n], x, omd, (t, n))
            optim.ema_reference_([mine[n]], [x], decay=1.0 - omd)
            assert not torch.equal(mine[n], x)
