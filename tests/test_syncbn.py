"""Synchronised BatchNorm on CPU: the count encoding, the PyTorch fallback of the message protocol with one
process playing W ranks, SPMD runs over gloo (module, DDP, no_sync, eval), ``convert_sync_batchnorm``, the float32
emulation of the deterministic scheme against the derived bounds, and the undecided-ReLU cap of every GPU case's
reference (``syncbn_edges``: bounds derived, nothing fitted)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import norm_edges as N
from . import syncbn_edges as SE

DT = [torch.bfloat16, torch.float16, torch.float32]
DT_IDS = ["bf16", "fp16", "fp32"]


# ------------------------------------------------------------------------------- count encoding

@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 25_690_112, 2 ** 31 - 1,
                               2 ** 31, 2 ** 31 + 1, 2 ** 36 - 1])
def test_count_roundtrip_cpu(n):
    """n = 4096 n_hi + n_lo survives two fp32 slots, and a SUM of 8 ranks' slots, on both sides of 2^24 and 2^31
    (one fp32 slot loses 2^24 + 1)."""
    from fluxmpi_amd.ops.syncbn import COUNT_RADIX, join_count, split_count

    hi, lo = split_count(n)
    assert 0 <= lo < COUNT_RADIX and hi * COUNT_RADIX + lo == n
    slots = torch.tensor([hi, lo], dtype=torch.float32)
    assert join_count(slots[0], slots[1]) == n
    msg = torch.cat([torch.zeros(16), slots])
    assert SE.count_of(msg) == n
    if n < 2 ** 33:  # 8 ranks of this size
        tot = torch.zeros(2)
        for _ in range(8):
            tot = tot + slots
        assert join_count(tot[0], tot[1]) == 8 * n
    if n == 2 ** 24 + 1:
        assert int(torch.tensor(float(n), dtype=torch.float32)) != n


# ------------------------------------------------------------------------------- fallback, one process

FALLBACK = [([37], 8), ([36, 1], 8), ([20, 0, 17], 24), ([1, 300, 0], 8)]


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("mode", list(SE.MODES))
@pytest.mark.parametrize("shard_rows,C", FALLBACK, ids=[f"{'+'.join(map(str, r))}x{c}" for r, c in FALLBACK])
def test_fallback_shards_cpu(shard_rows, C, mode, dtype):
    """W in {1, 2, 3} shards (an empty one, a 1-row one) through the PyTorch path of the op-level functions with the
    messages summed by hand: y, dx, sum_r dw, sum_r db and the running statistics against the float64 reference of
    the concatenated batch, within the bound of L_torch."""
    inp = N.rows_inputs("uniform", sum(shard_rows), C, dtype)
    shards = SE.split(inp, shard_rows)
    errs = []
    running = (torch.linspace(-1, 1, C), torch.linspace(0.5, 2, C))
    tag = f"fallback {shard_rows} C {C} {mode}"
    fwd, bwd = SE.play(SE.OpPlayer(), shards, mode, True, running, errs, tag)
    for sh, m in zip(shards, fwd["msgs"]):
        assert SE.count_of(m) == sh["x"].shape[0]
    assert SE.count_of(fwd["msg"]) == sum(shard_rows)
    SE.check_play(tag, inp, fwd, bwd, SE.L_torch(shard_rows), mode, True, dtype, errs, running)
    assert not errs, "\n".join(errs)


def module_case(cls, inp, dims, L, dtype, errs, tag):
    """One training forward + backward of ``cls(C)`` (ReLU after a residual) on the [n, C, h, w] view of ``inp``
    without a process group, every output against the float64 reference within the bound of ``L``. Also run on
    the GPU by ``test_syncbn_gpu.py`` (the saved statistics and mask are read from the autograd node)."""
    n, C, h, w = dims
    rows, dev = n * h * w, inp["x"].device
    nchw = lambda t: t.reshape(n, h, w, C).permute(0, 3, 1, 2)  # channels_last memory
    rows2 = lambda t: t.permute(0, 2, 3, 1).reshape(rows, C)
    bn = cls(C).to(dev)
    running = (torch.linspace(-1, 1, C, device=dev), torch.linspace(0.5, 2, C, device=dev))
    with torch.no_grad():
        bn.weight.copy_(inp["w"]), bn.bias.copy_(inp["b"])
        bn.running_mean.copy_(running[0]), bn.running_var.copy_(running[1])
    x = nchw(inp["x"]).detach().requires_grad_()
    res = nchw(inp["res"]).detach().requires_grad_()
    y = bn(x, relu=True, residual=res)
    saved = y.grad_fn.saved_tensors
    mask, mean32, inv32 = saved[1], saved[4].clone(), saved[5].clone()
    y.backward(nchw(inp["dy"]))
    assert int(bn.num_batches_tracked) == 1
    fwd = dict(mean=mean32, inv=inv32, y=rows2(y.detach()), mask=mask, rm=bn.running_mean, rv=bn.running_var)
    bwd = dict(dx=rows2(x.grad), dres=rows2(res.grad), dw=bn.weight.grad, db=bn.bias.grad)
    SE.check_play(tag, inp, fwd, bwd, L, "relu_res", True, dtype, errs, running)
    return bn


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_module_world1_cpu(dtype):
    """The autograd function without ``Init`` (world size 1, the PyTorch path): forward, backward, running statistics
    and num_batches_tracked; eval mode is torch's inference BatchNorm; ``bnlink`` is refused."""
    from fluxmpi_amd.ops.syncbn import SyncBatchNorm2d, sync_batch_norm

    n, C, h, w = 5, 6, 3, 4
    inp = N.rows_inputs("uniform", n * h * w, C, dtype)
    errs = []
    bn = module_case(SyncBatchNorm2d, inp, (n, C, h, w), SE.L_torch([n * h * w]), dtype, errs, "world 1")
    assert not errs, "\n".join(errs)
    x = inp["x"].reshape(n, h, w, C).permute(0, 3, 1, 2)
    ref = nn.BatchNorm2d(C)
    ref.load_state_dict(bn.state_dict())
    bn.eval(), ref.eval()
    assert torch.equal(bn(x), ref(x.float()).to(dtype))
    with pytest.raises(ValueError):
        sync_batch_norm(x, None, None, None, None, True, 0.1, 1e-5, bnlink=object())


# ------------------------------------------------------------------------------- SPMD over gloo

SPMD_C, SPMD_HW = 8, (3, 2)


def _shard_rows(W, uneven):
    """Samples per rank: 3, 5, 2, 4 ...; ``uneven``: the second rank's shard is empty."""
    n = [(3, 5, 2, 4)[k % 4] for k in range(W)]
    if uneven:
        n[1] = 0
    return n


def _global(W, uneven, seed=0):
    """Every rank rebuilds all shards from seeds: (global inputs [rows, C], samples per rank)."""
    ns = _shard_rows(W, uneven)
    rows = sum(ns) * SPMD_HW[0] * SPMD_HW[1]
    return N.rows_inputs("uniform", rows, SPMD_C, torch.float32, seed=seed), ns


def _nchw(t2, n):
    """[n h w, C] rows -> an [n, C, h, w] tensor (rows are NHWC pixels)."""
    return t2.reshape(n, SPMD_HW[0], SPMD_HW[1], SPMD_C).permute(0, 3, 1, 2).contiguous()


def _module_checks(uneven, dev="cpu"):
    """Also run by the two-ranks-on-one-GPU test (``dev`` = "cuda": the HIP path, bound of L_sync)."""
    import fluxmpi_amd as FluxMPI
    from fluxmpi_amd.ops.syncbn import SyncBatchNorm2d
    from fluxmpi_amd.parallel import runtime

    r, W = FluxMPI.local_rank(), FluxMPI.total_workers()
    inp, ns = _global(W, uneven)
    px = SPMD_HW[0] * SPMD_HW[1]
    shard_rows = [n * px for n in ns]
    mine = SE.split(inp, shard_rows)[r]
    for mode in SE.MODES:
        relu, use_res = SE.MODES[mode]
        bn = SyncBatchNorm2d(SPMD_C).to(dev)
        running = (torch.linspace(-1, 1, SPMD_C), torch.linspace(0.5, 2, SPMD_C))
        with torch.no_grad():
            bn.weight.copy_(inp["w"]), bn.bias.copy_(inp["b"])
            bn.running_mean.copy_(running[0]), bn.running_var.copy_(running[1])
        x = _nchw(mine["x"], ns[r]).to(dev).requires_grad_()
        res = _nchw(mine["res"], ns[r]).to(dev).requires_grad_() if use_res else None
        y = bn(x, relu=relu, residual=res)
        assert y.shape == x.shape
        mean32, inv32 = (t.cpu() for t in y.grad_fn.saved_tensors[4:6])  # the statistics the backward reads
        y.backward(_nchw(mine["dy"], ns[r]).to(dev))
        rows2 = lambda t: t.permute(0, 2, 3, 1).reshape(-1, SPMD_C)
        # gather every rank's outputs (padded to the largest shard) to check the whole batch on every rank
        cap = max(shard_rows)

        def gather(t2):
            pad = torch.zeros(cap, SPMD_C)
            pad[:t2.shape[0]] = t2.cpu()
            g = FluxMPI.allgather(pad.reshape(-1))
            return torch.cat([g[k].reshape(cap, SPMD_C)[:shard_rows[k]] for k in range(W)])

        ya, dxa = gather(rows2(y.detach())), gather(rows2(x.grad))
        dw, db = bn.weight.grad.cpu(), bn.bias.grad.cpu()
        FluxMPI.allreduce(dw), FluxMPI.allreduce(db)
        errs, tag = [], f"rank {r} of {W} {mode}"
        L = SE.L_torch(shard_rows) if dev == "cpu" else SE.L_sync(shard_rows, SPMD_C)
        fwd = dict(mean=mean32, inv=inv32, y=ya, rm=bn.running_mean.cpu(), rv=bn.running_var.cpu())
        z, _, und = SE.check_fwd(tag, inp, fwd, L, relu, use_res, True, torch.float32, errs, running=running)
        assert not bool(und.any())  # the seeds leave no undecided element: the module's decisions are z > 0
        assert int(bn.num_batches_tracked) == 1
        g = inp["dy"].double() * ((z > 0) if relu else 1)
        SE.check_bwd(tag, inp, dict(dx=dxa, dw=dw, db=db, dres=gather(rows2(res.grad)) if use_res else None),
                     mean32, inv32, g, L, True, torch.float32, errs)
        assert not errs, "\n".join(errs)
    # eval mode: no collective
    comm = runtime.comm_for(torch.zeros(1, device=dev))
    calls, orig = [0], comm.allreduce

    def counted(*a, **k):
        calls[0] += 1
        return orig(*a, **k)

    comm.allreduce = counted
    try:
        bn.eval()
        with torch.no_grad():
            bn(_nchw(mine["x"], ns[r]).to(dev), relu=True)
        assert calls[0] == 0
        bn.train()
        bn(_nchw(mine["x"], ns[r]).to(dev))
        assert calls[0] == 1
    finally:
        comm.allreduce = orig


def worker_module():
    import fluxmpi_amd as FluxMPI

    FluxMPI.Init()
    _module_checks(uneven=False)
    FluxMPI.Finalize()


def worker_module_uneven():
    import fluxmpi_amd as FluxMPI

    FluxMPI.Init()
    assert FluxMPI.total_workers() == 3
    _module_checks(uneven=True)
    FluxMPI.Finalize()


def test_module_gloo(spmd):
    """SyncBatchNorm2d forward / backward / running statistics on every rank against the full-batch reference,
    and eval mode issuing no collective, at the default world size."""
    spmd("tests.test_syncbn:worker_module", timeout=240)


def test_module_gloo_uneven3(spmd):
    """The same at 3 ranks with uneven shards, one of them empty."""
    spmd("tests.test_syncbn:worker_module_uneven", nprocs=3, timeout=240)


class _Net(nn.Module):
    """conv + SyncBN(+ReLU) + linear, loss summed over the samples."""

    def __init__(self, sync):
        super().__init__()
        from fluxmpi_amd.ops.syncbn import SyncBatchNorm2d
        torch.manual_seed(3)
        self.conv = nn.Conv2d(3, 8, 3, padding=1, bias=False)
        self.bn = SyncBatchNorm2d(8) if sync else nn.BatchNorm2d(8)
        self.fc = nn.Linear(8, 4)
        self.sync = sync

    def forward(self, x):
        h = self.conv(x)
        h = self.bn(h, relu=True) if self.sync else F.relu(self.bn(h))
        return self.fc(h.mean((2, 3)))


def _net_data(k, n):
    g = torch.Generator().manual_seed(50 + k)
    return torch.randn(n, 3, 4, 4, generator=g), torch.randn(n, 4, generator=g)


def _ddp_checks(uneven):
    import fluxmpi_amd as FluxMPI
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP

    r, W = FluxMPI.local_rank(), FluxMPI.total_workers()
    ns = _shard_rows(W, uneven)
    data = [_net_data(k, ns[k]) for k in range(W)]
    xa, ya = torch.cat([d[0] for d in data]), torch.cat([d[1] for d in data])
    for accumulate in (False, True):
        model, ref = _Net(True), _Net(False)
        ddp = DDP(model, O.Descent(0.01), bucket_mb=0.001, first_bucket_mb=0.0005)
        x, y = data[r]
        for _ in range(2):
            if accumulate:  # two micro-batches per rank under no_sync: the statistics are still synchronised
                h = ns[r] // 2
                with ddp.no_sync():
                    ((ddp(x[:h]) - y[:h]) ** 2).sum().backward()
                ((ddp(x[h:]) - y[h:]) ** 2).sum().backward()
                ddp.step()
                halves = [(torch.cat([d[0][:n // 2] for d, n in zip(data, ns)]),
                           torch.cat([d[1][:n // 2] for d, n in zip(data, ns)])),
                          (torch.cat([d[0][n // 2:] for d, n in zip(data, ns)]),
                           torch.cat([d[1][n // 2:] for d, n in zip(data, ns)]))]
            else:
                ((ddp(x) - y) ** 2).sum().backward()
                ddp.step()
                halves = [(xa, ya)]
            ref.zero_grad()
            for xh, yh in halves:  # the single-process full-batch reference with loss sum_r L_r
                ((ref(xh) - yh) ** 2).sum().backward()
            with torch.no_grad():
                for p in ref.parameters():
                    p -= 0.01 * p.grad
        for (n, p), q in zip(model.named_parameters(), ref.parameters()):
            # Not a derived bound: two optimiser steps through torch's convolution and linear layers (whose
            # summation orders are not ours to write down) have no closed-form error, so this check takes the
            # tolerance tests/test_ddp.py uses for W-rank fp32 sums in another order. It is about the protocol
            # (local statistics, a missed collective or a wrong dw / db scale are wrong by orders of magnitude
            # more); the per-element bounds of the SyncBN outputs and gradients are in _module_checks.
            torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-5, atol=1e-5,
                                       msg=lambda m: f"accumulate {accumulate} {n}: {m}")
        for p, q in zip(model.buffers(), ref.buffers()):
            torch.testing.assert_close(p, q, rtol=1e-5, atol=1e-5)  # as above


def worker_ddp():
    import fluxmpi_amd as FluxMPI

    FluxMPI.Init()
    _ddp_checks(uneven=False)
    FluxMPI.Finalize()


def worker_ddp_uneven():
    import fluxmpi_amd as FluxMPI

    FluxMPI.Init()
    _ddp_checks(uneven=True)
    FluxMPI.Finalize()


def test_ddp_gloo(spmd):
    """conv + SyncBN + linear under DDP with Descent, two steps, and the same under no_sync() accumulation, against
    the single-process full-batch model with loss sum_r L_r."""
    spmd("tests.test_syncbn:worker_ddp", timeout=240)


def test_ddp_gloo_uneven3(spmd):
    spmd("tests.test_syncbn:worker_ddp_uneven", nprocs=3, timeout=240)


# ------------------------------------------------------------------------------- convert_sync_batchnorm

def test_convert_shares_parameters_cpu():
    from fluxmpi_amd import SyncBatchNorm2d, convert_sync_batchnorm
    from fluxmpi_amd.ops.batchnorm import FusedBatchNorm2d

    net = nn.Sequential(nn.Conv2d(3, 8, 1), nn.BatchNorm2d(8), nn.Sequential(FusedBatchNorm2d(8, momentum=None),
                                                                             nn.BatchNorm2d(8, affine=False)))
    net[1].weight.requires_grad_(False)
    net[2].eval()
    before = {k: v for k, v in net.state_dict(keep_vars=True).items()}
    keys = list(net.state_dict().keys())
    out = convert_sync_batchnorm(net)
    assert out is net
    bns = [m for m in net.modules() if isinstance(m, nn.BatchNorm2d)]
    assert len(bns) == 3 and all(type(m) is SyncBatchNorm2d for m in bns)
    after = net.state_dict(keep_vars=True)
    assert list(after.keys()) == keys
    assert all(after[k] is before[k] for k in keys)  # shared, not copied
    assert not net[1].weight.requires_grad and net[1].bias.requires_grad
    assert net[1].training and not net[2][0].training
    assert net[2][0].momentum is None and not net[2][1].affine
    plain = nn.Sequential(nn.Conv2d(3, 8, 1), nn.BatchNorm2d(8), nn.Sequential(nn.BatchNorm2d(8, momentum=None),
                                                                               nn.BatchNorm2d(8, affine=False)))
    plain.load_state_dict(net.state_dict())  # loads into nn.BatchNorm2d
    net.load_state_dict(plain.state_dict())  # and back
    solo = convert_sync_batchnorm(nn.BatchNorm2d(4))
    assert type(solo) is SyncBatchNorm2d
    net.train()
    assert bool(torch.isfinite(net(torch.randn(4, 3, 5, 5))).all())


def test_convert_refuses_fused_resnet_cpu():
    from fluxmpi_amd import convert_sync_batchnorm
    from fluxmpi_amd.models.resnet import ResNet, resnet18ish

    for impl in ("fused", "hybrid"):
        with pytest.raises(ValueError):
            convert_sync_batchnorm(resnet18ish(conv_impl=impl))
        with pytest.raises(ValueError):
            convert_sync_batchnorm(nn.Sequential(resnet18ish(conv_impl=impl)))
        with pytest.raises(ValueError):
            ResNet((1, 1, 1, 1), 10, conv_impl=impl, norm="sync")
    assert resnet18ish(conv_impl="hybrid", norm="torch").norm_kind == "fused"  # every other combination as before
    m = convert_sync_batchnorm(resnet18ish(conv_impl="miopen", norm="fused"))
    assert all(type(b).__name__ == "SyncBatchNorm2d" for b in m.modules() if isinstance(b, nn.BatchNorm2d))


def _bn_calls(model):
    """Counts of calls that went through each SyncBatchNorm2d's own forward (forward hooks)."""
    from fluxmpi_amd.ops.syncbn import SyncBatchNorm2d

    calls = {}
    for name, m in model.named_modules():
        if isinstance(m, nn.BatchNorm2d):
            assert type(m) is SyncBatchNorm2d, name
            calls[name] = 0
            m.register_forward_hook(lambda mod, a, o, name=name: calls.__setitem__(name, calls[name] + 1))
    return calls


def test_resnet_sync_cpu():
    """ResNet(norm="sync") builds SyncBatchNorm2d everywhere and every one of them, the stem's included, runs through
    its own forward; a converted norm="fused" ResNet does the same (its stem leaves the fused BN + pool path)."""
    from fluxmpi_amd import convert_sync_batchnorm
    from fluxmpi_amd.models.resnet import resnet18ish

    torch.manual_seed(1)
    for m in (resnet18ish(norm="sync", conv_impl="miopen"),
              convert_sync_batchnorm(resnet18ish(norm="fused", conv_impl="miopen")),
              convert_sync_batchnorm(resnet18ish(norm="fused", conv_impl="gemm")),
              convert_sync_batchnorm(resnet18ish(norm="torch", conv_impl="gemm"))):
        assert m.norm_kind in ("sync", "torch")
        calls = _bn_calls(m)
        y = m(torch.randn(3, 3, 32, 32))
        y.sum().backward()
        assert bool(torch.isfinite(y).all()) and calls["bn1"] == 1 and all(v == 1 for v in calls.values()), calls


def test_deq_models_convert_cpu():
    """Both DEQ models take the conversion as they are (their BatchNorms are plain modules) and still run."""
    from fluxmpi_amd import SyncBatchNorm2d, convert_sync_batchnorm
    from fluxmpi_amd.models.deq import deq_cifar, deq_mnist

    torch.manual_seed(0)
    for build, x, names in [(lambda: deq_mnist(), torch.randn(2, 1, 8, 8), ("inj_norm", "out_norm")),
                            (lambda: deq_cifar(ch=32, groups=4), torch.randn(2, 3, 8, 8),
                             ("stem1_norm", "inj_norm", "out_norm"))]:
        m = build()
        keys = list(m.state_dict().keys())
        convert_sync_batchnorm(m)
        assert all(type(getattr(m, n)) is SyncBatchNorm2d for n in names)
        assert list(m.state_dict().keys()) == keys
        y = m(x)
        y.sum().backward()
        assert bool(torch.isfinite(y).all()) and getattr(m, names[0]).weight.grad is not None


# ------------------------------------------------------------------------------- emulation

EMU = [("uniform", 0, [301], 24), ("uniform", 0, [37, 0, 1100], 64), ("uniform", 0, [5, 50, 100], 2048),
       ("offset", 4, [683, 17], 96), ("offset", 32, [683, 17], 96), ("integer", 0, [20, 0, 108], 24),
       ("integer", 0, [100, 412], 2048), ("uniform", 0, [4100, 1], 8)]


def _emu_modes(family, ratio, shard_rows, C):
    eps_inv = (1 + ratio * ratio) * (SE.L_sync(shard_rows, C) + 3) * N.E23 / 2
    return ("none",) if eps_inv >= 5e-3 else tuple(SE.MODES)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("family,ratio,shard_rows,C", EMU,
                         ids=[f"{f}{r}-{'+'.join(map(str, s))}x{c}" for f, r, s, c in EMU])
def test_emulation_meets_bounds_cpu(family, ratio, shard_rows, C, dtype):
    """The deterministic scheme in float32 (lanes, workgroup partials, the fixed-order fold, the rank sum, the
    finalize: one addition at a time, no fma) stays inside the derived bounds; the exact family is exact."""
    inp = N.rows_inputs(family, sum(shard_rows), C, dtype, ratio)
    shards = SE.split(inp, shard_rows)
    running = (torch.full((C,), 0.25), torch.full((C,), 0.75))
    L = SE.L_sync(shard_rows, C)
    for mode in _emu_modes(family, ratio, shard_rows, C):
        relu, use_res = SE.MODES[mode]
        errs, tag = [], f"emulated {family}{ratio} {shard_rows} C {C} {mode}"
        fwd, bwd, g32 = SE.emulate(shards, relu, use_res, True, dtype, running)
        SE.check_fwd(tag, inp, fwd, L, relu, use_res, True, dtype, errs, running=running)
        SE.check_bwd(tag + " bwd", inp, bwd, fwd["mean"], fwd["inv"], g32.double(), L, True, dtype, errs,
                     exact=family == "integer")
        if family == "integer":
            s, q, n = SE.emulate_messages(shards)
            sd, qd, _, _ = SE.message_ref(inp["x"])
            assert torch.equal(s.double(), sd) and torch.equal(q.double(), qd) and n == sum(shard_rows)
            one = SE.emulate([inp], relu, use_res, True, dtype, running)
            for k in ("mean", "inv", "y"):
                assert torch.equal(fwd[k], one[0][k]), f"{tag}: {k} differs between W shards and one"
        assert not errs, "\n".join(errs)


def test_geometry_reaches_paths_cpu():
    """The GPU shapes reach what they are chosen for: one workgroup, a ragged tail, 3-4 workgroups; more partials
    than fold groups; and the documented geometry keeps every partial inside the buffer the op layer sizes."""
    assert SE.det_geometry(1, 64)[3] == 1 and SE.det_geometry(37, 64)[3] == 1
    assert 37 % SE.det_geometry(37, 64)[1] != 0  # ragged: rows not a multiple of rpi
    assert SE.det_geometry(1100, 64)[3] == 3 and SE.det_geometry(100, 2048)[3] == 4
    assert SE.det_geometry(50, 2048)[3] == 2 and SE.det_geometry(5, 2048)[3] == 1
    assert SE.det_geometry(10000, 64)[3] > SE.FOLD_GROUPS
    for rows, C in [(1, 8), (4100, 8), (301, 24), (10 ** 7, 64), (12544, 2048), (3 * 10 ** 6, 2048)]:
        _, rpi, rpb, blocks = SE.det_geometry(rows, C)
        assert blocks <= SE.MAX_BLOCKS and rpb % rpi == 0 and (blocks - 1) * rpb < rows <= blocks * rpb
