"""Fused softmax cross-entropy on the CPU: the reference against ``F.cross_entropy``, the rank rule, the
float32 emulation and the planted defects through the checker of ``xent_edges``, the argument errors,
``DeviceAugment(targets="labels")`` and the meter (``fluxmpi_amd/ops/xent.py``)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fluxmpi_amd as FluxMPI
from fluxmpi_amd.ops import augment as A
from fluxmpi_amd.ops import xent as X

from . import xent_edges as XE
from .conftest import run_spmd

REDS = ("mean", "sum", "none")


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _x64(B=6, C=10, seed=0):
    return XE.logits(B, C, torch.float64, seed)


@pytest.mark.parametrize("red", REDS)
@pytest.mark.parametrize("eps", (0.0, 0.1))
def test_reference_matches_torch_hard_and_dense(red, eps):
    """fp64 on both sides, sums of at most 1000 terms: 1e-12 relative."""
    for B, C in ((6, 10), (3, 1000)):
        x, y = _x64(B, C), XE.labels(B, C)
        for target in (y, XE.dense_target(B, C).double()):
            loss, loss_row, dx, _ = X.xent_reference(x, target, label_smoothing=eps, reduction=red)
            xr = x.clone().requires_grad_()
            want = F.cross_entropy(xr, target, label_smoothing=eps, reduction=red)
            want.sum().backward()
            assert _rel(loss, want.detach()) <= 1e-12
            assert _rel(dx, xr.grad) <= 1e-12
            assert _rel(loss_row, F.cross_entropy(x, target, label_smoothing=eps, reduction="none")) <= 1e-12


@pytest.mark.parametrize("lam", (0.0, 0.3, 1.0))
def test_reference_mixed_form(lam):
    B, C, eps = 6, 10, 0.1
    x, y = _x64(B, C), XE.labels(B, C)
    for lam_arg in (lam, torch.tensor(lam, dtype=torch.float32)):
        loss, loss_row, dx, rank = X.xent_reference(x, y, lam=lam_arg, label_smoothing=eps)
        # mix_targets rounds its entries to fp32: 1e-5
        soft = A.mix_targets(y, C, lam_arg, eps).double()
        assert _rel(loss, F.cross_entropy(x, soft)) <= 1e-5
        # its own closed form with lam32, rest32: 1e-12
        l32 = np.float32(lam)
        lam64, rest64 = float(l32), float(np.float32(1.0) - l32)
        lse = torch.logsumexp(x, 1)
        xy, xp = x[torch.arange(B), y], x[torch.arange(B), y.flip(0)]
        want = (lam64 + rest64) * lse - ((1 - eps) * (lam64 * xy + rest64 * xp) + (lam64 + rest64) * eps * x.mean(1))
        assert _rel(loss_row, want) <= 1e-12
        assert _rel(loss, want.mean()) <= 1e-12
        via_tuple = X.xent_reference(x, X.MixedLabels(y, lam_arg, eps))
        assert torch.equal(via_tuple[0], loss) and torch.equal(via_tuple[2], dx)
        assert torch.equal(rank, X.xent_reference(x, y)[3])  # the rank is the own label's


@pytest.mark.parametrize("red", REDS)
def test_cpu_path_gradient_matches_autograd_of_reference(red):
    B, C = 5, 12
    y, t = XE.labels(B, C), XE.dense_target(B, C)
    g = torch.rand(B) + 0.5 if red == "none" else torch.tensor(3.0)
    forms = [dict(target=y), dict(target=y, label_smoothing=0.1), dict(target=y, lam=0.3, label_smoothing=0.1),
             dict(target=t, label_smoothing=0.1)]
    for kw in forms:
        x = XE.logits(B, C, torch.float32).requires_grad_()
        loss = FluxMPI.softmax_cross_entropy(x, reduction=red, **kw)
        assert loss.dtype == torch.float32 and loss.shape == ((B,) if red == "none" else ())
        loss.backward(g)
        # autograd through the same formulas, in fp64
        x64 = x.detach().double().requires_grad_()
        spec = X._parse("t", x64, kw["target"], kw.get("label_smoothing", 0.0), kw.get("lam"), None, wide_ok=True)
        lse = torch.logsumexp(x64, 1)
        _, tt, W, _ = X._formulas(x64, spec, torch.float64)
        row = W.squeeze(1) * lse - (tt * x64).sum(1)
        ref = row if red == "none" else (row.mean() if red == "mean" else row.sum())
        ref.backward(g.double())
        assert _rel(loss.detach().double(), ref.detach()) <= 1e-6
        assert float((x.grad.double() - x64.grad).abs().max()) <= 1e-6 * float(g.abs().max())


def test_rank_rule():
    B, C = 64, 40
    x, y = XE.logits(B, C, torch.float32, seed=3), XE.labels(B, C, seed=3)
    rank = X.xent_reference(x, y)[3]
    assert rank.dtype == torch.int32
    for k in (1, 5):
        hit = (x.topk(k, dim=1).indices == y.unsqueeze(1)).any(1)  # no ties in random fp32 rows
        assert torch.equal(rank < k, hit)
    xt = XE.plant_ties(x, y)
    rank = X.xent_reference(xt, y)[3]
    for b in range(B):
        yb = int(y[b])
        want = int(yb > 0) + int(yb - 1 > 0)  # the tie at index 0 counts, those at the end do not; one larger value
        assert int(rank[b]) == want, (b, yb)
    cpu = FluxMPI.softmax_cross_entropy(xt, y, return_rank=True)[1]
    assert torch.equal(cpu, rank)


def _cases():
    B, C = 5, 24
    y = XE.labels(B, C)
    return {
        "hard": (XE.logits(B, C, torch.bfloat16), dict(target=y, label_smoothing=XE.EPS)),
        "hard-shifted": (XE.logits(B, C, torch.float32, shift=100.0), dict(target=y)),
        "mixed": (XE.logits(B, C, torch.float16), dict(target=y, lam=0.3, label_smoothing=XE.EPS)),
        "dense": (XE.logits(B, C, torch.bfloat16), dict(target=XE.dense_target(B, C), labels=y)),
        "ties": (XE.plant_ties(XE.logits(B, C, torch.float32), y), dict(target=y)),
    }


@pytest.mark.parametrize("red", REDS)
def test_emulation_fits_the_bounds(red):
    for name, (x, kw) in _cases().items():
        g = torch.rand(x.shape[0]) + 0.5 if red == "none" else 65536.0
        errs = []
        XE.check_all(name, XE.emulate(x, kw, red, g), XE.refs(x, kw, red, g), errs)
        XE.check_all(name + " general", XE.emulate(x, kw, red, g), XE.refs(x, kw, red, g, general=True), errs)
        assert not errs, errs


@pytest.mark.parametrize("defect,case", [("no_max", "hard-shifted"), ("inv_c", "hard"), ("partner_next", "mixed"),
                                         ("drop_w", "dense"), ("tie_wrong", "ties")])
def test_planted_defects_are_rejected(defect, case):
    x, kw = _cases()[case]
    errs = []
    XE.check_all(case, XE.emulate(x, kw, "mean", 1.0, defect=defect), XE.refs(x, kw, "mean", 1.0), errs)
    assert errs, f"{defect} passed the checker"
    errs = []
    XE.check_all(case, XE.emulate(x, kw, "mean", 1.0), XE.refs(x, kw, "mean", 1.0), errs)
    assert not errs, errs


def test_argument_errors():
    x = torch.zeros(4, 10)
    y = torch.zeros(4, dtype=torch.int64)
    f = FluxMPI.softmax_cross_entropy
    bad = [
        (ValueError, lambda: f(torch.zeros(4, 10, 2), y)),
        (ValueError, lambda: f(torch.zeros(10), y[:1])),
        (TypeError, lambda: f(x.double(), y)),
        (TypeError, lambda: f(x.to(torch.int32), y)),
        (ValueError, lambda: f(x, y[:3])),
        (ValueError, lambda: f(x, torch.zeros(4, 9))),
        (TypeError, lambda: f(x, torch.zeros(4, dtype=torch.int16))),
        (TypeError, lambda: f(x, [0, 1, 2, 3])),
        (ValueError, lambda: f(x, y.to("meta"))),
        (ValueError, lambda: f(x, y, label_smoothing=1.0)),
        (ValueError, lambda: f(x, y, label_smoothing=-0.1)),
        (ValueError, lambda: f(x, torch.zeros(4, 10), lam=0.5)),
        (ValueError, lambda: f(x, torch.zeros(4, 10), return_rank=True)),
        (ValueError, lambda: f(x, torch.zeros(4, 10), meter=FluxMPI.ClassificationMeter())),
        (ValueError, lambda: f(x, y, reduction="avg")),
        (ValueError, lambda: f(x, y + 10)),  # the CPU path checks the range
        (ValueError, lambda: FluxMPI.ClassificationMeter(topk=(1,))),
        (ValueError, lambda: FluxMPI.SoftmaxCrossEntropy(label_smoothing=1.5)),
    ]
    for exc, call in bad:
        with pytest.raises(exc) as ei:
            call()
        assert any(w in str(ei.value) for w in ("softmax_cross_entropy", "ClassificationMeter", "SoftmaxCrossEntropy"))
    loss, rank = f(x, torch.zeros(4, 10), labels=y, return_rank=True)  # labels= makes the dense form rankable
    assert rank.shape == (4,)


def test_empty_batch():
    x = torch.zeros(0, 7, requires_grad=True)
    y = torch.zeros(0, dtype=torch.int64)
    mean = FluxMPI.softmax_cross_entropy(x, y)
    assert mean.shape == () and torch.isnan(mean)
    total = FluxMPI.softmax_cross_entropy(x, y, reduction="sum")
    assert float(total) == 0.0
    rows, rank = FluxMPI.softmax_cross_entropy(x, y, reduction="none", return_rank=True)
    assert rows.shape == (0,) and rank.shape == (0,)
    total.backward()
    assert x.grad.shape == (0, 7)
    assert torch.isnan(F.cross_entropy(x, y)) and float(F.cross_entropy(x, y, reduction="sum")) == 0.0  # as torch


def test_module_and_nonfinite_free_defaults():
    x, y = XE.logits(4, 10, torch.float32), XE.labels(4, 10)
    crit = FluxMPI.SoftmaxCrossEntropy(label_smoothing=0.1, reduction="sum")
    assert torch.equal(crit(x, y), FluxMPI.softmax_cross_entropy(x, y, label_smoothing=0.1, reduction="sum"))
    nc = x.t().contiguous().t()  # non-contiguous logits
    assert torch.equal(FluxMPI.softmax_cross_entropy(nc, y), FluxMPI.softmax_cross_entropy(x, y))


def test_device_augment_labels_route():
    B, K = 6, 10
    img = torch.randint(0, 256, (B, 12, 12, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    y = XE.labels(B, K)
    common = dict(pad=2, seed=5, mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=K)
    dense, lab = FluxMPI.DeviceAugment(8, **common), FluxMPI.DeviceAugment(8, targets="labels", **common)
    for step in range(4):
        xd, yd = dense(img, y)
        xl, yl = lab(img, y)
        assert torch.equal(xd, xl)
        assert isinstance(yl, X.MixedLabels) and yl.labels is y and yl.label_smoothing == 0.1
        assert yl.lam == dense.draw(step).lam
        # the dense route is today's: bit for bit the existing functions
        mix = A.draw_mix(5, 0, step, (8, 8), 0.8, 1.0)
        assert torch.equal(yd, A.mix_targets(y, K, mix.lam, 0.1))
        assert torch.equal(xd, A.augment_batch(img, size=(8, 8), pad=2, seed=5, step=step, mix=mix))
        # and both routes give one loss
        z = XE.logits(B, K, torch.float32, seed=step)
        a, b = FluxMPI.softmax_cross_entropy(z, yl), F.cross_entropy(z, yd)
        assert abs(float(a) - float(b)) <= 1e-5 * abs(float(b))
    plain = FluxMPI.DeviceAugment(8, targets="labels")
    assert plain(img, y)[1] is y  # nothing mixes, no smoothing: the plain labels
    with pytest.raises(ValueError):
        FluxMPI.DeviceAugment(8, targets="soft")


def test_meter_cpu():
    meter = FluxMPI.ClassificationMeter(topk=(1, 5))
    C = 10
    tot, rows, c1, c5 = 0.0, 0, 0, 0
    for i, B in enumerate((4, 7, 3)):
        x, y = XE.logits(B, C, torch.float32, seed=i), XE.labels(B, C, seed=i)
        with torch.no_grad():
            FluxMPI.softmax_cross_entropy(x, y, meter=meter)
        _, row, _, rank = X.xent_reference(x, y)
        tot, rows, c1, c5 = tot + float(row.sum()), rows + B, c1 + int((rank < 1).sum()), c5 + int((rank < 5).sum())
    got = meter.read()
    assert got["rows"] == rows and got["top1"] == c1 / rows and got["top5"] == c5 / rows
    assert abs(got["loss"] - tot / rows) <= 1e-6 * abs(tot / rows)
    assert meter.block.dtype == torch.int64 and meter.block.numel() * 2 == X.METER_WORDS
    meter.reset()
    assert meter.read()["rows"] == 0 and np.isnan(meter.read()["loss"])


def _spmd_meter_reduce():
    FluxMPI.Init()
    rank, n = FluxMPI.local_rank(), FluxMPI.total_workers()
    C = 10
    meter = FluxMPI.ClassificationMeter()
    B = 3 + 2 * rank  # different batch sizes per rank
    x, y = XE.logits(B, C, torch.float32, seed=rank), XE.labels(B, C, seed=rank)
    FluxMPI.softmax_cross_entropy(x, y, meter=meter)
    tot, rows, c1, c5 = 0.0, 0, 0, 0
    for r in range(n):
        b = 3 + 2 * r
        _, row, _, rk = X.xent_reference(XE.logits(b, C, torch.float32, seed=r), XE.labels(b, C, seed=r))
        tot, rows, c1, c5 = tot + float(row.sum()), rows + b, c1 + int((rk < 1).sum()), c5 + int((rk < 5).sum())
    got = meter.read(reduce=True)
    assert got["rows"] == rows and got["top1"] == c1 / rows and got["top5"] == c5 / rows, (got, rows, c1, c5)
    assert abs(got["loss"] - tot / rows) <= 1e-6 * abs(tot / rows)
    assert meter.read()["rows"] == B  # the block itself stays local


def test_meter_reduce_two_ranks():
    run_spmd("tests.test_xent:_spmd_meter_reduce", nprocs=2)
