"""The fused softmax cross-entropy kernels (``csrc/kernels/xent.hip``) on the GPU: every element of the row
losses, the reduced loss and the gradient against the float64 reference within the bounds derived in
``xent_edges`` (nothing excluded: there is no undecided branch), exact cases that must EQUAL the
reference, the rank, determinism, the meter, HIP-graph capture and one DDP step.

Shapes are the smallest at which each path can go wrong: (1, 1); (3, 10) the general path; (5, 1000) the
register path with the last lanes masked (125 vectors); (4, 8); (2, 8192) the widest register row;
(2, 8200) and (1, 40000) the loop; (257, 16) rows not a multiple of 4 and more than one finish stride; a
slice one element off 16-byte alignment; a strided view.
"""
import pytest
import torch
import torch.nn.functional as F

import fluxmpi_amd as FluxMPI
from fluxmpi_amd.ops import _ext
from fluxmpi_amd.ops import xent as X
from fluxmpi_amd.ops.multi_tensor import DTYPE_CODE

from . import mfma_edges as E
from . import xent_edges as XE

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 1), (3, 10), (5, 1000), (4, 8), (2, 8192), (2, 8200), (1, 40000), (257, 16)]
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
BIG = 65536.0  # the loss scale


def _dev(kw):
    out = {}
    for k, v in kw.items():
        if isinstance(v, X.MixedLabels):
            v = X.MixedLabels(v.labels.to(DEV), v.lam.to(DEV) if isinstance(v.lam, torch.Tensor) else v.lam,
                              v.label_smoothing)
        out[k] = v.to(DEV) if isinstance(v, torch.Tensor) else v
    return out


def _run(x, kw, red, g):
    """Forward and backward on the GPU: ``{loss_row, loss, dx, rank}``. ``g``: a number (the loss is multiplied
    by a device scalar, as ``ddp.scale_loss`` does) or a ``[B]`` tensor (``"none"``)."""
    xg = x.to(DEV).requires_grad_()
    kwg = _dev(kw)
    has_labels = isinstance(kw["target"], X.MixedLabels) or not kw["target"].is_floating_point() or "labels" in kw
    out = FluxMPI.softmax_cross_entropy(xg, reduction=red, return_rank=has_labels, **kwg)
    loss, rank = out if has_labels else (out, None)
    assert loss.dtype == torch.float32 and loss.shape == ((x.shape[0],) if red == "none" else ())
    if isinstance(g, torch.Tensor):
        loss.backward(g.to(DEV))
    elif g == 1.0:
        loss.backward()
    else:
        (loss * torch.tensor(g, device=DEV)).backward()
    assert xg.grad.dtype == x.dtype
    with torch.no_grad():
        rows = loss if red == "none" else FluxMPI.softmax_cross_entropy(xg, reduction="none", **kwg)
    return {"loss_row": rows, "loss": loss.detach(), "dx": xg.grad, "rank": rank}


def _forms(B, C, dtype, ldt):
    """Every target form of a shape: hard and dense with eps in {0, 0.1}; mixed with lam in {0, 0.3, 1}
    as a float and as a device word. Rows 0 and B - 1 share a label (both weights on one class) and an
    odd B has a middle row that is its own partner; the dense rows do not sum to 1."""
    y = XE.labels(B, C, dtype=ldt)
    t32, t16 = XE.dense_target(B, C), XE.dense_target(B, C, dtype, seed=1)
    word = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    return {
        "hard": dict(target=y),
        "hard-eps": dict(target=y, label_smoothing=XE.EPS),
        "mixed-0.3": dict(target=y, lam=0.3, label_smoothing=XE.EPS),
        "mixed-0-word": dict(target=X.MixedLabels(y, word(0.0), 0.0)),
        "mixed-1": dict(target=y, lam=1.0),
        "mixed-0.3-word": dict(target=y, lam=word(0.3), label_smoothing=XE.EPS),
        "dense": dict(target=t32, labels=y),
        "dense-eps": dict(target=t16, label_smoothing=XE.EPS),
    }


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_element_within_the_bounds(gpu_ext, shape, dtype):
    B, C = shape
    x = XE.logits(B, C, dtype, seed=B + C)
    ldt = torch.int32 if (B + C) % 2 else torch.int64
    gvec = torch.rand(B, generator=E._gen("xent-g", B, C)) + 0.5
    # 65536 / B * |p - t| must stay inside fp16: B >= 2
    combos = [("mean", 1.0), ("sum", 1.0), ("none", gvec)] + ([("mean", BIG)] if B >= 2 else [])
    errs = []
    for name, kw in _forms(B, C, dtype, ldt).items():
        for red, g in combos:
            XE.check_all(f"{name} {red}", _run(x, kw, red, g), XE.refs(x, kw, red, g), errs)
    assert not errs, "\n".join(errs)


def test_unaligned_slice_takes_the_general_path_inside_its_buffer(gpu_ext):
    """[6, 1000] one element off 16-byte alignment, logits and every output inside sentinel buffers."""
    B, C = 6, 1000
    Xm = _ext.xent()
    stream = torch.cuda.current_stream().cuda_stream
    for dtype in (torch.bfloat16, torch.float32):
        x = XE.logits(B, C, dtype, seed=7)
        y = XE.labels(B, C)
        kw = dict(target=y, lam=0.3, label_smoothing=XE.EPS)
        errs = []

        def off_by_one(dt, n):
            buf, view = E.guarded(1, n + 1, n + 8, dt, DEV, fill=0)  # n + 8: the view itself starts aligned
            return buf, view, view[0, 1:]

        xbuf, xview, xs = off_by_one(dtype, B * C)
        xs.copy_(x.to(DEV).view(-1))
        xs = xs.view(B, C)
        assert xs.data_ptr() % 16 != 0 and xs.is_contiguous()
        dbuf, dview, dx = off_by_one(dtype, B * C)
        outs = [E.guarded(1, B, B + 8, torch.float32, DEV, fill=0) for _ in range(3)]
        rbuf, rview = E.guarded(1, B, B + 8, torch.int32, DEV, fill=0)
        yg = y.to(DEV)
        g = torch.ones((), device=DEV)
        Xm.xent_fwd(xs.data_ptr(), yg.data_ptr(), 0, outs[0][1].data_ptr(), outs[1][1].data_ptr(),
                    outs[2][1].data_ptr(), rview.data_ptr(), B, C, DTYPE_CODE[dtype], 4, 0, X.MODE_MIXED, XE.EPS, 0.3, 0,
                    stream)
        Xm.xent_bwd(xs.data_ptr(), yg.data_ptr(), 0, outs[1][1].data_ptr(), outs[2][1].data_ptr(), g.data_ptr(),
                    dx.data_ptr(), B, C, DTYPE_CODE[dtype], 4, 0, X.MODE_MIXED, 0, XE.EPS, 0.3, 0, stream)
        torch.cuda.synchronize()
        assert float(dview[0, 0]) == 0 and float(xview[0, 0]) == 0  # the element in front of the slice
        got = {"loss_row": E.take_guarded("loss_row", outs[0][0], outs[0][1], errs)[0],
               "dx": E.take_guarded("dx", dbuf, dview, errs)[0, 1:].view(B, C),
               "rank": E.take_guarded("rank", rbuf, rview, errs)[0]}
        for n, (b, v) in zip(("m", "s"), outs[1:]):
            E.take_guarded(n, b, v, errs)
        assert torch.equal(E.take_guarded("x", xbuf, xview, errs)[0, 1:].view(B, C).cpu(), x)  # and x is untouched
        R = XE.refs(x, kw, "mean", 1.0, general=True)
        XE.check_all(f"slice {dtype}", got, R, errs)
        # the public call on the same slice agrees with the raw launches bit for bit
        _, _, xs2 = off_by_one(dtype, B * C)
        xs2.copy_(x.to(DEV).view(-1))
        xs2 = xs2.view(B, C).requires_grad_()
        loss = FluxMPI.softmax_cross_entropy(xs2, yg, lam=0.3, label_smoothing=XE.EPS)
        loss.backward()
        assert torch.equal(xs2.grad, got["dx"])
        XE.check_all(f"slice {dtype} public", {"loss": loss.detach()}, R, errs)
        assert not errs, "\n".join(errs)


def test_strided_view_is_made_contiguous(gpu_ext):
    base = XE.logits(3, 2000, torch.bfloat16, seed=11)
    x = base[:, ::2]
    assert not x.is_contiguous()
    kw = dict(target=XE.labels(3, 1000), label_smoothing=XE.EPS)
    bg = base.to(DEV).requires_grad_()
    loss = FluxMPI.softmax_cross_entropy(bg[:, ::2], reduction="mean", **_dev(kw))
    loss.backward()
    errs = []
    XE.check_all("view", {"loss": loss.detach(), "dx": bg.grad[:, ::2]}, XE.refs(x.contiguous(), kw), errs)
    assert not errs, "\n".join(errs)
    assert float(bg.grad[:, 1::2].abs().max()) == 0.0


# ------------------------------------------------------------------------------------ exact cases

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_constant_rows_are_exact(gpu_ext, dtype):
    """Rows of one repeated value: e_j = 1, s = C a power of two, r = 1 / C exact, so dlogits ==
    (1 / C - [j = 0]) / 4 exactly; at C = 1024 after the one rounding to bf16."""
    B = 4
    y = torch.zeros(B, dtype=torch.int64)
    for v in (0.0, 3.140625, -77.5):
        for C in (1, 2, 64, 256, 1024):
            x = torch.full((B, C), v).to(dtype)
            assert float(x[0, 0]) == v
            got = _run(x, dict(target=y), "mean", 1.0)
            want = torch.full((B, C), 1.0 / C, dtype=torch.float64)
            want[:, 0] -= 1.0
            want /= B
            if C == 1024:
                if dtype != torch.bfloat16:
                    continue
                want = want.float().to(dtype).double()
            assert torch.equal(got["dx"].cpu().double(), want), (v, C)


def test_dominant_rows_are_exact(gpu_ext):
    """C = 16, one entry +1e4 and the rest -1e4 (fp16 values): s == 1, the loss is exactly 0 where the label
    is the maximum and exactly 20000 where it is not; dlogits is 0, or +1/B at the maximum and -1/B at
    the label."""
    B, C = 4, 16
    for dtype in DTYPES:
        big = float(torch.tensor(1e4).to(dtype))
        x = torch.full((B, C), -big)
        pos = torch.tensor([3, 0, 15, 8])
        x[torch.arange(B), pos] = big
        x = x.to(dtype)
        for ldt in (torch.int32, torch.int64):
            for y in (pos, (pos + 5) % C):
                got = _run(x, dict(target=y.to(ldt)), "sum", 1.0)
                hit = bool((y == pos).all())
                rows = torch.zeros(B) if hit else torch.full((B,), 2 * big)
                assert torch.equal(got["loss_row"].cpu(), rows)
                assert float(got["loss"]) == float(rows.sum())
                want = torch.zeros(B, C)
                if not hit:
                    want[torch.arange(B), pos] = 1.0
                    want[torch.arange(B), y] = -1.0
                assert torch.equal(got["dx"].cpu().float(), want)
                got = _run(x, dict(target=y.to(ldt)), "mean", 1.0)
                assert torch.equal(got["dx"].cpu().float(), want / B)
                assert torch.equal(got["rank"].cpu(), X.xent_reference(x, y)[3])
                assert not hit or int(got["rank"].abs().sum()) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_rank_equals_the_reference(gpu_ext, dtype):
    """Random rows (16-bit logits tie by themselves) and planted ties, on both paths."""
    for B, C in ((9, 40), (9, 64), (5, 1000), (3, 8200)):
        y = XE.labels(B, C, seed=2, dtype=torch.int32)
        for x in (XE.logits(B, C, dtype, seed=2), XE.plant_ties(XE.logits(B, C, dtype, seed=3), y)):
            want = X.xent_reference(x, y)[3]
            _, got = FluxMPI.softmax_cross_entropy(x.to(DEV), y.to(DEV), return_rank=True)
            assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), (B, C)
            t = XE.dense_target(B, C)
            _, got = FluxMPI.softmax_cross_entropy(x.to(DEV), t.to(DEV), labels=y.to(DEV), return_rank=True)
            assert torch.equal(got.cpu(), want), (B, C, "dense")


# ------------------------------------------------------------------------------- the other tests

def test_loss_bits_repeat(gpu_ext):
    x = XE.logits(1000, 1000, torch.bfloat16, seed=5).to(DEV)
    y = XE.labels(1000, 1000).to(DEV)
    a = FluxMPI.softmax_cross_entropy(x, y, label_smoothing=XE.EPS)
    b = FluxMPI.softmax_cross_entropy(x, y, label_smoothing=XE.EPS)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_meter_accumulates_on_the_device(gpu_ext):
    meter = FluxMPI.ClassificationMeter(topk=(1, 5))
    C = 1000
    tot, bound, rows, c1, c5 = 0.0, 0.0, 0, 0, 0
    for i, B in enumerate((5, 257, 64)):
        x, y = XE.logits(B, C, torch.bfloat16, seed=i, scale=1.0), XE.labels(B, C, seed=i)
        x[0, int(y[0])] = 9.0  # at least one hit
        with torch.no_grad():  # the evaluation loop
            loss = FluxMPI.softmax_cross_entropy(x.to(DEV), y.to(DEV), meter=meter)
        assert not loss.requires_grad
        R = XE.refs(x, dict(target=y), "sum")
        tot, bound, rows = tot + float(R["loss"]), bound + float(R["b_loss"]), rows + B
        c1, c5 = c1 + int((R["rank"] < 1).sum()), c5 + int((R["rank"] < 5).sum())
    assert meter.block.is_cuda and meter.block.numel() == 4
    got = meter.read()
    assert got["rows"] == rows and got["top1"] == c1 / rows and got["top5"] == c5 / rows and c1 > 0
    assert abs(got["loss"] * rows - tot) <= bound, (got["loss"] * rows, tot, bound)
    meter.reset()
    assert meter.read()["rows"] == 0 and int(meter.block.abs().sum()) == 0


def test_graph_capture_follows_its_inputs(gpu_ext):
    """Forward, the multiply by a device scalar, backward and the meter update captured once; after the
    logits, the labels and the device lam word change in place a replay equals the eager run bit for bit."""
    B, C = 32, 1000
    x = XE.logits(B, C, torch.bfloat16, seed=1).to(DEV).requires_grad_()
    y = XE.labels(B, C, seed=1).to(DEV)
    lam = torch.tensor(0.3, device=DEV)
    scale = torch.tensor(BIG, device=DEV)
    meter = FluxMPI.ClassificationMeter().to(DEV)

    def step(m):
        x.grad = None
        loss = FluxMPI.softmax_cross_entropy(x, X.MixedLabels(y, lam, XE.EPS), meter=m)
        (loss * scale).backward()
        return loss.detach(), x.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(FluxMPI.ClassificationMeter().to(DEV))  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_loss, g_grad = step(meter)
    with torch.no_grad():
        x.copy_(XE.logits(B, C, torch.bfloat16, seed=2).to(DEV))
        y.copy_(XE.labels(B, C, seed=2).to(DEV))
        lam.fill_(0.75)
    meter.reset()
    graph.replay()
    torch.cuda.synchronize()
    replay = (g_loss.clone(), g_grad.clone(), meter.read())
    eager_meter = FluxMPI.ClassificationMeter().to(DEV)
    e_loss, e_grad = step(eager_meter)
    assert torch.equal(replay[0].view(torch.int32), e_loss.view(torch.int32))
    assert torch.equal(replay[1].view(torch.int16), e_grad.view(torch.int16))
    assert replay[2] == eager_meter.read() and replay[2]["rows"] == B


def test_one_ddp_step_with_the_fused_loss(gpu_ext):
    """A 64-128-10 fp32 MLP under DDP(loss_scale="dynamic"), plain gradient descent, one step with the fused
    loss inside ``ddp.scale_loss`` against the same step through ``F.cross_entropy``.

    Tolerance. Both losses' dlogits lie within the derived bound b = b_dx of the float64 value (torch's
    own composition is taken to meet it too), so they differ by at most D = 2 b; the loss scale, a power
    of two, cancels exactly. With h the hidden activations the head's gradients then differ by at most
    dW2 <= D^T |h| and db2 <= sum_b D, the hidden gradient by D |W2| (tanh' <= 1), the first layer's by
    (D |W2|)^T |x| and its column sums; each fp32 GEMM adds its own rounding on both sides, 2 K E times the
    same products of absolute values with K the reduction length. A parameter moves by lr times that,
    plus 4u (|p| + lr |g|) for the update's own roundings."""
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    from .loss_scale_cases import mlp
    B, lr = 16, 0.5
    x = torch.randn(B, 64, generator=torch.Generator().manual_seed(3))
    y = XE.labels(B, 10, seed=4)
    after, logits0 = [], None
    for fused in (True, False):
        d = DDP(mlp(0, DEV), O.Descent(lr), loss_scale="dynamic")
        before = [p.detach().cpu().clone() for p in d.module.parameters()]
        logits = d(x.to(DEV))
        logits0 = logits.detach().cpu()
        loss = (FluxMPI.softmax_cross_entropy(logits, y.to(DEV)) if fused
                else F.cross_entropy(logits.float(), y.to(DEV)))
        d.scale_loss(loss).backward()
        d.step()
        assert int(d.step_skipped()) == 0
        after.append([p.detach().cpu().clone() for p in d.module.parameters()])
    R = XE.refs(logits0, dict(target=y))
    D = 2 * R["b_dx"]
    w1, b1, w2, b2 = (p.double() for p in before)
    xa = x.double().abs()
    h = torch.tanh(x.double() @ w1.t() + b1).abs()
    dxa = R["dx"].abs()
    dh = D @ w2.abs()
    dha = dxa @ w2.abs()
    e23, u = E.E23, XE.U32
    tol_g = [dh.t() @ xa + 2 * B * e23 * (dha.t() @ xa) + 2 * 10 * e23 * (dha.t() @ xa),
             dh.sum(0) + 2 * (B + 10) * e23 * dha.sum(0),
             D.t() @ h + 2 * B * e23 * (dxa.t() @ h),
             D.sum(0) + 2 * B * e23 * dxa.sum(0)]
    moved = False
    for p0, pa, pb, tg in zip(before, after[0], after[1], tol_g):
        step_size = (pa.double() - p0.double()).abs()
        tol = lr * tg + 4 * u * (p0.double().abs() + step_size) + E.TINY
        err = (pa.double() - pb.double()).abs()
        assert bool((err <= tol).all()), float((err / tol).max())
        moved = moved or float(step_size.max()) > 0
    assert moved
