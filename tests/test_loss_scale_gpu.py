"""Dynamic loss scaling and the non-finite step skip on the GPU: the exact per-element check
(``mt_check_finite`` and the check inside the sum-of-squares pass), the skip predicate of every
update kernel, the scaler update, and the DDP engine — exact unscaling, the skip, fp16 end to end
and HIP-graph replay."""
import pytest
import torch

from tests import loss_scale_cases as LS
from tests.test_clip_gpu import SIZES, UNALIGNED, _acc, _to_dev
from tests.test_loss_scale import scaler_script
from tests.test_rules_gpu import HYPER, KINDS, _leaves

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64]
BAD = [float("inf"), float("-inf"), float("nan")]
LAST = len(SIZES) - 1
# (leaf, element): element 0 of leaf 0; the last element of the last leaf (second launch group: 29
# leaves have elements, 24 go into the first launch); the 4097-element leaf's last vector element
# and its one-element scalar chunk; the 100-element leaf's last vector element (95) and first
# scalar-tail element (96); the last chunk of the multi-chunk leaf; the unaligned leaf (scalar path)
# at both ends and inside
SPOTS = [(0, 0), (LAST, SIZES[LAST] - 1), (4, 4095), (4, 4096), (8, 95), (8, 96), (5, 3 * 4096 + 2),
         (UNALIGNED, 0), (UNALIGNED, 2500), (UNALIGNED, SIZES[UNALIGNED] - 1)]


def _flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _extremes(dtype):
    """Leaves holding only the extremes: largest finite of each sign, smallest normal, subnormals, +-0."""
    fi = torch.finfo(dtype)
    sub = fi.tiny * fi.eps  # the smallest subnormal
    vals = torch.tensor([fi.max, -fi.max, fi.tiny, -fi.tiny, sub, -sub, 0.0, -0.0], dtype=torch.float64).to(dtype)
    assert bool(torch.isfinite(vals).all()) and float(vals[0]) == fi.max and 0 < float(vals[4]) < fi.tiny
    return [vals.repeat((n + 7) // 8)[:n].clone() for n in SIZES]


# ---------------------------------------------------------------- 1. the check
@pytest.mark.parametrize("dtype", DTYPES)
def test_check_finite_finds_every_planted_value(gpu_ext, dtype):
    from fluxmpi_amd.ops import optim
    gs = _to_dev(_leaves(0), dtype)
    assert len(gs) == 30 and gs[14].numel() == 0 and SIZES[4] == 4097 and SIZES[8] == 100
    flag = _flag()
    optim.check_finite_(gs, flag)
    assert int(flag) == 0  # clean leaves
    for bad in BAD:
        for leaf, el in SPOTS:
            keep = gs[leaf][el].clone()
            gs[leaf][el] = bad
            flag.zero_()
            optim.check_finite_(gs, flag)
            assert int(flag) == 1, (bad, leaf, el)
            gs[leaf][el] = keep
    flag.zero_()
    optim.check_finite_(gs, flag)
    assert int(flag) == 0  # every planted value was taken out again
    # sticky: after a dirty call, a clean call leaves the flag at 1
    gs[3][17] = float("nan")
    optim.check_finite_(gs, flag)
    gs[3][17] = 0.0
    optim.check_finite_(gs, flag)
    assert int(flag) == 1
    with pytest.raises(TypeError):
        optim.check_finite_(gs, torch.zeros(1, device="cuda"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_extremes_are_finite_though_their_squares_are_not(gpu_ext, dtype):
    from fluxmpi_amd.ops import optim
    gs = _to_dev(_extremes(dtype), dtype)
    flag = _flag()
    optim.check_finite_(gs, flag)
    assert int(flag) == 0
    out = torch.zeros(len(gs), dtype=_acc(dtype), device="cuda")
    optim.sumsq_(gs, out, flag=flag)
    assert int(flag) == 0
    if dtype in (torch.bfloat16, torch.float32):  # the reason the check is per element
        assert bool(torch.isinf(out[torch.tensor([n > 0 for n in SIZES], device="cuda")]).all())
    else:  # fp16 squares fit fp32; fp64's overflow fp64
        assert bool(torch.isinf(out[4])) == (dtype == torch.float64)


# ---------------------------------------------------------------- 2. the check inside the norm pass
@pytest.mark.parametrize("dtype", DTYPES)
def test_sumsq_with_flag_and_dev_pre(gpu_ext, dtype):
    from fluxmpi_amd.ops import optim
    at = _acc(dtype)
    gs = _to_dev(_leaves(0), dtype)
    n = len(gs)
    plain, fused = torch.zeros(2, n, dtype=at, device="cuda"), torch.full((2, n), -1.0, dtype=at, device="cuda")
    flag = _flag()
    optim.sumsq_(gs, plain[0], scales=plain[1], omega=10.0, grad_scale=0.5)
    optim.sumsq_(gs, fused[0], scales=fused[1], omega=10.0, grad_scale=0.5, flag=flag)
    assert torch.equal(plain, fused) and int(flag) == 0
    for bad in BAD:
        for leaf, el in SPOTS:
            keep = gs[leaf][el].clone()
            gs[leaf][el] = bad
            flag.zero_()
            optim.sumsq_(gs, fused[0], flag=flag)
            assert int(flag) == 1, (bad, leaf, el)
            gs[leaf][el] = keep
    optim.sumsq_(gs, fused[0], flag=flag)
    assert int(flag) == 1  # sticky here too
    # dev_pre = 2^-10: the scales of the gradients divided by 1024 (omega: exact in fp32, as the kernel takes it)
    pre, om = torch.tensor([2.0 ** -10], device="cuda"), 2.0 ** -6
    optim.sumsq_(gs, fused[0], scales=fused[1], omega=om, grad_scale=0.5, dev_pre=pre)
    want = optim.clip_scales_reference(optim.sumsq_reference([g.double() / 1024 for g in gs]), om, 0.5)
    assert (want < 1).any() and (want == 1).any()
    torch.testing.assert_close(fused[1].double().cpu(), want, rtol=1e-12 if dtype == torch.float64 else 1e-5, atol=0)
    assert torch.equal(fused[0], plain[0])  # the sums stay raw
    if dtype in (torch.float32, torch.float64):  # g / 1024 is exact: the same bits as the call on it
        small = _to_dev([t / 1024 for t in _leaves(0)], dtype)  # the same alignment, leaf by leaf
        optim.sumsq_(small, plain[0], scales=plain[1], omega=om, grad_scale=0.5)
        assert torch.equal(plain[1], fused[1])
    slot_a, slot_b = torch.zeros(3, device="cuda"), torch.zeros(3, device="cuda")
    optim.clip_total_(fused[0], slot_a, omega=om, grad_scale=0.5)
    optim.clip_total_(fused[0], slot_b, omega=om / 1024, grad_scale=0.5, dev_pre=pre)
    assert slot_a[0] == slot_b[0] and slot_b[1] == slot_a[1] / 1024 and slot_b[2] == slot_a[2] / 1024 > 0


# ---------------------------------------------------------------- 3. the skip predicate
SKIP_COMBOS = [(torch.bfloat16, torch.bfloat16, torch.float32, True), (torch.float16, torch.float16, torch.float32, True),
               (torch.float32, torch.float32, torch.float32, False), (torch.bfloat16, torch.bfloat16, torch.bfloat16, False)]
SKIP_KINDS = ["adam", "descent", "momentum", "nesterov", *KINDS, "lars", "lamb", "lars_fold_launch", "lamb_fold_launch"]


class _Job:
    """One update call's tensors on the device (the clip tests' leaf set, the offset leaf unaligned
    in every list) and the call itself."""

    def __init__(self, kind, pd, gd, sd, master):
        self.kind = kind.split("_")[0]
        self.p, self.g = _to_dev(_leaves(1), pd), _to_dev(_leaves(0), gd)
        self.s = [_to_dev([t.abs() * 0.1 for t in _leaves(40 + k)], sd) for k in range(3)]
        self.w = _to_dev([t.to(pd).float() for t in _leaves(1)], torch.float32) if master else None
        at = _acc(pd)
        self.ratios = torch.full((len(SIZES),), 0.375, dtype=at, device="cuda")
        self.ratios[SIZES.index(0)] = 1  # a leaf without elements: always 1
        self.hyper = torch.tensor([1e-3, 0.9 ** 3, 0.999 ** 3], device="cuda")

    def tensors(self):
        return [*self.p, *(t for s in self.s for t in s), *(self.w or []), self.ratios, self.hyper]

    def snapshot(self):
        return [t.clone() for t in self.tensors()]

    def call(self, **kw):
        from fluxmpi_amd.ops import optim
        k, p, g, s, w = self.kind, self.p, self.g, self.s, self.w
        if k == "adam":
            optim.adam_(p, g, s[0], s[1], lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, bc1=0.0, bc2=0.0,
                        weight_decay=0.01, masters=w, dev_hyper=self.hyper, **kw)
        elif k in ("descent", "momentum", "nesterov"):
            optim.sgd_(p, g, s[0], lr=1e-2, momentum=0.0 if k == "descent" else 0.9, nesterov=k == "nesterov",
                       masters=w, **kw)
        elif k == "lars":
            optim.lars_(p, g, s[0], lr=0.1, momentum=0.9, trust=0.02, weight_decay=0.01, eps=1e-9, masters=w,
                        ratios=self.ratios, **kw)
        elif k == "lamb":
            optim.lamb_(p, g, s[0], s[1], lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-6, bt1=0.0, bt2=0.0,
                        weight_decay=0.01, masters=w, dev_hyper=self.hyper, ratios=self.ratios, **kw)
        else:
            ns = optim.RULES[k][1]
            h = dict(HYPER[k])
            if optim.RULES[k][2]:
                h.update(bt1=0.9 ** 3, bt2=0.999 ** 3)
            optim.rule_(k, p, g, s[:ns], masters=w, **h, **kw)
        optim.adam_advance_(self.hyper, 0.9, 0.999, **kw)


# (Descent keeps no state, and the kernels are built for an fp32 master only beside fp32 states)
@pytest.mark.parametrize("kind,pd,gd,sd,master", [(k, *c) for k in SKIP_KINDS for c in SKIP_COMBOS
                                                  if not (k == "descent" and c[3])])
def test_skip_predicate(gpu_ext, monkeypatch, kind, pd, gd, sd, master):
    """dev_skip -> 1: nothing is written (parameters, masters, every state tensor, the ratio table,
    the hyper block after adam_advance_). dev_skip -> 0: the bits of the call without dev_skip."""
    if kind.endswith("_fold_launch"):
        monkeypatch.setenv("FLUXMPI_LAYERWISE_FOLD", "launch")  # the fold as a launch of its own
    skip = torch.ones(1, dtype=torch.int32, device="cuda")
    a, b = _Job(kind, pd, gd, sd, master), _Job(kind, pd, gd, sd, master)
    before = a.snapshot()
    a.call(dev_skip=skip)
    assert all(torch.equal(x, y) for x, y in zip(before, a.tensors())), "a skipped call wrote something"
    assert int(skip) == 1
    skip.zero_()
    a.call(dev_skip=skip)
    b.call()
    after = a.tensors()
    assert all(torch.equal(x, y) for x, y in zip(after, b.tensors()))
    changed = [not torch.equal(x, y) for x, y in zip(before, after)]
    # (a bf16 parameter may round back to itself; its master and the states do not)
    assert sum(changed) >= 20 and any(changed[:len(SIZES)]) and changed[-1], "the unskipped call moves things"


# ---------------------------------------------------------------- 4. the scaler update
def test_loss_scale_update_follows_the_script(gpu_ext):
    from fluxmpi_amd.ops import optim
    scaler_script(optim.loss_scale_update_, "cuda")


def test_loss_scale_update_matches_the_reference_bit_for_bit(gpu_ext):
    """Factors that are no powers of two, a scripted flag sequence: scale, inverse and counters."""
    from fluxmpi_amd.ops import optim
    kw = dict(growth=1.7, backoff=0.3, interval=3, min_scale=1.0, max_scale=300.0)
    dev, ref = optim.loss_scale_block(100.0, "cuda"), optim.loss_scale_block(100.0, "cpu")
    low = 100.0
    for flag in [0, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0] + [0] * 36:
        dev[optim.LS_FLAG] = flag
        ref[optim.LS_FLAG] = flag
        optim.loss_scale_update_(dev, **kw)
        optim.loss_scale_update_reference_(ref, **kw)
        assert torch.equal(dev.cpu(), ref), (flag, dev.cpu().view(torch.float32)[:2], ref.view(torch.float32)[:2])
        low = min(low, float(ref.view(torch.float32)[0]))
    # 86.7 x 0.3^7 is below min_scale; 1.7^13 is above max_scale
    assert low == 1.0 and float(ref.view(torch.float32)[0]) == 300.0 and int(ref[optim.LS_SKIPPED]) == 8


# ---------------------------------------------------------------- 5. / 6. / 9. the engine
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["adam", "momentum", "clipnorm", "global", "lamb"])
def test_engine_exact_unscaling(gpu_ext, name, dtype):
    LS.case_exact_unscaling(name, "cuda", dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["adam", "momentum", "clipnorm", "global", "lamb"])
def test_engine_skips_a_non_finite_step(gpu_ext, name, dtype):
    LS.case_skip(name, "cuda", dtype)


def test_engine_errors(gpu_ext):
    LS.case_errors("cuda")


def test_engine_launches_nothing_new_without_loss_scale(gpu_ext, monkeypatch):
    from fluxmpi_amd.ops import optim
    d = LS.engine("adam", "cuda", torch.bfloat16)
    assert d._ls is None and d._ls_block is None
    called = []
    monkeypatch.setattr(optim, "check_finite_", lambda *a, **k: called.append("check"))
    monkeypatch.setattr(optim, "loss_scale_update_", lambda *a, **k: called.append("update"))
    LS.give(d, LS.step_grads(d, 0))
    d.step()
    assert called == []
    e = LS.engine("adam", "cuda", torch.bfloat16, loss_scale=1.0)
    LS.give(e, LS.step_grads(e, 0))
    e.step()
    assert called == ["check", "update"]  # one check pass over all buckets, one scaler launch


# ---------------------------------------------------------------- 7. fp16 end to end
def _fp16_data():
    g = torch.Generator().manual_seed(31)
    x = torch.randn(32, 64, generator=g)
    return x.cuda(), torch.randn(32, 10, generator=g).cuda()


def _train(dtype, c, steps, loss_scale=None):
    """``steps`` Adam steps of the 64-128-10 MLP on ``c * mse``; returns the engine."""
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    d = DDP(LS.mlp(2, "cuda", dtype), O.Adam(1e-3), loss_scale=loss_scale, **LS.SMALL)
    x, y = _fp16_data()
    for _ in range(steps):
        loss = ((d(x.to(dtype)).float() - y) ** 2).mean() * c
        d.scale_loss(loss).backward()
        d.step()
    return d


def _weights(d):
    """What the engine trains, in fp32 and in the order of the parameter names: the masters of a
    16-bit model, else the parameters (the bucket layout differs between the dtypes)."""
    out = {}
    for b in d.buckets:
        src = b.master if b.master is not None else b.flat_param
        for name, p, o in zip(b.names, b.params, b.offsets):
            out[name] = src[o:o + p.numel()].float()
    return torch.cat([out[k] for k in sorted(out)])


def test_fp16_trains_through_underflow_with_a_loss_scale(gpu_ext):
    """c = 2^-26 puts every fp16 gradient of the MLP below half the smallest fp16 subnormal: without
    a loss scale they are all zero and nothing moves. With 2^16 the masters follow the fp32 model.

    Allowance: twice the largest difference between the fp16 model's masters and the fp32 model's
    parameters after the same 5 steps at c = 1, where nothing underflows (fp16 rounding of
    activations and gradients), measured in the test. Measured on the MI355X: allowance
    2 x 2.138e-03 = 4.276e-03; the scaled run's largest difference 3.242e-05 (the masters moved by
    up to 5.36e-04)."""
    c, steps = 2.0 ** -26, 5
    start = _weights(_train(torch.float16, c, 0))
    d0 = _train(torch.float16, c, 0)
    x, y = _fp16_data()
    (((d0(x.half()).float() - y) ** 2).mean() * c).backward()
    assert all(p.grad is not None and not bool(p.grad.any()) for p in d0.module.parameters()), "fp16 gradients underflow"
    assert torch.equal(_weights(_train(torch.float16, c, steps)), start), "zero gradients: Adam does not move"
    base = float((_weights(_train(torch.float16, 1.0, steps)) - _weights(_train(torch.float32, 1.0, steps))).abs().max())
    scaled = _train(torch.float16, c, steps, loss_scale=2.0 ** 16)
    want = _weights(_train(torch.float32, c, steps))
    err = float((_weights(scaled) - want).abs().max())
    moved = float((_weights(scaled) - start).abs().max())
    print(f"fp16 vs fp32 at c=1: {base:.3e}; allowance {2 * base:.3e}; scaled run: {err:.3e}; moved {moved:.3e}")
    assert int(scaled.skipped_steps()) == 0 and float(scaled.loss_scale()) == 2.0 ** 16
    assert moved > 1e-4 and float((want - start).abs().max()) > 1e-4
    assert err <= 2 * base


def test_fp16_overflowing_scale_backs_off_until_a_step_fits(gpu_ext):
    """LossScale(init=2^24) on the plain loss: the first backwards overflow fp16. The parameters stay
    bit-identical through the skipped steps, every skip halves the scale, the first clean step moves."""
    from fluxmpi_amd import LossScale
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    d = DDP(LS.mlp(2, "cuda", torch.float16), O.Adam(1e-3), loss_scale=LossScale(init=2.0 ** 24), **LS.SMALL)
    x, y = _fp16_data()
    start, skips = LS.state(d), 0
    for _ in range(24):
        d.scale_loss(((d(x.half()).float() - y) ** 2).mean()).backward()
        d.step()
        if int(d.step_skipped()) == 0:
            break
        skips += 1
        assert LS.same(start, LS.state(d)), "a skipped step wrote something"
    scale = float(d.loss_scale())
    print(f"{skips} skipped steps, scale 2^{torch.tensor(scale).log2().item():.0f}")
    assert skips >= 1 and int(d.skipped_steps()) == skips and scale == 2.0 ** (24 - skips) and int(d.step_skipped()) == 0
    assert not LS.same(start, LS.state(d))
    assert all(bool(torch.isfinite(t.float()).all()) for t in LS.state(d))


# ---------------------------------------------------------------- 8. HIP-graph replay
@pytest.mark.parametrize("mode", ["clipnorm", "adam"])
def test_graphed_step_scales_skips_and_proceeds(gpu_ext, mode):
    """GraphedStep with loss_fn returning ddp.scale_loss(loss): the replays equal a twin's eager
    steps bit for bit, through growths of the scale (interval 3), a replay fed an input that makes
    the loss non-finite (skipped, read from the device counters) and the replay after it."""
    import torch.nn.functional as F
    from fluxmpi_amd import LossScale
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    from fluxmpi_amd.parallel.graph import GraphedStep

    def make():
        # the check inside the norm pass (clipnorm) and as a pass of its own (adam)
        rule = O.OptimiserChain(O.ClipNorm(0.3), O.Adam(1e-2)) if mode == "clipnorm" else O.Adam(1e-2)
        return DDP(LS.mlp(4, "cuda"), rule, loss_scale=LossScale(init=1024.0, interval=3), **LS.SMALL)

    def loss_fn(d, xx, yy):
        return d.scale_loss(F.mse_loss(d(xx), yy))

    d1, d2 = make(), make()
    x, y = _fp16_data()
    bad = x.clone()
    bad[0, 0] = float("inf")
    g = GraphedStep(d1, loss_fn, x, y, warmup=2)
    for _ in range(2):
        loss_fn(d2, x, y).backward()
        d2.step()
    for i, xx in enumerate([x, x, x, bad, x, x, x, x]):
        g(xx, y)
        loss_fn(d2, xx, y).backward()
        before = LS.state(d2)
        d2.step()
        torch.cuda.synchronize()
        assert LS.same(LS.state(d1), LS.state(d2)), i
        assert torch.equal(d1._ls_block, d2._ls_block)
        if mode == "clipnorm" and i != 3:  # (the skipped step's norm is NaN on both)
            assert torch.equal(d1.grad_norm(), d2.grad_norm())
        assert int(d1.step_skipped()) == int(i == 3) and int(d1.skipped_steps()) == int(i >= 3)
        assert LS.same(before, LS.state(d2)) == (i == 3)
    # 2 warm-up steps + replay 0: grown to 2048; replay 3: back to 1024; replays 4 - 6: 2048 again
    assert float(d1.loss_scale()) == float(d2.loss_scale()) == 2048.0
