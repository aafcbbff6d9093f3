"""Stochastic rounding on the GPU: ``stochastic_round_`` and the ``sr=`` instantiations of the fused update
kernels bit for bit against ``ops.philox.sr_reference``, a stalled bf16 update that moves, and
``DDP(master_weights=False, stochastic_rounding=...)`` (reproducible, graph replay, ``overlap_opt``, the
flat and the per-leaf route, a skipped step, and the option switched off)."""
import pytest
import torch

from fluxmpi_amd.ops import optim as fused
from fluxmpi_amd.ops import philox
from tests import loss_scale_cases as LS
from tests import test_sr as TS

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
bits16 = TS.bits16


# ---------------------------------------------------------------- the stand-alone cast
SIZES = [1, 7, 8, 9, 4095, 4096, 4097, 8200]
OFFSETS = [0, 8, 3]
CAST = dict(seed=(0xABCDEF12 << 32) | 0x3456789A, stream=6, step=5)


@pytest.fixture(scope="module")
def cast_case():
    """25 leaves (two launches): every size, every fourth leaf a slice 2 bytes (dst) / 4 bytes (src) off
    16-byte alignment, offsets 0 / 8 / 3. The expected bits, computed once."""
    g = torch.Generator().manual_seed(21)
    sizes = [SIZES[i % len(SIZES)] for i in range(25)]
    offs = [OFFSETS[i % 3] for i in range(25)]
    shift = [1 if i % 4 == 1 else 0 for i in range(25)]
    xs = [torch.randn(n, generator=g) * 2.0 ** float(torch.randint(-20, 20, (1,), generator=g)) for n in sizes]
    xs[3][:4] = torch.tensor([float("inf"), float("nan"), -0.0, 3.3e38])
    want = [philox.sr_reference(x, CAST["seed"], CAST["stream"], 0, CAST["step"], o) for x, o in zip(xs, offs)]
    assert {(n, o % 8 == 0, s) for n, o, s in zip(sizes, offs, shift)} >= {(4097, True, 0), (4097, False, 0)}
    return sizes, offs, shift, xs, want


def _cast_buffers(sizes, shift, xs):
    src, dst = [], []
    for n, s, x in zip(sizes, shift, xs):
        xb = torch.zeros(n + 8, device="cuda")
        db = torch.full((n + 8,), float("nan"), dtype=BF, device="cuda")
        xb[s:s + n] = x.cuda()
        src.append(xb[s:s + n])
        dst.append(db[s:s + n])
        assert (dst[-1].data_ptr() % 16 != 0) == bool(s)
    return src, dst


@pytest.mark.parametrize("source", ["host", "block"])
def test_stochastic_round_bit_exact(gpu_ext, cast_case, source):
    sizes, offs, shift, xs, want = cast_case
    src, dst = _cast_buffers(sizes, shift, xs)
    if source == "host":
        sr = fused.SR(CAST["seed"], stream=CAST["stream"], step=CAST["step"], offsets=offs)
    else:  # the device block wins over the host step
        sr = fused.SR(CAST["seed"], stream=CAST["stream"], step=1234, offsets=offs,
                      dev_block=fused.sr_block("cuda", step=CAST["step"]))
    skip = torch.ones(1, dtype=torch.int32, device="cuda")
    fused.stochastic_round_(dst, src, sr, dev_skip=skip)
    assert all(bool(torch.isnan(d).all()) for d in dst), "a skipped launch wrote"
    skip.zero_()
    fused.stochastic_round_(dst, src, sr, dev_skip=skip)
    for i, (d, w) in enumerate(zip(dst, want)):
        TS.assert_bits(d, w, (i, sizes[i], offs[i], shift[i]))
    dst2 = [torch.full_like(d, float("nan")) for d in dst]
    fused.stochastic_round_(dst2, src, sr)  # no predicate: the other instantiation
    for i, (d, w) in enumerate(zip(dst2, want)):
        TS.assert_bits(d, w, i)


def test_sr_advance_on_the_device(gpu_ext):
    blk = fused.sr_block("cuda", step=(1 << 32) - 2)
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    fused.sr_advance_(blk, dev_skip=flag)
    assert int(blk[0]) & 0xFFFFFFFF == (1 << 32) - 2
    fused.sr_advance_(blk)
    fused.sr_advance_(blk, dev_skip=flag.zero_())
    assert int(blk[0]) == 0 and bool(blk[1:].eq(0).all())  # a uint32 wraps


# ---------------------------------------------------------------- the update kernels
LEAVES = [4097, 8, 5]
LEAF_OFF = [0, 4104, 4112 + 3]  # the last one off a multiple of 8: the scalar path draws the same bits
SEED, STREAM = 0x1234567887654321, 9
HYP = dict(lr=1e-2, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.01, grad_scale=0.5)
KINDS = ["adam", "momentum", "nesterov", "descent"] + sorted(fused.RULES)


def _nstates(kind):
    return {"adam": 2, "momentum": 1, "nesterov": 1, "descent": 0}.get(kind) if kind not in fused.RULES \
        else fused.RULES[kind][1]


def _run(kind, p, g, st, **kw):
    if kind == "adam":
        fused.adam_(p, g, st[0], st[1], bc1=1 - 0.9 ** 3, bc2=1 - 0.99 ** 3, **HYP, **kw)
    elif kind in fused.RULES:
        fused.rule_(kind, p, g, st, bt1=0.9 ** 3, bt2=0.99 ** 3, **HYP, **kw)
    else:
        fused.sgd_(p, g, st[0] if st else [], lr=HYP["lr"], momentum=0.0 if kind == "descent" else 0.9,
                   nesterov=kind == "nesterov", weight_decay=HYP["weight_decay"], grad_scale=HYP["grad_scale"], **kw)


@pytest.mark.parametrize("kind", KINDS)
def test_update_kernels_bit_exact(gpu_ext, kind):
    """No CPU copy of the rule: the existing (fp32, bf16, fp32, no master) instantiation on fp32 copies of
    bf16 values writes the pre-rounding values of the same expressions; the sr kernels must store
    sr_reference of those (slot 0 the parameter, 1..3 the states)."""
    ns = _nstates(kind)
    gen = torch.Generator().manual_seed(31)
    p0 = [torch.randn(n, generator=gen).to(BF).cuda() for n in LEAVES]
    g0 = [(torch.randn(n, generator=gen) * 0.3).to(BF).cuda() for n in LEAVES]
    s0 = [[(torch.randn(n, generator=gen).abs() * 0.05 + 1e-3).to(BF).cuda() for n in LEAVES] for _ in range(ns)]
    pf = [t.float() for t in p0]
    sf = [[t.float() for t in l] for l in s0]
    _run(kind, pf, g0, sf)  # the twin: round to nearest has nothing to round here
    torch.cuda.synchronize()
    assert not any(torch.equal(a.to(BF).float(), a) for a in pf[:1])  # the update left the bf16 grid
    for step, use_block in ((0, False), (7, True)):
        mk = lambda: fused.SR(SEED, stream=STREAM, offsets=LEAF_OFF,  # noqa: E731
                              **({"dev_block": fused.sr_block("cuda", step=step)} if use_block else {"step": step}))
        want_p = [philox.sr_reference(x, SEED, STREAM, 0, step, o) for x, o in zip(pf, LEAF_OFF)]
        # (bf16, bf16, bf16, no master): every store rounds stochastically
        p, st = [t.clone() for t in p0], [[t.clone() for t in l] for l in s0]
        _run(kind, p, g0, st, sr=mk())
        for i in range(len(LEAVES)):
            assert torch.equal(bits16(p[i]), bits16(want_p[i])), (kind, "p", i, step)
            for k in range(ns):
                want = philox.sr_reference(sf[k][i], SEED, STREAM, k + 1, step, LEAF_OFF[i])
                assert torch.equal(bits16(st[k][i]), bits16(want)), (kind, "state", k, i, step)
        # (bf16, bf16, fp32, no master): the states are the twin's bits
        p, st = [t.clone() for t in p0], [[t.float() for t in l] for l in s0]
        _run(kind, p, g0, st, sr=mk())
        for i in range(len(LEAVES)):
            assert torch.equal(bits16(p[i]), bits16(want_p[i])), (kind, "p / fp32 states", i, step)
            for k in range(ns):
                assert torch.equal(st[k][i], sf[k][i]), (kind, "fp32 state", k, i, step)
    # with the predicate set nothing is written
    p, st = [t.clone() for t in p0], [[t.clone() for t in l] for l in s0]
    _run(kind, p, g0, st, sr=mk(), dev_skip=torch.ones(1, dtype=torch.int32, device="cuda"))
    assert all(torch.equal(a, b) for a, b in zip(p + [t for l in st for t in l], p0 + [t for l in s0 for t in l]))


def test_update_errors_on_the_gpu(gpu_ext):
    p = [torch.zeros(8, dtype=BF, device="cuda")]
    with pytest.raises(ValueError):
        fused.sgd_(p, p, [], lr=0.1, masters=[p[0].float()], sr=fused.SR(0))
    h = [torch.zeros(8, dtype=torch.float16, device="cuda")]
    with pytest.raises(TypeError):
        fused.sgd_(h, h, [], lr=0.1, sr=fused.SR(0))


# ---------------------------------------------------------------- a stalled update moves
def test_stalled_update_moves(gpu_ext):
    """Descent, p = 1.0, g = 1, lr = 2^-12 (a 16th of the bf16 ulp 2^-8 below 1), 256 steps: round to
    nearest leaves 1.0; under SR the mean of 4096 elements is 1 - 256 * 2^-12 = 0.9375 within 3e-3 (per step
    error variance <= (2^-8)^2 / 4, 256 steps: sigma <= 2^-5 per element, 4.9e-4 over 4096; six of those)."""
    n, steps, lr = 4096, 256, 2.0 ** -12
    g = [torch.ones(n, dtype=BF, device="cuda")]
    rn = [torch.ones(n, dtype=BF, device="cuda")]
    sr_p = [torch.ones(n, dtype=BF, device="cuda")]
    blk = fused.sr_block("cuda")
    sr = fused.SR(42, stream=1, dev_block=blk)
    for _ in range(steps):
        fused.sgd_(rn, g, [], lr=lr)
        fused.sgd_(sr_p, g, [], lr=lr, sr=sr)
        fused.sr_advance_(blk)
    assert bool((rn[0].float() == 1.0).all())
    assert int(blk[0]) == steps
    mean = float(sr_p[0].double().mean())
    print(f"mean after {steps} steps: {mean:.6f}")
    assert abs(mean - 0.9375) <= 3e-3
    cpu_p, cpu_g, cblk = [torch.ones(n, dtype=BF)], [torch.ones(n, dtype=BF)], fused.sr_block("cpu")
    for _ in range(steps):
        fused.sgd_(cpu_p, cpu_g, [], lr=lr, sr=fused.SR(42, stream=1, dev_block=cblk))
        fused.sr_advance_(cblk)
    assert torch.equal(bits16(sr_p[0]), bits16(cpu_p[0]))


# ---------------------------------------------------------------- the engine
def _engine(name="adam", sr=3, **kw):
    return TS.sr_engine(name, "cuda", sr=sr, **kw)


def _data():
    g = torch.Generator().manual_seed(11)
    return torch.randn(8, 64, generator=g).cuda().to(BF), torch.randn(8, 10, generator=g).cuda()


def _loss(d, x, y):
    return torch.nn.functional.mse_loss(d(x).float(), y)


def test_engine_reproducible_and_seeded(gpu_ext):
    a, b, c, rn = _engine(sr=3), _engine(sr=3), _engine(sr=4), _engine(sr=None)
    for d in (a, b, c, rn):
        TS.run_steps(d, 3)
    torch.cuda.synchronize()
    assert LS.same(LS.state(a), LS.state(b))
    assert not LS.same(LS.state(a), LS.state(c)) and not LS.same(LS.state(a), LS.state(rn))
    assert int(a.sr_step()) == 3 and a.sr_step().is_cuda and a.sr_step().dim() == 0


def test_graphed_step_equals_eager(gpu_ext):
    from fluxmpi_amd.parallel.graph import GraphedStep
    d1, d2 = _engine(), _engine()
    x, y = _data()
    loss_fn = lambda d, xx, yy: _loss(d, xx, yy)  # noqa: E731
    g = GraphedStep(d1, loss_fn, x, y, warmup=2)
    for _ in range(2):
        loss_fn(d2, x, y).backward()
        d2.step()
    for i in range(3):
        g(x, y)
        loss_fn(d2, x, y).backward()
        d2.step()
        torch.cuda.synchronize()
        assert LS.same(LS.state(d1), LS.state(d2)), i
        assert int(d1.sr_step()) == int(d2.sr_step()) == 3 + i
    rn = _engine(sr=None)
    for _ in range(5):
        loss_fn(rn, x, y).backward()
        rn.step()
    assert not LS.same(LS.state(d1), LS.state(rn))


def test_overlap_opt_equals_step(gpu_ext):
    a, b = _engine(overlap_opt=False), _engine(overlap_opt=True)
    assert b.overlap_opt and b._opt_stream is not None and not a.overlap_opt
    x, y = _data()
    for _ in range(3):
        for d in (a, b):
            _loss(d, x, y).backward()
            d.step()
    torch.cuda.synchronize()
    assert LS.same(LS.state(a), LS.state(b)) and int(b.sr_step()) == 3


def test_flat_route_equals_per_leaf_route(gpu_ext):
    """clip_global_norm with a norm so large that the scale is exactly 1: per-leaf slices at their bucket
    offsets against the packed flat bucket (view mode: one launch per bucket)."""
    a = _engine(grad_mode="view")
    b = _engine(clip_global_norm=1e30)
    c = _engine()
    x, y = _data()
    for _ in range(3):
        for d in (a, b, c):
            _loss(d, x, y).backward()
            d.step()
    torch.cuda.synchronize()
    assert LS.same(LS.state(a), LS.state(c)) and LS.same(LS.state(b), LS.state(c))


def test_loss_scale_skip_keeps_every_bit(gpu_ext):
    from fluxmpi_amd import LossScale
    d = _engine(loss_scale=LossScale(init=1024.0, interval=1000))
    TS.run_steps(d, 1, mult=1024.0)
    before, blk = LS.state(d), d._sr_block.clone()
    grads = LS.step_grads(d, 1, 1024.0)
    grads[-2].view(-1)[3] = float("inf")
    LS.give(d, grads)
    d.step()
    assert LS.same(before, LS.state(d)) and torch.equal(blk, d._sr_block) and int(d.sr_step()) == 1
    assert int(d.step_skipped()) == 1
    TS.run_steps(d, 1, first=2, mult=512.0)
    assert int(d.sr_step()) == 2 and not LS.same(before, LS.state(d))


def test_option_off_is_the_parent_path(gpu_ext):
    """stochastic_rounding=None: nothing allocated, and the bits of the existing round-to-nearest kernel
    driven by hand over the same slices."""
    d = _engine(sr=None)
    assert d._sr_block is None and d._sr_seed is None
    flat = [b.flat_param.clone() for b in d.buckets]
    m = [torch.zeros_like(f) for f in flat]
    v = [torch.zeros_like(f) for f in flat]
    r = d.adam
    hyper = torch.tensor([r.eta, r.beta[0], r.beta[1]], dtype=torch.float32, device="cuda")
    for t in range(2):
        grads = LS.step_grads(d, t)
        LS.give(d, grads)
        d.step()
        by_param = {id(p): g for p, g in zip(d.module.parameters(), grads)}
        for k, b in enumerate(d.buckets):
            sl = lambda f: [f[o:o + p.numel()] for p, o in zip(b.params, b.offsets)]  # noqa: E731
            fused.adam_(sl(flat[k]), [by_param[id(p)].reshape(-1) for p in b.params], sl(m[k]), sl(v[k]), lr=r.eta,
                        beta1=r.beta[0], beta2=r.beta[1], eps=r.epsilon, bc1=0.0, bc2=0.0, dev_hyper=hyper)
        fused.adam_advance_(hyper, r.beta[0], r.beta[1])
    torch.cuda.synchronize()
    for k, b in enumerate(d.buckets):
        assert torch.equal(b.flat_param, flat[k]) and torch.equal(b.exp_avg, m[k]) and torch.equal(b.exp_avg_sq, v[k])
