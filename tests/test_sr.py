"""Stochastic rounding on the CPU (``ops.philox``, the reference path of ``ops.optim``'s ``sr=`` and of
``DDP(master_weights=False, stochastic_rounding=...)``): the generator's known answers, the rounding's
properties, unbiasedness, independence from how an element is reached, the engine on two gloo ranks,
checkpoints and errors. The helpers are shared with ``test_sr_gpu.py``."""
import math

import numpy as np
import pytest
import torch

from fluxmpi_amd.ops import optim as fused
from fluxmpi_amd.ops import philox
from tests import loss_scale_cases as LS

BF = torch.bfloat16


# ---------------------------------------------------------------- shared helpers
def bits16(t):
    """bf16 tensor -> its bit patterns as int64 (CPU)."""
    return t.detach().cpu().contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def from_bits32(u):
    return torch.tensor(np.asarray(u, dtype=np.uint32).view(np.int32)).view(torch.float32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits16(a) if a.dtype == BF else a.cpu(),
                                                                     bits16(b) if b.dtype == BF else b.cpu())


def assert_bits(got, want, what=None):
    """Equal bf16 bits; where the expected value is a NaN any NaN will do (which NaN the round-to-nearest
    cast of a NaN yields is the platform's)."""
    g, w = bits16(got), bits16(want)
    nan = torch.isnan(want.detach().cpu()) & torch.isnan(got.detach().cpu())
    assert got.shape == want.shape and bool(((g == w) | nan).all()), what


def sr_engine(name, dev, seed=0, sr=True, **kw):
    """The 64-128-10 bf16 MLP without masters, several buckets."""
    return LS.engine(name, dev, BF, seed=seed, master_weights=False, stochastic_rounding=sr, **kw)


def run_steps(d, steps, first=0, mult=1.0):
    for t in range(first, first + steps):
        LS.give(d, LS.step_grads(d, t, mult))
        d.step()


# ---------------------------------------------------------------- the generator
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
          "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    got = philox.philox4x32(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert " ".join(f"{int(w):08x}" for w in got) == want


def test_philox_vectorised_equals_one_by_one():
    ctr = np.array([c for c, _, _ in KNOWN], dtype=np.uint64)
    key = np.array([k for _, k, _ in KNOWN], dtype=np.uint64)
    got = philox.philox4x32(ctr, key)
    for i, (_, _, want) in enumerate(KNOWN):
        assert " ".join(f"{int(w):08x}" for w in got[i]) == want


def test_random_bits_layout():
    """r_j = (w[j >> 1] >> (16 * (j & 1))) & 0xffff of the call with counter (q lo, q hi, stream * 4 + slot,
    step) and key (seed lo, seed hi), also for q beyond 2^32."""
    seed, stream, slot, step = (0x299F31D0 << 32) | 0xA4093822, 5, 2, 77
    for e0 in (0, 8 * 123, (1 << 35) + 16):
        r = philox.random_bits(8, seed, stream, slot, step, e0)
        q = e0 >> 3
        w = philox.philox4x32(np.array([q & 0xFFFFFFFF, q >> 32, stream * 4 + slot, step], dtype=np.uint64),
                              np.array([0xA4093822, 0x299F31D0], dtype=np.uint64))
        assert [int(x) for x in r] == [(int(w[j >> 1]) >> (16 * (j & 1))) & 0xFFFF for j in range(8)]


# ---------------------------------------------------------------- the rounding
def test_representable_unchanged_for_every_r():
    x = torch.tensor([1.0, -1.0, 0.0, -0.0, 3.140625, -2.0 ** -126, 2.0 ** -133, 3.3895313892515355e38,
                      float("inf"), -float("inf")])
    assert torch.equal(x.to(BF).float(), x)  # all of them are bf16 values
    for r in (0, 1, 0x7FFF, 0x8000, 0xFFFF):
        assert torch.equal(bits16(philox.sr_round(x, r)), bits16(x.to(BF))), r
    allr = philox.sr_round(torch.full((65536,), 1.5), np.arange(65536))
    assert bool((allr.float() == 1.5).all())


def test_zero_subnormal_inf_nan():
    assert bits16(philox.sr_round(torch.tensor([0.0, -0.0]), 0xFFFF)).tolist() == [0x0000, 0x8000]
    # an fp32 subnormal between 0 and the least bf16 subnormal (bits 0x00010000): down to 0 or up to it
    sub = from_bits32([0x00004000, 0x80004000])
    assert bits16(philox.sr_round(sub, 0xBFFF)).tolist() == [0x0000, 0x8000]
    assert bits16(philox.sr_round(sub, 0xC000)).tolist() == [0x0001, 0x8001]
    # inf and NaN: the round-to-nearest cast, whatever r; a NaN never becomes anything else
    special = from_bits32([0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7F80FFFF])
    for r in (0, 0x8000, 0xFFFF):
        got = philox.sr_round(special, r)
        assert bits16(got[:2]).tolist() == [0x7F80, 0xFF80]
        assert torch.isnan(got[2:]).all() and torch.equal(torch.signbit(got), torch.signbit(special))
        assert_bits(got, special.to(BF))
    # a finite value above the largest bf16 may carry into inf: correct stochastic rounding
    big = from_bits32([0x7F7FFFFF, 0xFF7FFFFF])
    assert bits16(philox.sr_round(big, 0)).tolist() == [0x7F7F, 0xFF7F]
    assert bits16(philox.sr_round(big, 1)).tolist() == [0x7F80, 0xFF80]


def test_sign_kept_and_result_is_a_neighbour():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1 << 14, generator=g) * torch.tensor(2.0).pow(torch.randint(-40, 40, (1 << 14,), generator=g))
    got = philox.sr_reference(x, seed=11, stream=2, slot=1, step=9, offset=40)
    u = bits32(x)
    down, up = u >> 16, (u >> 16) + 1  # the two bf16 neighbours by magnitude (the sign bit rides along)
    b = bits16(got)
    exact = (u & 0xFFFF) == 0
    assert bool(((b == down) | ((b == up) & ~exact)).all())
    assert torch.equal(torch.signbit(got), torch.signbit(x))
    assert bool((got.float().abs() >= x.abs()).logical_or(b == down).all())
    assert bool((b == up).any()) and bool((b == down).any())


def test_probability_is_the_discarded_fraction():
    """Over all 65536 values of r exactly (u & 0xffff) of them round away from zero."""
    for low in (0x0001, 0x4000, 0xFFFF):
        x = from_bits32([0x3F800000 | low]).expand(65536).contiguous()
        b = bits16(philox.sr_round(x, np.arange(65536)))
        assert int((b == 0x3F81).sum()) == low and int((b == 0x3F80).sum()) == 65536 - low


def test_unbiased():
    """x = 1 + 2^-7 / 4, n = 2^20: |fraction rounded up - 1/4| <= 6 sqrt(1/4 * 3/4 / n) = 2.6e-3."""
    n = 1 << 20
    x = torch.full((n,), 1.0 + 2.0 ** -7 / 4)
    got = philox.sr_reference(x, seed=0, stream=0, slot=0, step=0)
    up = float((got.float() > 1.0).double().mean())
    bound = 6 * math.sqrt(0.25 * 0.75 / n)
    print(f"fraction rounded up {up:.6f} (bound {bound:.2e} around 0.25)")
    assert bound < 2.6e-3 and abs(up - 0.25) <= bound
    assert set(bits16(got).unique().tolist()) == {0x3F80, 0x3F81}


# ---------------------------------------------------------------- independence from the path
def test_same_element_same_bits_however_reached():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(100, generator=g)
    whole = philox.sr_reference(x, 7, stream=3, slot=1, step=2, offset=16)
    for cut in (1, 3, 8, 50, 99):
        parts = torch.cat([philox.sr_reference(x[:cut], 7, 3, 1, 2, 16), philox.sr_reference(x[cut:], 7, 3, 1, 2, 16 + cut)])
        assert torch.equal(bits16(whole), bits16(parts)), cut
    one = torch.cat([philox.sr_reference(x[i:i + 1], 7, 3, 1, 2, 16 + i) for i in range(100)])
    assert torch.equal(bits16(whole), bits16(one))


def test_slot_stream_step_seed_give_other_words():
    base = dict(seed=1, stream=0, slot=0, step=0)
    r0 = philox.random_bits(64, **base)
    for k, v in (("slot", 1), ("stream", 1), ("step", 1), ("seed", 2), ("seed", 1 + (1 << 32))):
        assert not np.array_equal(r0, philox.random_bits(64, **{**base, k: v})), k
    # stream * 4 + slot: no (stream, slot) pair shares its counter word with another
    assert len({philox.random_bits(8, 1, s, k, 0).tobytes() for s in range(3) for k in range(4)}) == 12
    for bad in (dict(stream=1 << 30), dict(slot=4), dict(step=1 << 32), dict(seed=1 << 64), dict(seed=-1)):
        with pytest.raises(ValueError):
            philox.random_bits(8, **{**base, **bad})


# ---------------------------------------------------------------- the functional API on CPU leaves
def leaves(sizes, seed=0, sdt=BF, states=2):
    g = torch.Generator().manual_seed(seed)
    p = [torch.randn(n, generator=g).to(BF) for n in sizes]
    gr = [(torch.randn(n, generator=g) * 0.1).to(BF) for n in sizes]
    st = [[(torch.randn(n, generator=g).abs() * 0.01).to(sdt) for n in sizes] for _ in range(states)]
    return p, gr, st


ADAM = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, bc1=0.1, bc2=0.001)


def test_adam_reference_is_sr_of_the_unrounded_update():
    """The bf16 outputs under sr are sr_reference of what an fp32 copy of the leaves computes."""
    sizes, off = [9, 40], [0, 16]
    p, g, (m, v) = leaves(sizes)
    pf, mf, vf = [[t.float() for t in l] for l in (p, m, v)]
    fused.adam_reference_(pf, g, mf, vf, **ADAM)
    sr = fused.SR(5, stream=2, step=3, offsets=off)
    fused.adam_(p, g, m, v, **ADAM, sr=sr)
    for i in range(2):
        for got, pre, slot in ((p[i], pf[i], 0), (m[i], mf[i], 1), (v[i], vf[i], 2)):
            assert torch.equal(bits16(got), bits16(philox.sr_reference(pre, 5, 2, slot, 3, off[i])))
    # fp32 states are stored as they are; the parameter still rounds stochastically
    p2, g2, (m2, v2) = leaves(sizes, sdt=torch.float32)
    pf2 = [t.float() for t in p2]
    m3, v3 = [t.clone() for t in m2], [t.clone() for t in v2]
    fused.adam_reference_(pf2, g2, m3, v3, **ADAM)
    fused.adam_(p2, g2, m2, v2, **ADAM, sr=sr)
    assert all(torch.equal(a, b) for a, b in zip(m2 + v2, m3 + v3))
    assert all(torch.equal(bits16(p2[i]), bits16(philox.sr_reference(pf2[i], 5, 2, 0, 3, off[i]))) for i in range(2))


def test_block_step_and_advance():
    blk = fused.sr_block("cpu", step=6)
    p, g, (m, v) = leaves([33])
    q, h, (n, w) = leaves([33])
    fused.adam_(p, g, m, v, **ADAM, sr=fused.SR(1, dev_block=blk, step=999))  # the block wins
    fused.adam_(q, h, n, w, **ADAM, sr=fused.SR(1, step=6))
    assert torch.equal(bits16(p[0]), bits16(q[0])) and torch.equal(bits16(m[0]), bits16(n[0]))
    flag = torch.ones(1, dtype=torch.int32)
    fused.sr_advance_(blk, dev_skip=flag)
    assert int(blk[0]) == 6
    fused.sr_advance_(blk)
    assert int(blk[0]) == 7 and blk[1:].eq(0).all()
    top = fused.sr_block("cpu", step=(1 << 32) - 1)
    assert int(top[0]) & 0xFFFFFFFF == (1 << 32) - 1
    fused.sr_advance_(top)
    assert int(top[0]) == 0  # a uint32 wraps


def test_stochastic_round_cpu_and_skip():
    x = [torch.randn(n, generator=torch.Generator().manual_seed(n)) for n in (5, 17)]
    d = [torch.full((n,), float("nan"), dtype=BF) for n in (5, 17)]
    sr = fused.SR(9, stream=1, step=4, offsets=[3, 8])
    fused.stochastic_round_(d, x, sr, dev_skip=torch.ones(1, dtype=torch.int32))
    assert all(torch.isnan(t).all() for t in d)
    fused.stochastic_round_(d, x, sr)
    assert all(torch.equal(bits16(d[i]), bits16(philox.sr_reference(x[i], 9, 1, 0, 4, (3, 8)[i]))) for i in range(2))


def test_functional_errors():
    p, g, (m, v) = leaves([8])
    sr = fused.SR(0)
    with pytest.raises(ValueError):
        fused.adam_(p, g, m, v, **ADAM, masters=[p[0].float()], sr=sr)
    h = [t.half() for t in p]
    with pytest.raises(TypeError):
        fused.adam_(h, [t.half() for t in g], [t.half() for t in m], [t.half() for t in v], **ADAM, sr=sr)
    with pytest.raises(TypeError):
        fused.sgd_([t.float() for t in p], g, [], lr=0.1, sr=sr)
    with pytest.raises(TypeError):
        fused.rule_("lion", h, [t.half() for t in g], [[t.half() for t in m]], lr=0.1, beta1=0.9, beta2=0.99, sr=sr)
    with pytest.raises(ValueError):
        fused.adam_(p, g, m, v, **ADAM, sr=fused.SR(0, offsets=[0, 8]))
    with pytest.raises(TypeError):
        fused.stochastic_round_([p[0].half()], [p[0].float()], sr)
    for bad in (dict(seed=-1), dict(seed=0, stream=1 << 30), dict(seed=0, step=1 << 32), dict(seed=0, offsets=[-8])):
        with pytest.raises(ValueError):
            fused.SR(**bad)


# ---------------------------------------------------------------- the engine on CPU leaves
def test_engine_moves_and_is_reproducible():
    a, b, c, rn = sr_engine("adam", "cpu", sr=3), sr_engine("adam", "cpu", sr=3), sr_engine("adam", "cpu", sr=4), \
        sr_engine("adam", "cpu", sr=None)
    assert rn._sr_block is None
    for d in (a, b, c, rn):
        run_steps(d, 3)
    assert LS.same(LS.state(a), LS.state(b))
    assert not LS.same(LS.state(a), LS.state(c)) and not LS.same(LS.state(a), LS.state(rn))
    assert int(a.sr_step()) == 3 and a.sr_step().dim() == 0 and a.sr_step().dtype == torch.int32
    with pytest.raises(RuntimeError):
        rn.sr_step()
    assert all(b_.exp_avg.dtype == BF and b_.master is None for b_ in a.buckets)


def test_engine_true_is_seed_zero():
    a, b = sr_engine("momentum", "cpu", sr=True), sr_engine("momentum", "cpu", sr=0)
    for d in (a, b):
        run_steps(d, 2)
    assert LS.same(LS.state(a), LS.state(b))


def test_engine_flat_route_equals_per_leaf_route():
    """clip_global_norm with a norm so large that the scale is exactly 1: the update runs leaf by leaf
    on slices of the bucket at their offsets, and draws the bits of the one flat launch."""
    a, b = sr_engine("adam", "cpu", sr=1), sr_engine("adam", "cpu", sr=1, clip_global_norm=1e30)
    for d in (a, b):
        run_steps(d, 3)
    assert LS.same(LS.state(a), LS.state(b))


def test_engine_loss_scale_skip_keeps_every_bit():
    from fluxmpi_amd import LossScale
    d = sr_engine("adam", "cpu", sr=2, loss_scale=LossScale(init=1024.0, interval=1000))
    run_steps(d, 1, mult=1024.0)
    before, blk = LS.state(d), d._sr_block.clone()
    grads = LS.step_grads(d, 1, 1024.0)
    grads[-2].view(-1)[3] = float("inf")
    LS.give(d, grads)
    d.step()
    assert LS.same(before, LS.state(d)) and torch.equal(blk, d._sr_block) and int(d.sr_step()) == 1
    run_steps(d, 1, first=2, mult=512.0)
    assert int(d.sr_step()) == 2 and not LS.same(before, LS.state(d))


@pytest.mark.parametrize("name", ["adam", "momentum"])
def test_state_dict_round_trip(name):
    """Two steps, save, load into a fresh engine, two steps == four uninterrupted steps."""
    whole, first = sr_engine(name, "cpu", sr=6), sr_engine(name, "cpu", sr=6)
    run_steps(whole, 4)
    run_steps(first, 2)
    sd = first.state_dict()
    assert sd["sr"] == {"seed": 6, "step": 2}
    second = sr_engine(name, "cpu", seed=9, sr=6)
    second.load_state_dict(sd)
    assert int(second.sr_step()) == 2
    run_steps(second, 2, first=2)
    assert LS.same(LS.state(whole), LS.state(second))
    # a checkpoint without the key starts at step 0
    del sd["sr"]
    second.load_state_dict(sd)
    assert int(second.sr_step()) == 0
    assert "sr" not in sr_engine(name, "cpu", sr=None).state_dict()


def test_engine_errors():
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP
    with pytest.raises(ValueError):
        DDP(LS.mlp(0, "cpu", BF), O.Adam(), master_weights=True, stochastic_rounding=True)
    with pytest.raises(ValueError):
        DDP(LS.mlp(0, "cpu", BF), O.Adam(), stochastic_rounding=1)  # master_weights defaults to True
    for rule in (O.LARS(0.1), O.LAMB(1e-2)):
        with pytest.raises(ValueError):
            DDP(LS.mlp(0, "cpu", BF), rule, master_weights=False, stochastic_rounding=True)
    with pytest.raises(TypeError):
        DDP(LS.mlp(0, "cpu", torch.float16), O.Adam(), master_weights=False, stochastic_rounding=True)
    # fp32 buckets are untouched: the bits of the engine without the option
    a = DDP(LS.mlp(0, "cpu"), O.Adam(1e-2), master_weights=False, stochastic_rounding=True, **LS.SMALL)
    b = DDP(LS.mlp(0, "cpu"), O.Adam(1e-2), master_weights=False, **LS.SMALL)
    for d in (a, b):
        run_steps(d, 2)
    assert LS.same(LS.state(a), LS.state(b)) and int(a.sr_step()) == 2


# ---------------------------------------------------------------- two ranks over gloo
def worker_two_ranks():
    """Each rank its own data; after 3 steps parameters and moments have equal bits on both ranks. On
    step 2 only rank 1's LOCAL gradient holds an inf: both ranks skip, bits and sr_step() unchanged."""
    import fluxmpi_amd as FluxMPI
    from fluxmpi_amd import optimisers as O
    from fluxmpi_amd.parallel.ddp import DDP

    FluxMPI.Init()
    W, r = FluxMPI.total_workers(), FluxMPI.local_rank()
    assert W == 2
    d = DDP(LS.mlp(r, "cpu", BF), O.Adam(1e-2), master_weights=False, stochastic_rounding=17, loss_scale="dynamic",
            overlap=False, **LS.SMALL)  # seeds of the models differ: the root's weights are broadcast
    assert d.communicate and len(d.buckets) > 1

    def agree(t):
        """Bit-identical on both ranks: with two ranks a + b == 2 a means b == a."""
        s = FluxMPI.allreduce_gradients({"x": t.detach().clone().double()}, on_gpu=False)["x"]
        return torch.equal(s, t.detach().double() * 2)

    x = torch.randn(W, 8, 64, generator=torch.Generator().manual_seed(5))[r].to(BF)
    start = LS.state(d)
    for step in (1, 2, 3, 4):
        d.scale_loss(d(x).float().pow(2).mean()).backward()
        if step == 2 and r == 1:
            next(d.module.parameters()).grad.view(-1)[0] = float("inf")
        before, cnt = LS.state(d), int(d.sr_step())
        d.step()
        assert LS.same(before, LS.state(d)) == (step == 2), step
        assert int(d.sr_step()) == cnt + (0 if step == 2 else 1)
    assert int(d.sr_step()) == 3 and int(d.skipped_steps()) == 1 and not LS.same(start, LS.state(d))
    assert agree(d.sr_step().reshape(1))
    for b in d.buckets:
        assert b.exp_avg.dtype == BF
        assert agree(b.flat_param) and agree(b.exp_avg) and agree(b.exp_avg_sq)
    FluxMPI.Finalize()


def test_two_ranks_keep_equal_bits(spmd):
    spmd("tests.test_sr:worker_two_ranks", nprocs=2)
