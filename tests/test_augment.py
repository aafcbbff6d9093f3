"""The device input pipeline's host side (``ops/augment.py``): the generator's word order, the draws, the
CPU reference against an independent composition, the mixing draw, the soft targets, the public class
and every argument check. No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fluxmpi_amd as FluxMPI
from fluxmpi_amd.ops import augment as A
from fluxmpi_amd.ops.philox import philox4x32

B, H, W, PAD, SIZE = 5, 37, 41, 4, (32, 36)


@pytest.fixture(scope="module")
def img():
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)


def bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------- generator and draws
def test_philox_known_answer():
    got = philox4x32(np.zeros(4), np.zeros(2))
    assert [f"{int(v):08x}" for v in got] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]


def test_sample_draws_word_order():
    ox, oy, flip = A.sample_draws(5, 0, 0, 0, 0, 14, 14)
    assert ox.tolist() == [5, 13, 0, 11, 13]
    assert oy.tolist() == [12, 5, 4, 5, 9]
    assert flip.tolist() == [0, 1, 1, 1, 0]


def test_sample_draws_ranges_and_coverage():
    ox, oy, flip = A.sample_draws(4096, 0, 0, 0, 0, 33, 33)
    for o in (ox, oy):
        assert o.min() == 0 and o.max() == 32
        counts = np.bincount(o, minlength=33)
        # every offset occurs: 124 expected per bin, +- 4 sigma = 44 (the bins count 101 .. 143)
        assert counts.min() >= 80 and counts.max() <= 168
    assert set(flip.tolist()) == {0, 1} and 0.46 < flip.mean() < 0.54  # 4 sigma = 0.031 (0.492 here)
    ox1, oy1, _ = A.sample_draws(64, 7, 3, 9, 1 << 40, 1, 1)  # range 1: offset 0
    assert not ox1.any() and not oy1.any()
    big = A.sample_draws(256, 1, 0, 0, 0, (1 << 32) - 1, 3)
    assert big[0].max() < (1 << 32) - 1 and big[1].max() <= 2
    # the draws depend on (seed, stream, step, sample) alone
    a = A.sample_draws(8, 5, 1, 2, 16, 14, 14)
    b = A.sample_draws(24, 5, 1, 2, 0, 14, 14)
    assert all(np.array_equal(x, y[16:]) for x, y in zip(a, b))
    for other in ((6, 1, 2), (5, 2, 2), (5, 1, 3)):
        c = A.sample_draws(24, *other, 0, 14, 14)
        assert not all(np.array_equal(x, y) for x, y in zip(b, c))


# ---------------------------------------------------------------- the reference
def _composed(img, size, pad, fill, flip, mean, std, seed=0, stream=0, step=0):
    """torchvision's order in plain torch: pad the bytes, crop at the drawn offsets, flip, normalise."""
    h, w = size
    n, hh, ww, _ = img.shape
    ox, oy, fl = A.sample_draws(n, seed, stream, step, 0, ww + 2 * pad - w + 1, hh + 2 * pad - h + 1)
    x = F.pad(img.permute(0, 3, 1, 2), (pad, pad, pad, pad), value=fill)
    out = []
    for b in range(n):
        c = x[b, :, oy[b]:oy[b] + h, ox[b]:ox[b] + w]
        if flip and fl[b]:
            c = c.flip(-1)
        out.append(c)
    y = torch.stack(out).float() / 255.0
    m = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    return (y - m) / s, torch.stack(out)


@pytest.mark.parametrize("fill", [0, 255])
@pytest.mark.parametrize("flip", [True, False])
def test_reference_matches_composition(img, fill, flip):
    """The two formulas differ ((u / 255 - mean) / std against u * a + b), so this comparison alone has a
    tolerance: 2 fp32 ulp at the larger of the two terms u * a and b whose sum the value is (near
    u / 255 = mean the sum cancels, and an ulp of the result itself would measure nothing). Each
    formula rounds three times at that magnitude or below."""
    kw = dict(size=SIZE, pad=PAD, fill=fill, flip=flip, mean=A.IMAGENET_MEAN, std=A.IMAGENET_STD)
    want, cropped = _composed(img, **kw)
    got = A.augment_reference(img, dtype=torch.float32, **kw)
    assert got.dtype == torch.float32 and got.shape == want.shape
    a, b = A.norm_constants(A.IMAGENET_MEAN, A.IMAGENET_STD)
    mag = np.maximum(np.abs(cropped.numpy().astype(np.float32) * a.reshape(1, 3, 1, 1)), np.abs(b).reshape(1, 3, 1, 1))
    tol = 2.0 * np.spacing(mag.astype(np.float32))
    err = (got.double() - want.double()).abs().numpy()
    print("max error / tolerance:", float((err / tol).max()))
    assert (err <= tol).all(), float((err / tol).max())
    if fill == 255:
        assert (cropped == 255).any()
    # the casts are the round-to-nearest casts of those values
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(bits(A.augment_reference(img, dtype=dt, **kw)), bits(got.to(dt)))


def test_identity_case_is_exact(img):
    a, b = A.norm_constants((0.5, 0.25, 0.125), (0.25, 0.5, 1.5))
    got = A.augment_reference(img, size=(H, W), flip=False, mean=(0.5, 0.25, 0.125), std=(0.25, 0.5, 1.5),
                              dtype=torch.float32, step=5)
    prod = img.numpy().astype(np.float32) * a
    assert prod.dtype == np.float32
    want = torch.from_numpy(prod + b).permute(0, 3, 1, 2)
    assert torch.equal(got, want)
    assert a.dtype == np.float32 and a[0] == np.float32(1.0 / (255.0 * 0.25)) and b[2] == np.float32(-0.125 / 1.5)


def test_separately_rounded_constants_differ_from_fma():
    """What the kernel must not do: a fused multiply-add changes the fp32 bits of 389 of the 768 (byte,
    channel) pairs with the ImageNet constants."""
    a, b = A.norm_constants(A.IMAGENET_MEAN, A.IMAGENET_STD)
    u = np.arange(256, dtype=np.float32)[:, None]
    two = (u * a[None, :]) + b[None, :]
    fused = (u.astype(np.float64) * a[None, :].astype(np.float64) + b[None, :].astype(np.float64)).astype(np.float32)
    assert two.dtype == np.float32 and int((two != fused).sum()) == 389


def test_center_crop_draws_nothing(img):
    kw = dict(size=SIZE, pad=PAD, crop="center", dtype=torch.float32)
    x0 = A.augment_reference(img, step=0, **kw)
    x1 = A.augment_reference(img, step=77, seed=9, stream=4, sample_offset=100, **kw)
    assert torch.equal(x0, x1)
    oy, ox = (H + 2 * PAD - SIZE[0]) // 2 - PAD, (W + 2 * PAD - SIZE[1]) // 2 - PAD
    a, b = A.norm_constants(A.IMAGENET_MEAN, A.IMAGENET_STD)
    want = img[:, oy:oy + SIZE[0], ox:ox + SIZE[1]].numpy().astype(np.float32) * a + b
    assert torch.equal(x0.permute(0, 2, 3, 1), torch.from_numpy(want))


def test_channels_layout_and_zero_channel(img):
    x3 = A.augment_batch(img, size=SIZE, pad=PAD, channels=3)
    x4 = A.augment_batch(img, size=SIZE, pad=PAD, channels=4)
    assert tuple(x4.shape) == (B, 4, *SIZE) and x4.permute(0, 2, 3, 1).is_contiguous()
    assert x4.is_contiguous(memory_format=torch.channels_last) and x4.dtype == torch.bfloat16
    assert torch.equal(bits(x4[:, :3]), bits(x3)) and not bits(x4[:, 3]).any()


def test_mix_semantics(img):
    kw = dict(size=SIZE, pad=PAD, dtype=torch.float32, step=2)
    y = A.augment_reference(img, **kw)
    yp = y.flip(0)
    lam = 0.3
    mixed = A.augment_reference(img, mix=A.MixDraw(1, lam), **kw)
    assert torch.equal(mixed, yp + torch.tensor(lam, dtype=torch.float32) * (y - yp))
    assert torch.equal(mixed[2], y[2])  # odd B: the middle sample partners itself
    assert torch.equal(A.augment_reference(img, mix=A.MixDraw(1, 0.0), **kw), yp + 0.0 * (y - yp))
    box = (5, 7, 20, 30)
    cut = A.augment_reference(img, mix=A.MixDraw(2, 0.5, box), **kw)
    want = y.clone()
    want[:, :, 5:20, 7:30] = yp[:, :, 5:20, 7:30]
    assert torch.equal(cut, want)
    assert torch.equal(A.augment_reference(img, mix=A.MixDraw(2, 1.0, (4, 4, 4, 9)), **kw), y)
    assert torch.equal(A.augment_reference(img, mix=A.MixDraw(2, 0.0, (0, 0, *SIZE)), **kw), yp)


def test_sample_offset_follows_the_shard():
    g = torch.Generator().manual_seed(1)
    data = torch.randint(0, 256, (2 * B, H, W, 3), dtype=torch.uint8, generator=g)
    whole = A.augment_batch(data, size=SIZE, pad=PAD, seed=3, step=4)
    draws = A.sample_draws(2 * B, 3, 0, 4, 0, 14, 14)
    for rank in (0, 1):
        shard = FluxMPI.DistributedDataContainer(data, rank=rank, world=2)
        batch = shard[0:B]
        assert torch.equal(batch, data[rank * B:(rank + 1) * B])
        mine = A.sample_draws(B, 3, 0, 4, rank * B, 14, 14)
        assert all(np.array_equal(m, d[rank * B:(rank + 1) * B]) for m, d in zip(mine, draws))
        x = A.augment_batch(batch, size=SIZE, pad=PAD, seed=3, step=4, sample_offset=rank * B)
        assert torch.equal(bits(x), bits(whole[rank * B:(rank + 1) * B]))
    assert not np.array_equal(draws[0][:B], draws[0][B:])


# ---------------------------------------------------------------- mixing draw and targets
def test_mix_targets():
    labels = torch.tensor([1, 0, 3, 2, 3])
    t = A.mix_targets(labels, 4, 0.3, label_smoothing=0.1)
    assert t.dtype == torch.float32 and tuple(t.shape) == (5, 4)
    assert torch.allclose(t.sum(1), torch.ones(5), atol=1e-6)
    s = F.one_hot(labels, 4).float() * 0.9 + 0.1 / 4
    assert torch.allclose(A.mix_targets(labels, 4, 1.0, label_smoothing=0.1), s, atol=1e-7)
    assert torch.allclose(t[2], s[2], atol=1e-7)  # odd B: the middle row is S(y)
    assert torch.allclose(t, 0.3 * s + 0.7 * s.flip(0), atol=1e-6)
    assert torch.equal(A.mix_targets(labels, 4, 1.0), F.one_hot(labels, 4).float())
    # a 0-dim tensor lam gives the bits of the float
    assert torch.equal(A.mix_targets(labels, 4, torch.tensor(0.3), 0.1), t)
    with pytest.raises(TypeError, match="mix_targets"):
        A.mix_targets(labels.float(), 4, 0.5)
    with pytest.raises(ValueError, match="mix_targets"):
        A.mix_targets(labels, 4, 0.5, label_smoothing=1.0)


def test_draw_mix_rules():
    size = (32, 36)
    modes = set()
    for step in range(64):
        d = A.draw_mix(3, 0, step, size, mixup_alpha=0.4, cutmix_alpha=1.0)
        assert d == A.draw_mix(3, 0, step, size, mixup_alpha=0.4, cutmix_alpha=1.0)
        modes.add(d.mode)
        assert 0.0 <= d.lam <= 1.0
        if d.mode == 2:
            y0, x0, y1, x1 = d.box
            assert 0 <= y0 <= y1 <= 32 and 0 <= x0 <= x1 <= 36
            assert d.lam == 1.0 - ((y1 - y0) * (x1 - x0)) / (32 * 36)
    assert modes == {1, 2}
    # consecutive steps and streams own their numbers
    seq = [A.draw_mix(3, 0, s, size, mixup_alpha=0.4).lam for s in range(16)]
    assert len(set(seq)) == 16
    assert A.draw_mix(3, 1, 0, size, mixup_alpha=0.4).lam != seq[0]
    assert A.draw_mix(4, 0, 0, size, mixup_alpha=0.4).lam != seq[0]
    assert A.draw_mix(3, 0, 0, size) == A.MixDraw(0, 1.0, (0, 0, 0, 0))
    assert A.draw_mix(3, 0, 0, size, mixup_alpha=0.4, prob=0.0).mode == 0
    assert all(A.draw_mix(3, 0, s, size, cutmix_alpha=1.0).mode == 2 for s in range(8))
    assert all(A.draw_mix(3, 0, s, size, mixup_alpha=1.0, cutmix_alpha=1.0, switch_prob=0.0).mode == 1
               for s in range(8))
    mean = np.mean([A.draw_mix(3, 0, s, size, mixup_alpha=1.0).lam for s in range(400)])
    assert 0.44 < mean < 0.56  # Beta(1, 1) is uniform


def test_draw_mix_edge_lambdas():
    """lambda = 1: the box has no side and is empty wherever its centre falls. lambda = 0: the box has
    the image's sides around a uniform centre and is clipped, so it is the full image when the centre is
    the image's (timm's rule); the steps are walked until that centre arises."""
    size = (4, 4)
    full = 0
    for step in range(256):
        e = A.draw_mix(1, 0, step, size, cutmix_alpha=1.0, lam=1.0)
        y0, x0, y1, x1 = e.box
        assert e.mode == 2 and (y1 - y0) * (x1 - x0) == 0 and e.lam == 1.0
        f = A.draw_mix(1, 0, step, size, cutmix_alpha=1.0, lam=0.0)
        y0, x0, y1, x1 = f.box
        assert 0 <= y0 <= y1 <= 4 and 0 <= x0 <= x1 <= 4
        assert f.lam == 1.0 - ((y1 - y0) * (x1 - x0)) / 16
        if f.box == (0, 0, 4, 4):
            full += 1
            assert f.lam == 0.0
    assert full > 0
    with pytest.raises(ValueError, match="draw_mix"):
        A.draw_mix(1, 0, 0, size, cutmix_alpha=1.0, lam=1.5)


# ---------------------------------------------------------------- the public class
def test_device_augment_class(img, monkeypatch):
    labels = torch.arange(B)
    aug = FluxMPI.DeviceAugment(SIZE, pad=PAD)
    x0, y0 = aug(img, labels)
    x1, _ = aug(img, labels)
    assert y0 is labels and aug.state_dict() == {"seed": 0, "step": 2}
    assert torch.equal(bits(x0), bits(A.augment_reference(img, size=SIZE, pad=PAD, step=0)))
    assert torch.equal(bits(x1), bits(A.augment_reference(img, size=SIZE, pad=PAD, step=1)))
    xs, _ = aug(img, labels, step=0)  # an explicit step leaves the counter alone
    assert aug.step == 2 and torch.equal(bits(xs), bits(x0))
    # eval: centre crop, no flip, no mix, no step
    e0, ye = aug.eval()(img, labels)
    e1, _ = aug(img)
    assert ye is labels and aug.step == 2 and torch.equal(bits(e0), bits(e1))
    assert torch.equal(bits(e0), bits(A.augment_reference(img, size=SIZE, pad=PAD, crop="center", flip=False)))
    aug.train()
    # state
    other = FluxMPI.DeviceAugment(SIZE, pad=PAD, seed=5)
    other.load_state_dict({"seed": 0, "step": 1})
    assert torch.equal(bits(other(img)[0]), bits(x1)) and other.step == 2
    # ranks draw different crops from one seed
    import fluxmpi_amd.parallel as P
    monkeypatch.setattr(P, "Initialized", lambda: True)
    monkeypatch.setattr(P, "local_rank", lambda: 3)
    xr, _ = aug(img, step=0)
    assert torch.equal(bits(xr), bits(A.augment_reference(img, size=SIZE, pad=PAD, step=0, sample_offset=3 * B)))


def test_device_augment_mixing(img):
    labels = torch.tensor([1, 0, 3, 2, 3])
    with pytest.raises(ValueError, match="num_classes"):
        FluxMPI.DeviceAugment(SIZE, mixup_alpha=0.2)
    aug = FluxMPI.DeviceAugment(SIZE, pad=PAD, seed=3, mixup_alpha=0.4, cutmix_alpha=1.0, num_classes=4,
                                label_smoothing=0.1, channels=4)
    for step in range(4):
        d = aug.draw(step)
        x, y = aug(img, labels)
        assert torch.equal(bits(x), bits(A.augment_reference(img, size=SIZE, pad=PAD, seed=3, step=step, mix=d,
                                                               channels=4)))
        assert torch.equal(y, A.mix_targets(labels, 4, d.lam, 0.1))
    smooth = FluxMPI.DeviceAugment(SIZE, pad=PAD, label_smoothing=0.1, num_classes=4)
    assert torch.equal(smooth(img, labels)[1], A.mix_targets(labels, 4, 1.0, 0.1))
    with pytest.raises(ValueError, match="use_block"):
        aug(img, labels, use_block=True)  # the block lives on a GPU


# ---------------------------------------------------------------- argument checks
def test_argument_checks(img):
    ok = dict(size=SIZE, pad=PAD)
    bad = [
        (TypeError, dict(u8=img.float())),
        (TypeError, dict(u8=img.numpy())),
        (ValueError, dict(u8=img[0])),
        (ValueError, dict(u8=img[..., :2])),
        (ValueError, dict(u8=img[:, ::2])),
        (ValueError, dict(size=(H + 2 * PAD + 1, 36))),
        (ValueError, dict(size=(32, W + 2 * PAD + 1))),
        (ValueError, dict(size=(0, 36))),
        (TypeError, dict(size=32)),
        (ValueError, dict(pad=-1)),
        (ValueError, dict(fill=256)),
        (ValueError, dict(crop="centre")),
        (ValueError, dict(channels=1)),
        (ValueError, dict(channels=5)),
        (TypeError, dict(dtype=torch.float32)),
        (TypeError, dict(dtype=torch.uint8)),
        (ValueError, dict(seed=-1)),
        (ValueError, dict(seed=1 << 64)),
        (ValueError, dict(stream=1 << 30)),
        (ValueError, dict(step=1 << 32)),
        (ValueError, dict(step=-1)),
        (ValueError, dict(sample_offset=-1)),
        (ValueError, dict(mean=(0.5, 0.5))),
        (ValueError, dict(std=(1.0, 0.0, 1.0))),
        (ValueError, dict(mix=A.MixDraw(3, 0.5))),
        (ValueError, dict(mix=A.MixDraw(1, float("nan")))),
        (ValueError, dict(mix=A.MixDraw(2, 0.5, (0, 0, 33, 36)))),
        (ValueError, dict(mix=A.MixDraw(2, 0.5, (0, 0, 32, 37)))),
        (ValueError, dict(mix=A.MixDraw(2, 0.5, (-1, 0, 32, 36)))),
        (ValueError, dict(mix=A.MixDraw(2, 0.5, (9, 0, 8, 36)))),
        (ValueError, dict(dev_block=torch.zeros(8, dtype=torch.int32))),  # CPU tensors take no block
        (TypeError, dict(out=torch.empty(B, *SIZE, 3, dtype=torch.float16))),
        (ValueError, dict(out=torch.empty(B, *SIZE, 4, dtype=torch.bfloat16))),
        (ValueError, dict(out=torch.empty(B, 3, *SIZE, dtype=torch.bfloat16))),  # NCHW-contiguous: not the NHWC buffer
        (ValueError, dict(out=torch.empty(B * 32 * 36 * 3 + 8, dtype=torch.bfloat16)[1:-7].view(B, *SIZE, 3))),
    ]
    for exc, change in bad:
        kw = {**ok, **change}
        u8 = kw.pop("u8", img)
        with pytest.raises(exc, match="augment_batch"):
            A.augment_batch(u8, **kw)
    # the maximal output is fine, and out= is filled and returned
    full = A.augment_batch(img, size=(H + 2 * PAD, W + 2 * PAD), pad=PAD)
    assert tuple(full.shape) == (B, 3, H + 2 * PAD, W + 2 * PAD)
    out = torch.empty(B, *SIZE, 3, dtype=torch.bfloat16)
    x = A.augment_batch(img, out=out, **ok)
    assert x.data_ptr() == out.data_ptr() and torch.equal(bits(x), bits(A.augment_reference(img, **ok)))
    for name, call in (("sample_draws", lambda: A.sample_draws(4, 0, 1 << 30, 0, 0, 3, 3)),
                       ("sample_draws", lambda: A.sample_draws(4, 0, 0, 0, 0, 0, 3)),
                       ("draw_mix", lambda: A.draw_mix(0, 0, 1 << 32, SIZE, 0.2)),
                       ("DeviceAugment", lambda: FluxMPI.DeviceAugment(SIZE, channels=2)),
                       ("DeviceAugment", lambda: FluxMPI.DeviceAugment(SIZE, seed=-1))):
        with pytest.raises(ValueError, match=name):
            call()
    with pytest.raises(TypeError, match="DeviceAugment"):
        FluxMPI.DeviceAugment(SIZE, dtype=torch.float32)


def test_four_channel_input_on_the_cpu_paths():
    """The ResNet takes the 4-channel batch everywhere: a path that runs the 3-channel filter reads its
    first three channels."""
    from fluxmpi_amd.models import resnet18ish
    torch.manual_seed(0)
    model = resnet18ish(num_classes=4).eval()
    x4 = torch.randn(2, 4, 32, 32).contiguous(memory_format=torch.channels_last)
    x4[:, 3] = 0
    with torch.no_grad():
        assert torch.equal(model(x4), model(x4[:, :3]))
