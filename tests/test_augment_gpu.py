"""The device input pipeline on the GPU (``csrc/kernels/augment.hip``): every comparison is bit for bit
(``view(int16)``) against ``ops.augment.augment_reference``.

The base case: ``B = 5`` images of 37 x 41, ``pad = 4``, ``size = (32, 36)``: ranges ``rx = ry = 14``; a
row is 4 vector groups of 8 pixels and a tail of 4; with seed 0 the five samples draw both flip values
and four distinct ``ox`` (two crops inside the image, three over its edge); sample 2 partners itself.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import fluxmpi_amd as FluxMPI
from fluxmpi_amd.ops import augment as A

pytestmark = pytest.mark.gpu

B, H, W, PAD, SIZE = 5, 37, 41, 4, (32, 36)
DTYPES = [torch.bfloat16, torch.float16]
MIXUP = A.MixDraw(1, 0.3)
MODES = {
    "none": A.MixDraw(),
    "mixup0": A.MixDraw(1, 0.0), "mixup1": A.MixDraw(1, 1.0), "mixup.3": MIXUP,
    "cut_interior": A.MixDraw(2, 0.5, (5, 7, 20, 30)), "cut_two_edges": A.MixDraw(2, 0.5, (10, 20, 32, 36)),
    "cut_empty": A.MixDraw(2, 1.0, (8, 9, 8, 9)), "cut_full": A.MixDraw(2, 0.0, (0, 0, 32, 36)),
}


@pytest.fixture(scope="module")
def images():
    """The uint8 batch inside a larger buffer, at byte offsets 0..3 of a 16-byte-aligned base."""
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    img[0, 0, 0] = torch.tensor([0, 255, 128], dtype=torch.uint8)
    n = img.numel()
    buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    views = []
    for off in range(4):
        hold = buf.clone()
        hold[off:off + n] = img.reshape(-1).cuda()
        v = hold[off:off + n].view(B, H, W, 3)
        assert v.data_ptr() % 16 == off
        views.append(v)
    ox, oy, flip = A.sample_draws(B, 0, 0, 0, 0, W + 2 * PAD - SIZE[1] + 1, H + 2 * PAD - SIZE[0] + 1)
    # what makes the base case a test: both flip values, four distinct offsets, crops inside the image
    # and over its edge
    assert set(flip.tolist()) == {0, 1} and len(set(ox.tolist())) >= 4
    inside = [(0 <= x - PAD and x - PAD + SIZE[1] <= W) for x in ox.tolist()]
    assert any(inside) and not all(inside)
    return img, views


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def check(u8_gpu, u8_cpu, what="", **kw):
    got = A.augment_batch(u8_gpu, **kw)
    want = A.augment_reference(u8_cpu, **kw)
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == want.dtype
    assert got.permute(0, 2, 3, 1).is_contiguous() and got.data_ptr() % 16 == 0
    g, w = bits(got.permute(0, 2, 3, 1)), bits(want.permute(0, 2, 3, 1))
    bad = (g != w)
    assert not bad.any(), (what, kw, int(bad.sum()), bad.nonzero()[:4].tolist())
    if kw.get("channels", 3) == 4:
        assert not g[..., 3].any(), (what, "channel 3 is not +0")
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [3, 4])
def test_alignment_and_fill(gpu_ext, images, C, dtype):
    img, views = images
    for off in range(4):
        for fill in (0, 255):
            for name in ("none", "mixup.3"):
                check(views[off], img, (off, fill, name), size=SIZE, pad=PAD, fill=fill, channels=C, dtype=dtype,
                      mix=MODES[name])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [3, 4])
def test_modes(gpu_ext, images, C, dtype):
    img, views = images
    for name, mix in MODES.items():
        check(views[1], img, name, size=SIZE, pad=PAD, fill=7, channels=C, dtype=dtype, mix=mix, step=3, stream=2,
              seed=(0x12345678 << 32) | 0x9ABCDEF0, sample_offset=(1 << 32) + 5)


GEOMETRIES = {
    "no_flip": dict(size=SIZE, pad=PAD, flip=False),
    "center": dict(size=SIZE, pad=PAD, crop="center"),
    "identity": dict(size=(H, W), pad=0),  # range 1; 5 groups and a tail of 1
    "w8": dict(size=(32, 8), pad=PAD),  # vector groups only
    "w7": dict(size=(32, 7), pad=PAD),  # tail only
    "h1": dict(size=(1, 36), pad=PAD),
    "wide_pad": dict(size=(45, 57), pad=10),  # larger than the image: every crop crosses the edge
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [3, 4])
def test_geometries(gpu_ext, images, C, dtype):
    img, views = images
    for name, geo in GEOMETRIES.items():
        h, w = geo["size"]
        for mix in (A.MixDraw(), MIXUP, A.MixDraw(2, 0.5, (0, min(2, w), h, w))):
            check(views[3], img, (name, mix), channels=C, dtype=dtype, mix=mix, **geo)
    # B = 1: the partner is the sample itself
    for mix in (A.MixDraw(), MIXUP, MODES["cut_interior"]):
        check(views[2][2:3], img[2:3], ("B1", mix), size=SIZE, pad=PAD, channels=C, dtype=dtype, mix=mix)


def test_empty_batch(gpu_ext, images):
    img, views = images
    x = A.augment_batch(views[0][:0], size=SIZE, pad=PAD, channels=4)
    assert tuple(x.shape) == (0, 4, *SIZE)


def test_index_past_2_31(gpu_ext):
    """Sample 3 of four 16384 x 16384 images starts 2.4e9 bytes into the batch: its centre crop is the
    identity transform of those bytes."""
    n, side = 4, 16384
    u = torch.empty(n, side, side, 3, dtype=torch.uint8, device="cuda")
    lo = (side - 8) // 2, (side - 24) // 2
    g = torch.Generator().manual_seed(9)
    patch = torch.randint(0, 256, (n, 8, 24, 3), dtype=torch.uint8, generator=g)
    u[:, lo[0]:lo[0] + 8, lo[1]:lo[1] + 24] = patch.cuda()
    assert u[3, lo[0], lo[1]].data_ptr() - u.data_ptr() > 1 << 31
    got = A.augment_batch(u, size=(8, 24), crop="center", channels=4, mix=MIXUP)
    want = A.augment_reference(patch, size=(8, 24), crop="center", channels=4, mix=MIXUP)
    torch.cuda.synchronize()
    assert torch.equal(bits(got.permute(0, 2, 3, 1)), bits(want.permute(0, 2, 3, 1)))


@pytest.mark.parametrize("name", ["none", "mixup.3", "cut_interior"])
def test_block_route_equals_value_route(gpu_ext, images, name):
    img, views = images
    mix = MODES[name]
    kw = dict(size=SIZE, pad=PAD, channels=4, seed=11)
    by_value = check(views[1], img, name, step=6, mix=mix, **kw)
    block = torch.zeros(A.BLOCK_WORDS, dtype=torch.int32, device="cuda")
    A.block_set(block, 6, mix)
    # the block wins over the host's step and mix
    by_block = A.augment_batch(views[1], step=1234, mix=A.MixDraw(), dev_block=block, **kw)
    torch.cuda.synchronize()
    words = block.cpu().tolist()
    assert words[:6] == [6, mix.mode, *mix.box] and words[7] == 0
    assert float(A.block_lam(block)) == float(np.float32(mix.lam))
    assert torch.equal(bits(by_block), bits(by_value))


def test_graph_capture_follows_the_block(gpu_ext, images):
    img, views = images
    labels = torch.tensor([1, 0, 3, 2, 3], device="cuda")
    kw = dict(pad=PAD, channels=4, seed=3, mixup_alpha=0.4, cutmix_alpha=1.0, num_classes=4, label_smoothing=0.1)
    aug = FluxMPI.DeviceAugment(SIZE, **kw)
    eager = FluxMPI.DeviceAugment(SIZE, **kw)
    aug.prepare(step=0, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug(views[0], labels, use_block=True)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x, y = aug(views[0], labels, use_block=True)
    seen = []
    for step in (0, 1):
        drawn = aug.prepare(step=step)
        graph.replay()
        torch.cuda.synchronize()
        xe, ye = eager(views[0], labels, step=step)
        assert drawn == eager.draw(step)
        assert torch.equal(bits(x), bits(xe)), step
        assert torch.equal(y, ye), step
        seen.append((bits(x).clone(), y.clone()))
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[0][1], seen[1][1])


def test_out_is_reused(gpu_ext, images):
    img, views = images
    out = torch.full((B, *SIZE, 4), float("nan"), dtype=torch.bfloat16, device="cuda")
    x = A.augment_batch(views[0], size=SIZE, pad=PAD, channels=4, out=out)
    assert x.data_ptr() == out.data_ptr() and tuple(x.shape) == (B, 4, *SIZE)
    want = A.augment_reference(img, size=SIZE, pad=PAD, channels=4)
    assert torch.equal(bits(out), bits(want.permute(0, 2, 3, 1)))
    x2 = A.augment_batch(views[0], size=SIZE, pad=PAD, channels=4, step=1, out=x)  # the view is taken too
    assert x2.data_ptr() == out.data_ptr()
    assert torch.equal(bits(out), bits(A.augment_reference(img, size=SIZE, pad=PAD, channels=4, step=1)
                                       .permute(0, 2, 3, 1)))
    with pytest.raises(ValueError, match="augment_batch"):
        A.augment_batch(views[0], size=SIZE, pad=PAD, channels=4, out=out.view(-1)[4:4 + 16].view(1, 1, 4, 4))
    with pytest.raises(ValueError, match="aligned"):
        big = torch.empty(out.numel() + 8, dtype=torch.bfloat16, device="cuda")
        A.augment_batch(views[0], size=SIZE, pad=PAD, channels=4, out=big[1:1 + out.numel()].view(B, *SIZE, 4))


def test_device_augment_eval_and_step(gpu_ext, images):
    img, views = images
    aug = FluxMPI.DeviceAugment(SIZE, pad=PAD, channels=3)
    labels = torch.arange(B, device="cuda")
    x0, y0 = aug(views[0], labels)
    x1, _ = aug(views[0], labels)
    assert y0 is labels and aug.state_dict() == {"seed": 0, "step": 2}
    assert torch.equal(bits(x0), bits(A.augment_reference(img, size=SIZE, pad=PAD, step=0)))
    assert torch.equal(bits(x1), bits(A.augment_reference(img, size=SIZE, pad=PAD, step=1)))
    e0, _ = aug.eval()(views[0])
    e1, _ = aug(views[0])
    assert aug.step == 2 and torch.equal(bits(e0), bits(e1))
    assert torch.equal(bits(e0), bits(A.augment_reference(img, size=SIZE, pad=PAD, crop="center", flip=False)))


def test_stem_takes_the_four_channel_batch(gpu_ext):
    from fluxmpi_amd.ops import stem as S
    g = torch.Generator().manual_seed(2)
    u = torch.randint(0, 256, (2, 256, 256, 3), dtype=torch.uint8, generator=g).cuda()
    kw = dict(size=(224, 224), seed=4, step=2)
    x3 = A.augment_batch(u, channels=3, **kw)
    x4 = A.augment_batch(u, channels=4, **kw)
    conv = nn.Conv2d(3, 64, 7, 2, 3, bias=False).cuda()
    bn3, bn4 = nn.BatchNorm2d(64).cuda(), nn.BatchNorm2d(64).cuda()
    if not S.supported(x3, conv.weight, conv, bn3):
        pytest.skip("the stem kernels do not take this input here")
    assert S.supported(x4, conv.weight, conv, bn4)
    assert torch.equal(bits(x4[:, :3]), bits(x3))
    y3 = S.stem(x3, conv, bn3)
    y4 = S.stem(x4, conv, bn4)
    (y3.float().sum()).backward()
    g3 = conv.weight.grad.clone()
    conv.weight.grad = None
    (y4.float().sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(bits(y3), bits(y4))
    assert torch.equal(bn3.running_var, bn4.running_var)
    assert torch.equal(g3, conv.weight.grad)
