"""The resampling form of the device input pipeline on the GPU (``csrc/kernels/resize_crop.hip``): every
comparison is bit for bit (``view(int16)``) against ``ops.augment.resized_crop_reference``.

The base case: ``B = 5`` images of 37 x 41, output ``(32, 36)``: a row is 4 vector groups of 8 pixels and a
tail of 4; sample 2 partners itself. The batch is a view in the middle of a larger buffer, more than one
image of sentinel bytes in front and behind, at byte offsets 0..3 of a 16-byte-aligned address: a wrong
index shows as a mismatch, not as an access outside the allocation.
"""
import numpy as np
import pytest
import torch

import fluxmpi_amd as FluxMPI
from fluxmpi_amd.ops import augment as A

pytestmark = pytest.mark.gpu

B, H, W = 5, 37, 41
DTYPES = [torch.bfloat16, torch.float16]
MIXUP = A.MixDraw(1, 0.3)
# the table of tests/test_augment_gpu.py
MODES = {
    "none": A.MixDraw(),
    "mixup0": A.MixDraw(1, 0.0), "mixup1": A.MixDraw(1, 1.0), "mixup.3": MIXUP,
    "cut_interior": A.MixDraw(2, 0.5, (5, 7, 20, 30)), "cut_two_edges": A.MixDraw(2, 0.5, (10, 20, 32, 36)),
    "cut_empty": A.MixDraw(2, 1.0, (8, 9, 8, 9)), "cut_full": A.MixDraw(2, 0.0, (0, 0, 32, 36)),
}
# output sizes: the base case, vector groups only, tail only, and a reduction of the 37 rows to 3 (12x:
# an output row's source pair is staged on its own; every other height stages the union of the rows)
SIZES = [(32, 36), (32, 8), (32, 5), (3, 36)]
# five boxes (top, left, bh, bw, flip) per family, both flip values in each
FAMILIES = {
    "identity": [(0, 0, 32, 36, 0), (5, 5, 32, 36, 1), (2, 3, 32, 36, 1), (5, 0, 32, 36, 0), (0, 5, 32, 36, 1)],
    "enlarge": [(3, 4, 9, 11, 0), (0, 0, 1, 1, 1), (36, 40, 1, 1, 0), (20, 15, 9, 11, 1), (28, 30, 9, 11, 0)],
    "whole": [(0, 0, H, W, 0), (0, 0, H, W, 1), (0, 0, H, W, 0), (0, 0, H, W, 1), (0, 0, H, W, 1)],
    "edges": [(0, 5, 20, 30, 0), (17, 5, 20, 30, 1), (5, 0, 25, 20, 1), (5, 21, 25, 20, 0), (30, 33, 7, 8, 1)],
    "bw1": [(2, 7, 30, 1, 0), (0, 40, 37, 1, 1), (0, 0, 37, 1, 0), (10, 20, 1, 1, 1), (36, 0, 1, 41, 0)],
    "mixed": [(1, 2, 35, 17, 1), (0, 0, 4, 41, 0), (9, 9, 19, 23, 0), (0, 0, 37, 41, 1), (11, 30, 26, 11, 0)],
}


def table(name):
    return np.array(FAMILIES[name], dtype=np.int32)


def fit(mix, size):
    """The mode with its cutmix box clipped into an output of ``size``."""
    h, w = size
    y0, x0, y1, x1 = mix.box
    return A.MixDraw(mix.mode, mix.lam, (min(y0, h), min(x0, w), min(y1, h), min(x1, w)))


@pytest.fixture(scope="module")
def images():
    """``(img, views, buffers)``: the CPU batch, its four GPU views at byte offsets 0..3 and their buffers."""
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    img[0, 0, 0] = torch.tensor([0, 255, 128], dtype=torch.uint8)
    n = img.numel()
    guard = (H * W * 3 + 15) // 16 * 16 + 16  # more than one image, a multiple of 16
    views, buffers = [], []
    for off in range(4):
        buf = torch.full((guard + off + n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[guard + off:guard + off + n] = img.reshape(-1).cuda()
        v = buf[guard + off:guard + off + n].view(B, H, W, 3)
        assert v.data_ptr() % 16 == off
        views.append(v)
        buffers.append(buf)
    return img, views, buffers


def bits(t):
    return t.contiguous().view(torch.int16)


_WANT = {}


def want_bits(img, boxes, key, **kw):
    """The reference's bits on the GPU, computed once per distinct call."""
    if key not in _WANT:
        _WANT[key] = bits(A.resized_crop_reference(img, boxes, **kw).permute(0, 2, 3, 1)).cuda()
    return _WANT[key]


def check(u8_gpu, img, boxes, key, **kw):
    got = A.resized_crop_batch(u8_gpu, torch.from_numpy(boxes).cuda(), **kw)
    want = want_bits(img, boxes, key, **kw)
    assert got.dtype == kw["dtype"] and tuple(got.shape) == (img.shape[0], kw["channels"], *kw["size"])
    assert got.permute(0, 2, 3, 1).is_contiguous() and got.data_ptr() % 16 == 0
    g = bits(got.permute(0, 2, 3, 1))
    if not torch.equal(g, want):
        bad = g != want
        raise AssertionError((key, int(bad.sum()), bad.nonzero()[:4].tolist()))
    if kw["channels"] == 4:
        assert not g[..., 3].any(), (key, "channel 3 is not +0")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [3, 4])
def test_families_modes_widths_alignments(gpu_ext, images, C, dtype):
    img, views, _ = images
    for fam in FAMILIES:
        boxes = table(fam)
        for size in SIZES:
            for name, mode in MODES.items():
                mix = fit(mode, size)
                for off in range(4):
                    check(views[off], img, boxes, (fam, size, name, C, dtype), size=size, channels=C, dtype=dtype, mix=mix)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["none", "mixup.3", "cut_interior"])
def test_enlargement_and_single_sample(gpu_ext, images, name):
    """An output larger than the image (every source row is read by several output rows), and B = 1 (the
    partner is the sample itself)."""
    img, views, _ = images
    mix = MODES[name]
    for fam in ("whole", "enlarge", "mixed"):
        check(views[1], img, table(fam), (fam, "up", name), size=(75, 50), channels=4, dtype=torch.bfloat16, mix=mix)
        check(views[2][2:3], img[2:3], table(fam)[2:3], (fam, "B1", name), size=(32, 36), channels=3,
              dtype=torch.float16, mix=mix)


def test_identity_scale_equals_the_crop_kernel(gpu_ext, images):
    img, views, _ = images
    h, w = 32, 36
    ox, oy, fl = A.sample_draws(B, 0, 0, 0, 0, W - w + 1, H - h + 1)
    boxes = np.stack([oy, ox, np.full(B, h), np.full(B, w), fl], axis=1).astype(np.int32)
    for mix in (A.MixDraw(), MIXUP):
        a = A.resized_crop_batch(views[3], boxes, size=(h, w), channels=4, mix=mix)  # a host table: uploaded
        b = A.augment_batch(views[3], size=(h, w), pad=0, channels=4, mix=mix)
        assert torch.equal(bits(a), bits(b))


def test_rrc_boxes_at_the_flagship_shape(gpu_ext):
    """256 x 256 -> 224 x 224 with drawn boxes: 8 output rows per workgroup, 28 workgroups per sample."""
    g = torch.Generator().manual_seed(6)
    img = torch.randint(0, 256, (4, 256, 256, 3), dtype=torch.uint8, generator=g)
    boxes = A.rrc_boxes(4, 256, 256, seed=1, step=3)
    u = img.cuda()
    for C, mix in ((3, A.MixDraw()), (4, MIXUP), (4, A.MixDraw(2, 0.5, (50, 60, 200, 224)))):
        kw = dict(size=(224, 224), channels=C, dtype=torch.bfloat16, mix=mix)
        check(u, img, boxes, ("flagship", C, mix), **kw)


def test_empty_batch(gpu_ext, images):
    img, views, _ = images
    x = A.resized_crop_batch(views[0][:0], torch.zeros(0, 5, dtype=torch.int32, device="cuda"), size=(32, 36), channels=4)
    assert tuple(x.shape) == (0, 4, 32, 36)


def test_device_table_is_clamped(gpu_ext, images):
    """A device table is used as it is; it forms addresses, so the kernel clamps it (the guard bands make
    the test safe)."""
    img, views, _ = images
    wild = np.array([[-3, W, H + 9, 5, 7], [2, 3, 4, 500, -1], [-(1 << 30), -(1 << 30), 1 << 30, 1 << 30, 2],
                     [1 << 30, 1 << 30, -5, 0, 1], [0, 0, H, W, 0]], dtype=np.int32)
    clamped = A.clamp_boxes(wild, H, W)
    assert clamped[0].tolist() == [0, W - 1, H, 1, 1] and clamped[2].tolist() == [0, 0, H, W, 0]
    assert clamped[3].tolist() == [H - 1, W - 1, 1, 1, 1]
    for mix in (A.MixDraw(), MIXUP):
        kw = dict(size=(32, 36), channels=4, dtype=torch.bfloat16, mix=mix)
        got = A.resized_crop_batch(views[1], torch.from_numpy(wild).cuda(), **kw)
        want = A.resized_crop_reference(img, clamped.astype(np.int32), **kw)
        assert torch.equal(bits(got).cpu(), bits(want))
        assert torch.equal(bits(want), bits(A.resized_crop_reference(img, wild, **kw)))
    with pytest.raises(ValueError, match="resized_crop_batch: the box of sample 0"):
        A.resized_crop_batch(views[1], wild, size=(32, 36))  # the same table on the host is refused
    with pytest.raises(ValueError, match="resized_crop_batch: a device table"):
        A.resized_crop_batch(views[1], torch.from_numpy(wild).cuda().long(), size=(32, 36))
    with pytest.raises(ValueError, match="resized_crop_batch: a device table"):
        A.resized_crop_batch(img, torch.from_numpy(wild).cuda(), size=(32, 36))


def test_index_past_2_31(gpu_ext):
    """Eleven 16384 x 4096 images are 2.2e9 bytes: small boxes in the first and the last image, which are
    partners under mixup; the reference runs on the patches."""
    n, rows, cols = 11, 16384, 4096
    u = torch.empty(n, rows, cols, 3, dtype=torch.uint8, device="cuda")
    g = torch.Generator().manual_seed(9)
    patch = torch.randint(0, 256, (n, 9, 11, 3), dtype=torch.uint8, generator=g)
    where = [(rows - 9 - 3, cols - 11 - 2) if b >= n // 2 else (5, 7) for b in range(n)]
    for b, (y, x) in enumerate(where):
        u[b, y:y + 9, x:x + 11] = patch[b].cuda()
    assert u[n - 1, where[-1][0], where[-1][1]].data_ptr() - u.data_ptr() > 1 << 31
    flips = [b & 1 for b in range(n)]
    boxes = np.array([(y, x, 9, 11, f) for (y, x), f in zip(where, flips)], dtype=np.int32)
    local = np.array([(0, 0, 9, 11, f) for f in flips], dtype=np.int32)
    kw = dict(size=(8, 24), channels=4, mix=MIXUP)
    got = A.resized_crop_batch(u, torch.from_numpy(boxes).cuda(), **kw)
    want = A.resized_crop_reference(patch, local, **kw)
    torch.cuda.synchronize()
    assert torch.equal(bits(got).cpu(), bits(want))


def test_out_is_reused(gpu_ext, images):
    img, views, _ = images
    boxes = table("mixed")
    kw = dict(size=(32, 36), channels=4)
    out = torch.full((B, 32, 36, 4), float("nan"), dtype=torch.bfloat16, device="cuda")
    x = A.resized_crop_batch(views[0], boxes, out=out, **kw)
    assert x.data_ptr() == out.data_ptr() and tuple(x.shape) == (B, 4, 32, 36)
    assert torch.equal(bits(out).cpu(), bits(A.resized_crop_reference(img, boxes, **kw).permute(0, 2, 3, 1)))
    x2 = A.resized_crop_batch(views[0], table("edges"), out=x, **kw)  # the view is taken too
    assert x2.data_ptr() == out.data_ptr()
    assert torch.equal(bits(out).cpu(), bits(A.resized_crop_reference(img, table("edges"), **kw).permute(0, 2, 3, 1)))
    with pytest.raises(ValueError, match="aligned"):
        big = torch.empty(out.numel() + 8, dtype=torch.bfloat16, device="cuda")
        A.resized_crop_batch(views[0], boxes, out=big[1:1 + out.numel()].view(B, 32, 36, 4), **kw)


@pytest.mark.parametrize("name", ["none", "mixup.3", "cut_interior"])
def test_block_route_equals_value_route(gpu_ext, images, name):
    img, views, _ = images
    mix = MODES[name]
    boxes = torch.from_numpy(table("mixed")).cuda()
    kw = dict(size=(32, 36), channels=4)
    by_value = A.resized_crop_batch(views[1], boxes, mix=mix, **kw)
    block = torch.zeros(A.BLOCK_WORDS, dtype=torch.int32, device="cuda")
    A.block_set(block, 6, mix)
    by_block = A.resized_crop_batch(views[1], boxes, mix=A.MixDraw(), dev_block=block, **kw)  # the block wins
    assert torch.equal(bits(by_block), bits(by_value))
    assert torch.equal(bits(by_value).cpu(), bits(A.resized_crop_reference(img, table("mixed"), mix=mix, **kw)))


def test_graph_capture_follows_the_block_and_the_table(gpu_ext, images):
    img, views, _ = images
    labels = torch.tensor([1, 0, 3, 2, 3], device="cuda")
    kw = dict(crop="resized", channels=4, seed=3, mixup_alpha=0.4, num_classes=4, label_smoothing=0.1,
              scale=(0.2, 1.0))
    aug = FluxMPI.DeviceAugment((32, 36), **kw)
    eager = FluxMPI.DeviceAugment((32, 36), **kw)
    with pytest.raises(ValueError, match="prepare needs batch"):
        aug.prepare(step=0, device="cuda")
    aug.prepare(step=0, device="cuda", batch=B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug(views[0], labels, use_block=True)  # warm-up outside the capture: it also creates the table
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x, y = aug(views[0], labels, use_block=True)
    seen = []
    for step in (0, 1):
        drawn = aug.prepare(step, batch=B)
        graph.replay()
        torch.cuda.synchronize()
        xe, ye = eager(views[0], labels, step=step)
        assert drawn == eager.draw(step) and drawn.mode == 1
        assert torch.equal(bits(x), bits(xe)), step
        assert torch.equal(y, ye), step
        want = A.resized_crop_reference(img, A.rrc_boxes(B, H, W, scale=(0.2, 1.0), seed=3, step=step), size=(32, 36),
                                        channels=4, mix=drawn)
        assert torch.equal(bits(x).cpu(), bits(want)), step
        seen.append((bits(x).clone(), y.clone()))
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[0][1], seen[1][1])
    with pytest.raises(ValueError, match="DeviceAugment: the device table of boxes was created for batch 5"):
        aug.prepare(2, batch=B + 1)
    with pytest.raises(ValueError, match="DeviceAugment: the device table of boxes is for 5 images"):
        aug(views[0][:3], labels[:3], use_block=True)


def test_eval_at_the_stored_scale_equals_the_crop_pipeline(gpu_ext):
    g = torch.Generator().manual_seed(2)
    u = torch.randint(0, 256, (2, 256, 256, 3), dtype=torch.uint8, generator=g).cuda()
    a, _ = FluxMPI.DeviceAugment(224, crop="resized", channels=4).eval()(u)
    b, _ = FluxMPI.DeviceAugment(224, crop="pad", channels=4).eval()(u)
    assert torch.equal(bits(a), bits(b))
    t, _ = FluxMPI.DeviceAugment(224, crop="resized", channels=4, seed=7)(u, step=4)
    want = A.resized_crop_reference(u.cpu(), A.rrc_boxes(2, 256, 256, seed=7, step=4), size=(224, 224), channels=4)
    assert torch.equal(bits(t).cpu(), bits(want))
