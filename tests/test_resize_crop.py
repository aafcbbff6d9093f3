"""The resampling form of the device input pipeline on the CPU: the numpy reference of
``resized_crop_batch`` (the kernel's oracle), the box draws and ``DeviceAugment(crop="resized")``.

The bound of the float64 comparison: the integer arithmetic rounds once at the end (0.5 of a byte level)
and quantises the two weights to 1/2048, each within 2^-12 of the exact weight, which moves a value that
spans at most 255 levels by at most 255 * 2^-12 per weight: ``0.5 + 255 * 2 * 2^-12 < 0.63``.
"""
import numpy as np
import pytest
import torch

import fluxmpi_amd as FluxMPI
from fluxmpi_amd.ops import augment as A

BOUND = 0.63
RAW = dict(mean=(0.0, 0.0, 0.0), std=(1 / 255, 1 / 255, 1 / 255), dtype=torch.float32)  # y = the resampled byte


def bits(t):
    return t.contiguous().view(torch.int16)


def rand_images(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)


def exact_bilinear(img, box, h, w):
    """float64 bilinear interpolation of one image's box, half-pixel centres, edge-clamped: [h, w, 3]."""
    top, left, bh, bw, flip = (int(v) for v in box)
    src = img[top:top + bh, left:left + bw].astype(np.float64)
    cy = np.clip((np.arange(h) + 0.5) * bh / h - 0.5, 0, bh - 1)
    cx = np.clip((np.arange(w) + 0.5) * bw / w - 0.5, 0, bw - 1)
    y0, x0 = np.floor(cy).astype(int), np.floor(cx).astype(int)
    y1, x1 = np.minimum(y0 + 1, bh - 1), np.minimum(x0 + 1, bw - 1)
    fy, fx = (cy - y0)[:, None, None], (cx - x0)[None, :, None]
    up = src[y0][:, x0] * (1 - fx) + src[y0][:, x1] * fx
    dn = src[y1][:, x0] * (1 - fx) + src[y1][:, x1] * fx
    out = up * (1 - fy) + dn * fy
    return out[:, ::-1] if flip else out


# ---- the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("mix", [None, (1, 0.3, (0, 0, 0, 0)), (2, 0.5, (5, 7, 20, 30))])
def test_identity_scale_is_the_plain_crop(flip, mix):
    B, H, W, h, w = 5, 37, 41, 32, 36
    u = rand_images(B, H, W)
    kw = dict(size=(h, w), channels=4, mix=mix)
    ox, oy, fl = A.sample_draws(B, 3, 0, 2, 0, W - w + 1, H - h + 1)
    if flip:
        assert set(fl.tolist()) == {0, 1}
    else:
        fl = np.zeros_like(fl)
    boxes = np.stack([oy, ox, np.full(B, h), np.full(B, w), fl], axis=1).astype(np.int32)
    got = A.resized_crop_batch(u, boxes, **kw)
    want = A.augment_reference(u, pad=0, seed=3, step=2, flip=bool(flip), **kw)
    assert got.shape == want.shape == (B, 4, h, w) and got.dtype == torch.bfloat16
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(got), bits(A.resized_crop_reference(u, boxes, **kw)))


def test_within_the_bound_of_float64_bilinear():
    H, W = 61, 67
    u = rand_images(6, H, W, seed=4)
    rng = np.random.default_rng(7)
    fixed = [(0, 0, 1, 1, 0), (H - 1, W - 1, 1, 1, 1), (0, 5, 9, 11, 0), (H - 9, 5, 9, 11, 1), (7, 0, 9, 11, 1),
             (7, W - 11, 9, 11, 0), (0, 0, H, W, 0), (0, 0, H, W, 1), (10, 12, 1, 30, 0), (10, 12, 30, 1, 1)]
    worst = 0.0
    for h, w in [(32, 36), (3, 5), (80, 90), (1, 1), (61, 67)]:
        boxes = list(fixed)
        while len(boxes) % 6 or len(boxes) < 60:
            bh, bw = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
            boxes.append((int(rng.integers(0, H - bh + 1)), int(rng.integers(0, W - bw + 1)), bh, bw,
                          int(rng.integers(0, 2))))
        for k in range(0, len(boxes), 6):
            t = np.array(boxes[k:k + 6], dtype=np.int32)
            got = A.resized_crop_reference(u, t, size=(h, w), **RAW).permute(0, 2, 3, 1).numpy()
            assert np.array_equal(got, np.rint(got)) and got.min() >= 0 and got.max() <= 255  # bytes
            for b in range(6):
                err = np.abs(got[b] - exact_bilinear(u[b].numpy(), t[b], h, w)).max()
                worst = max(worst, float(err))
                assert err <= BOUND, (h, w, t[b].tolist(), err)
    print(f"worst |v - exact| = {worst:.4f} of a byte level (bound {BOUND})")


def test_constant_image_gives_the_constant():
    u = torch.full((2, 19, 23, 3), 0, dtype=torch.uint8)
    u[..., 0], u[..., 1], u[..., 2] = 255, 1, 128
    boxes = np.array([[0, 0, 19, 23, 0], [3, 4, 5, 2, 1]], dtype=np.int32)
    for size in [(7, 9), (40, 50), (19, 23)]:
        got = A.resized_crop_reference(u, boxes, size=size, **RAW)
        for c, v in enumerate((255, 1, 128)):
            assert (got[:, c] == v).all()


def test_two_by_two_to_four_by_four_by_hand():
    # weights 0, 1/4, 3/4, 1 along each axis: every value below is an exact integer
    u = torch.zeros(1, 3, 4, 3, dtype=torch.uint8)
    u[0, 1:3, 1:3, :] = torch.tensor([[0, 200], [100, 60]], dtype=torch.uint8)[:, :, None]
    want = np.array([[0, 50, 150, 200], [25, 60, 130, 165], [75, 80, 90, 95], [100, 90, 70, 60]], dtype=np.float32)
    got = A.resized_crop_reference(u, np.array([[1, 1, 2, 2, 0]], dtype=np.int32), size=(4, 4), **RAW)
    for c in range(3):
        assert np.array_equal(got[0, c].numpy(), want)


@pytest.mark.parametrize("size", [(32, 36), (5, 7), (50, 60)])
def test_flip_reverses_the_columns(size):
    u = rand_images(3, 37, 41, seed=2)
    boxes = np.array([[0, 0, 37, 41, 0], [5, 6, 9, 11, 0], [30, 2, 7, 39, 0]], dtype=np.int32)
    flipped = boxes.copy()
    flipped[:, 4] = 1
    a = A.resized_crop_reference(u, boxes, size=size)
    b = A.resized_crop_reference(u, flipped, size=size)
    assert torch.equal(bits(b), bits(a.flip(-1)))


def test_the_reference_clamps_like_the_kernel():
    H, W = 37, 41
    t = np.array([[-3, W, H + 9, 5, 7], [2, 3, 4, 500, -1]], dtype=np.int32)
    c = A.clamp_boxes(t, H, W)
    assert c.tolist() == [[0, W - 1, H, 1, 1], [2, 3, 4, W - 3, 1]]
    u = rand_images(2, H, W)
    assert torch.equal(bits(A.resized_crop_reference(u, t, size=(8, 8))),
                       bits(A.resized_crop_reference(u, c, size=(8, 8))))
    ok = A.rrc_boxes(16, H, W)
    assert np.array_equal(A.clamp_boxes(ok, H, W), ok)


# ---- the boxes -------------------------------------------------------------------------------------
def test_rrc_boxes_lie_inside_and_follow_scale_and_ratio():
    H, W, n = 200, 300, 4000
    boxes, attempts = A.rrc_boxes(n, H, W, seed=5, return_attempts=True)
    assert boxes.dtype == np.int32 and boxes.shape == (n, 5)
    top, left, bh, bw, flip = boxes.T.astype(np.int64)
    assert (top >= 0).all() and (bh >= 1).all() and (top + bh <= H).all()
    assert (left >= 0).all() and (bw >= 1).all() and (left + bw <= W).all()
    assert set(flip.tolist()) == {0, 1}
    acc = attempts < 10  # drawn, not the fallback
    assert acc.sum() > 0.99 * n
    # a side is within 1/2 of its unrounded value: the area and aspect of (bh +- 1/2, bw +- 1/2) bracket the draw
    lo_area, hi_area = (bh - 0.5) * (bw - 0.5) / (H * W), (bh + 0.5) * (bw + 0.5) / (H * W)
    lo_asp, hi_asp = (bw - 0.5) / (bh + 0.5), (bw + 0.5) / (bh - 0.5)
    assert (lo_area[acc] <= 1.0).all() and (hi_area[acc] >= 0.08).all()
    assert (lo_asp[acc] <= 4 / 3).all() and (hi_asp[acc] >= 3 / 4).all()
    # the draws spread: small and large boxes, both orientations, offsets over the range
    assert bh.min() < H // 3 and bh.max() > 0.9 * H and (bw > bh).any() and (bw < bh).any()
    assert len(set(top.tolist())) > 50 and len(set(left.tolist())) > 50
    assert (attempts > 0).any()  # some first attempts did not fit and were drawn again
    assert not A.rrc_boxes(64, H, W, flip=False)[:, 4].any()
    # the flip is the translation crop's
    assert np.array_equal(flip, A.sample_draws(n, 5, 0, 0, 0, 7, 9)[2])


def test_rrc_boxes_are_deterministic_and_per_sample():
    kw = dict(seed=(1 << 40) + 3, stream=2, step=9)
    a = A.rrc_boxes(8, 64, 80, **kw)
    assert np.array_equal(a, A.rrc_boxes(8, 64, 80, **kw))
    assert np.array_equal(a, np.concatenate([A.rrc_boxes(4, 64, 80, **kw), A.rrc_boxes(4, 64, 80, sample_offset=4, **kw)]))
    big = A.rrc_boxes(4, 64, 80, sample_offset=(1 << 40) + 1, **kw)
    assert np.array_equal(big[1:], A.rrc_boxes(3, 64, 80, sample_offset=(1 << 40) + 2, **kw))
    for other in (dict(kw, step=10), dict(kw, stream=3), dict(kw, seed=4)):
        assert not np.array_equal(a[:, :4], A.rrc_boxes(8, 64, 80, **other)[:, :4])
    assert A.rrc_boxes(0, 64, 80).shape == (0, 5)


def test_rrc_boxes_fallback_and_accept_paths():
    H = 64
    boxes, attempts = A.rrc_boxes(32, H, H, scale=(1, 1), ratio=(2, 2), return_attempts=True)
    assert (attempts == 10).all()  # bw = round(sqrt(2) H) > W every time: the fallback
    assert (boxes[:, :4] == np.array([H // 4, 0, H // 2, H])).all()
    boxes, attempts = A.rrc_boxes(32, H, H, scale=(0.25, 0.25), ratio=(1, 1), return_attempts=True)
    assert (attempts == 0).all()  # accepted at once
    assert (boxes[:, 2] == H // 2).all() and (boxes[:, 3] == H // 2).all()
    # torchvision's other fallbacks: a wide image, and one whose aspect lies inside ratio
    assert A.rrc_boxes(1, 10, 100, scale=(4, 4), ratio=(1, 2))[0, :4].tolist() == [0, 40, 10, 20]
    assert A.rrc_boxes(1, 10, 15, scale=(4, 4), ratio=(1, 2))[0, :4].tolist() == [0, 0, 10, 15]


def test_center_boxes():
    assert A.center_boxes(3, 256, 256, 224).tolist() == [[16, 16, 224, 224, 0]] * 3
    assert A.center_boxes(1, 256, 256, (224, 224)).dtype == np.int32
    assert A.center_boxes(1, 100, 200, 50, crop_pct=1.0).tolist() == [[0, 50, 100, 100, 0]]
    assert A.center_boxes(1, 37, 41, (32, 36), crop_pct=0.5).tolist() == [[9, 10, 18, 20, 0]]
    assert A.center_boxes(1, 2, 2, 224, crop_pct=0.1).tolist() == [[0, 0, 1, 1, 0]]  # never empty
    with pytest.raises(ValueError, match="center_boxes"):
        A.center_boxes(1, 256, 256, 224, crop_pct=0.0)


# ---- errors, each naming the op --------------------------------------------------------------------
def test_argument_errors():
    u = rand_images(2, 9, 11)
    ok = np.array([[0, 0, 9, 11, 0], [1, 2, 3, 4, 1]], dtype=np.int32)
    op = "resized_crop_batch"
    for bad, sample in [((-1, 0, 3, 3, 0), 0), ((0, 0, 10, 3, 0), 0), ((0, 9, 3, 3, 0), 0), ((0, 0, 0, 3, 0), 0),
                        ((0, 0, 3, 0, 0), 1), ((0, 0, 3, 3, 2), 1), ((7, 0, 3, 3, 0), 1)]:
        t = ok.copy()
        t[sample] = bad
        with pytest.raises(ValueError, match=f"{op}: the box of sample {sample}"):
            A.resized_crop_batch(u, t, size=(4, 4))
        with pytest.raises(ValueError, match=f"{op}: the box of sample {sample}"):
            A.resized_crop_batch(u, torch.from_numpy(t), size=(4, 4))
    with pytest.raises(ValueError, match=f"{op}: boxes is an integer table"):
        A.resized_crop_batch(u, ok[:1], size=(4, 4))
    with pytest.raises(ValueError, match=f"{op}: boxes is an integer table"):
        A.resized_crop_batch(u, ok.astype(np.float32), size=(4, 4))
    with pytest.raises(ValueError, match=f"{op}: the sides"):
        A.resized_crop_batch(u, ok, size=(4, 16385))
    with pytest.raises(ValueError, match=f"{op}: the sides"):
        A.resized_crop_batch(torch.zeros(1, 1, 16385, 3, dtype=torch.uint8), ok[:1], size=(4, 4))
    with pytest.raises(ValueError, match=f"{op}: the sides"):
        A.resized_crop_batch(u, ok, size=(0, 4))
    with pytest.raises(TypeError, match=f"{op}: the input is uint8"):
        A.resized_crop_batch(u.float(), ok, size=(4, 4))
    with pytest.raises(TypeError, match=f"{op}: the input is a torch tensor"):
        A.resized_crop_batch(u.numpy(), ok, size=(4, 4))
    with pytest.raises(ValueError, match=f"{op}: the input is \\[B, H, W, 3\\]"):
        A.resized_crop_batch(u[..., :2], ok, size=(4, 4))
    with pytest.raises(TypeError, match=f"{op}: size is"):
        A.resized_crop_batch(u, ok, size=4)
    with pytest.raises(TypeError, match=f"{op}: dtype"):
        A.resized_crop_batch(u, ok, size=(4, 4), dtype=torch.float32)
    with pytest.raises(ValueError, match=f"{op}: channels"):
        A.resized_crop_batch(u, ok, size=(4, 4), channels=5)
    with pytest.raises(ValueError, match=f"{op}: the mix mode"):
        A.resized_crop_batch(u, ok, size=(4, 4), mix=(3, 0.5, (0, 0, 0, 0)))
    with pytest.raises(ValueError, match=f"{op}: the box .* must lie inside the output"):
        A.resized_crop_batch(u, ok, size=(4, 4), mix=(2, 0.5, (0, 0, 5, 4)))
    with pytest.raises(ValueError, match=f"{op}: dev_block"):
        A.resized_crop_batch(u, ok, size=(4, 4), dev_block=torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match=f"{op}: out must be the dense NHWC"):
        A.resized_crop_batch(u, ok, size=(4, 4), out=torch.zeros(2, 4, 4, 4, dtype=torch.bfloat16))
    for kw in (dict(stream=1 << 26), dict(seed=-1), dict(step=1 << 32), dict(scale=(0.0, 1.0)), dict(ratio=(2.0, 1.0))):
        with pytest.raises(ValueError, match="rrc_boxes"):
            A.rrc_boxes(2, 9, 11, **kw)
    with pytest.raises(TypeError, match="rrc_boxes: scale"):
        A.rrc_boxes(2, 9, 11, scale=0.5)
    with pytest.raises(ValueError, match="rrc_boxes"):
        A.rrc_boxes(2, 9, 16385)


def test_out_is_written_on_the_cpu():
    u = rand_images(2, 9, 11)
    t = A.center_boxes(2, 9, 11, (4, 6))
    out = torch.zeros(2, 4, 6, 4, dtype=torch.float16)
    x = A.resized_crop_batch(u, t, size=(4, 6), channels=4, dtype=torch.float16, out=out)
    assert x.data_ptr() == out.data_ptr() and tuple(x.shape) == (2, 4, 4, 6)
    assert torch.equal(bits(x), bits(A.resized_crop_reference(u, t, size=(4, 6), channels=4, dtype=torch.float16)))
    assert not bits(out)[..., 3].any()


# ---- DeviceAugment(crop="resized") -------------------------------------------------------------------
def test_device_augment_resized_on_the_cpu():
    B, H, W, size = 6, 40, 48, (32, 36)
    u = rand_images(B, H, W, seed=8)
    labels = torch.arange(B) % 4
    kw = dict(crop="resized", channels=4, seed=3, mixup_alpha=0.4, cutmix_alpha=1.0, num_classes=4,
              label_smoothing=0.1, scale=(0.3, 1.0), ratio=(0.5, 2.0))
    aug = FluxMPI.DeviceAugment(size, **kw)
    seen = []
    for step in range(3):
        x, y = aug(u, labels)
        mix = aug.draw(step)
        boxes = A.rrc_boxes(B, H, W, scale=(0.3, 1.0), ratio=(0.5, 2.0), seed=3, step=step)
        assert tuple(x.shape) == (B, 4, *size) and x.dtype == torch.bfloat16 and tuple(y.shape) == (B, 4)
        assert torch.equal(bits(x), bits(A.resized_crop_reference(u, boxes, size=size, channels=4, mix=mix)))
        assert torch.equal(y, A.mix_targets(labels, 4, mix.lam, 0.1))
        seen.append(bits(x).clone())
    assert not torch.equal(seen[0], seen[1]) and aug.state_dict() == {"seed": 3, "step": 3}
    # the offset names the samples: the second half of the batch alone draws the same boxes
    plain = FluxMPI.DeviceAugment(size, crop="resized", seed=3)
    whole, _ = plain(u, step=5)
    half, _ = plain(u[3:], step=5, sample_offset=3)
    assert torch.equal(bits(whole[3:]), bits(half))
    # a state round trip replays the step
    other = FluxMPI.DeviceAugment(size, **kw)
    other.load_state_dict({"seed": 3, "step": 1})
    x1, y1 = other(u, labels)
    assert torch.equal(bits(x1), seen[1])
    # labels targets
    lab = FluxMPI.DeviceAugment(size, **dict(kw, targets="labels", num_classes=None))
    _, ym = lab(u, labels, step=0)
    assert ym.labels is labels and ym.lam == aug.draw(0).lam
    # eval: Resize + CenterCrop, no flip, no mix, no step
    e0, l0 = aug.eval()(u, labels)
    e1, _ = aug(u, labels)
    assert l0 is labels and aug.step == 3 and torch.equal(bits(e0), bits(e1))
    assert torch.equal(bits(e0), bits(A.resized_crop_reference(u, A.center_boxes(B, H, W, size), size=size, channels=4)))
    with pytest.raises(ValueError, match="DeviceAugment: use_block"):
        aug(u, labels, use_block=True)
    with pytest.raises(ValueError, match="DeviceAugment: use_block needs GPU"):
        aug.train()(u, labels, use_block=True)


def test_device_augment_eval_at_the_stored_scale_is_the_centre_crop():
    u = rand_images(2, 256, 256, seed=1)
    a, _ = FluxMPI.DeviceAugment(224, crop="resized", channels=4).eval()(u)
    b, _ = FluxMPI.DeviceAugment(224, crop="pad", channels=4).eval()(u)
    assert torch.equal(bits(a), bits(b))


def test_device_augment_errors_and_the_default():
    with pytest.raises(ValueError, match="DeviceAugment: crop is"):
        FluxMPI.DeviceAugment(32, crop="random")
    with pytest.raises(ValueError, match="DeviceAugment: with crop='resized'"):
        FluxMPI.DeviceAugment(32, crop="resized", pad=4)
    with pytest.raises(ValueError, match="DeviceAugment: with crop='resized'"):
        FluxMPI.DeviceAugment(32, crop="resized", fill=1)
    with pytest.raises(ValueError, match="DeviceAugment: scale"):
        FluxMPI.DeviceAugment(32, crop="resized", scale=(1.0, 0.5))
    with pytest.raises(TypeError, match="DeviceAugment: ratio"):
        FluxMPI.DeviceAugment(32, crop="resized", ratio=1.0)
    with pytest.raises(ValueError, match="DeviceAugment: crop_pct"):
        FluxMPI.DeviceAugment(32, crop="resized", crop_pct=1.5)
    with pytest.raises(ValueError, match="DeviceAugment: with crop='resized' prepare needs batch"):
        FluxMPI.DeviceAugment(32, crop="resized").prepare(0, device="cpu")
    # crop="pad" is the default and is what it was
    u = rand_images(5, 37, 41)
    for kw in (dict(), dict(crop="pad")):
        aug = FluxMPI.DeviceAugment((32, 36), pad=4, fill=7, mixup_alpha=0.3, num_classes=5, seed=2, **kw)
        x, _ = aug(u, torch.arange(5))
        want = A.augment_reference(u, size=(32, 36), pad=4, fill=7, seed=2, step=0, mix=aug.draw(0))
        assert aug.crop == "pad" and torch.equal(bits(x), bits(want))
