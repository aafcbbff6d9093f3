"""The shape gate of the one-pass conv3 -> bn3 backward (``fused_block.conv3bn3_admits``, the part of
``conv3bn3_ok`` that depends on the filter, the pixel count, the device's compute units and the
``FLUXMPI_CONV3BN3`` switch). No GPU: the gate is plain arithmetic.

The 128 -> 512 blocks of a small input must keep the unfused launches (tests/golden/resnet_launch_trace.json
records them at a few hundred pixels); the 64 -> 256 path is as it was at every size."""
import os

import pytest

S1, S2 = (256, 64, 1, 1), (512, 128, 1, 1)


@pytest.fixture
def fb():
    from fluxmpi_amd.ops import fused_block
    return fused_block


def test_default_is_both_stages(fb):
    assert fb.CONV3BN3 == int(os.environ.get("FLUXMPI_CONV3BN3", "2"))
    assert "FLUXMPI_CONV3BN3" in os.environ or fb.CONV3BN3 == 2


@pytest.mark.parametrize("cus", [1, 104, 256, 304])
def test_stage2_needs_64_pixels_per_compute_unit(fb, monkeypatch, cus):
    monkeypatch.setattr(fb, "CONV3BN3", 2)
    for pixels in (1, 49, 392, 64 * cus - 1):
        assert fb.conv3bn3_admits(S2, pixels, cus) is (pixels >= 64 * cus), pixels
    assert not fb.conv3bn3_admits(S2, 64 * cus - 1, cus)
    for pixels in (64 * cus, 64 * cus + 1, 256 * 28 * 28 + 64 * cus):
        assert fb.conv3bn3_admits(S2, pixels, cus), pixels


@pytest.mark.parametrize("switch", [1, 2, True])
def test_stage1_at_every_size(fb, monkeypatch, switch):
    monkeypatch.setattr(fb, "CONV3BN3", switch)
    for pixels in (1, 49, 392, 6272, 256 * 56 * 56):
        for cus in (1, 256, 304):
            assert fb.conv3bn3_admits(S1, pixels, cus)


def test_switch_values(fb, monkeypatch):
    big = 256 * 28 * 28
    for switch, s1, s2 in ((0, False, False), (False, False, False), (1, True, False), (True, True, False),
                           (2, True, True)):
        monkeypatch.setattr(fb, "CONV3BN3", switch)
        assert fb.conv3bn3_admits(S1, big, 256) is s1, switch
        assert fb.conv3bn3_admits(S2, big, 256) is s2, switch


def test_other_filters_are_refused(fb, monkeypatch):
    monkeypatch.setattr(fb, "CONV3BN3", 2)
    for shape in ((1024, 256, 1, 1), (2048, 512, 1, 1), (512, 128, 3, 3), (256, 128, 1, 1), (512, 64, 1, 1)):
        assert not fb.conv3bn3_admits(shape, 1 << 20, 256), shape


def test_slab_count_is_one_per_compute_unit(fb, monkeypatch):
    """``conv3bn3_slabs`` for the 512-channel form: one workgroup per compute unit, never more than tiles."""
    import torch

    class _Props:
        multi_processor_count = 256

    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda d: _Props())
    assert fb.conv3bn3_slabs(256 * 28 * 28, "cuda", 512) == 256
    assert fb.conv3bn3_slabs(392, "cuda", 512) == 13
    assert fb.conv3bn3_slabs(1, "cuda", 512) == 1
    assert fb.conv3bn3_slabs(256 * 56 * 56, "cuda") == 512
    assert fb.conv3bn3_slabs(256 * 56 * 56, "cuda", 256) == 512
