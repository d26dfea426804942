"""The RandomResizedCrop / flip draw, checked without a GPU:
maeclip_crop_params_host runs the very function the device kernel runs
(input.hip mc_crop_draw) on the CPU, and tests/augment_ref.py restates it in
numpy float64. Boxes must agree sample for sample. The one licence: exp / log
of the C library and numpy's may differ in the last bit, which can move a box
only where a pre-rounding w or h lies on a half-integer to ~1e-13; samples
where any examined attempt came within 1e-6 of one are left out, and their
share is capped at 0.1 % (expected: 2 values x ~1.3 attempts x 2e-6 ~ 1e-5 of
the samples; measured over the 30 configurations below: 2 of 122880)."""
import numpy as np
import pytest
import torch

from tests.augment_ref import crop_params_ref

SIZES = [(256, 256), (37, 200), (200, 16), (8, 8), (1, 1)]     # (H, W)
ELONGATED = [(37, 200), (200, 16)]
SCALES = [(0.08, 1.0), (0.9, 1.0)]
STEPS = [0, 1, 2 ** 40]
RATIO = (3 / 4, 4 / 3)
B = 4096
SEED = 3


def host_boxes(sizes, scale=SCALES[0], ratio=RATIO, flip_p=0.5, seed=SEED, step=0, sample_offset=0):
    from mae_clip_amd import data
    return data.crop_params_host(torch.as_tensor(np.asarray(sizes), dtype=torch.int32), scale, ratio, flip_p, seed,
                                 step, sample_offset).numpy()


def _sizes(hw, n=B):
    return np.tile(np.asarray(hw, dtype=np.int32), (n, 1))


@pytest.fixture(scope="module")
def draws():
    """(size, scale, step) -> (library boxes, restated boxes, near_tie, fallback), computed once"""
    out = {}
    for hw in SIZES:
        for scale in SCALES:
            for step in STEPS:
                ref, near, fb = crop_params_ref(_sizes(hw), scale, RATIO, 0.5, SEED, step, 0)
                out[hw, scale, step] = (host_boxes(_sizes(hw), scale, step=step), ref, near, fb)
    return out


def test_boxes_match_the_restatement(draws):
    excluded = total = 0
    for key, (got, ref, near, _) in draws.items():
        keep = ~near
        assert np.array_equal(got[keep], ref[keep]), (key, np.nonzero((got != ref).any(1) & keep)[0][:8])
        excluded += int(near.sum())
        total += near.size
    print(f"near-tie samples excluded: {excluded} of {total}")
    assert excluded <= 1e-3 * total, (excluded, total)


def test_flip_matches_exactly(draws):
    """the coin has no rounding in it: no sample is excused"""
    for key, (got, ref, _, _) in draws.items():
        assert np.array_equal(got[:, 4], ref[:, 4]), key
        assert 0.4 < got[:, 4].mean() < 0.6, key


def test_every_box_lies_inside_its_image(draws):
    for (hw, _, _), (got, _, _, _) in draws.items():
        H, W = hw
        x0, y0, w, h = got[:, 0], got[:, 1], got[:, 2], got[:, 3]
        assert (x0 >= 0).all() and (y0 >= 0).all() and (w >= 1).all() and (h >= 1).all(), hw
        assert (x0 + w <= W).all() and (y0 + h <= H).all(), hw


@pytest.mark.parametrize("hw", ELONGATED)
def test_elongated_images_reach_the_centre_crop(draws, hw):
    H, W = hw
    for scale in SCALES:
        got, ref, near, fb = draws[hw, scale, 0]
        assert fb.any(), (hw, scale)
        g = got[fb & ~near]
        # ratio-clamped, centred: the long side is cut to the nearest allowed ratio
        if W > H:
            assert (g[:, 3] == H).all() and (g[:, 2] == np.rint(H * np.float64(np.float32(4 / 3)))).all()
        else:
            assert (g[:, 2] == W).all() and (g[:, 3] == np.rint(W / np.float64(np.float32(3 / 4)))).all()
        assert (g[:, 0] == (W - g[:, 2]) // 2).all() and (g[:, 1] == (H - g[:, 3]) // 2).all()


def test_mixed_sizes_in_one_call():
    """per-sample sizes: each sample is drawn for its own image"""
    sizes = np.asarray([SIZES[i % len(SIZES)] for i in range(500)], dtype=np.int32)
    ref, near, _ = crop_params_ref(sizes, SCALES[0], RATIO, 0.5, SEED, 7, 11)
    got = host_boxes(sizes, step=7, sample_offset=11)
    assert np.array_equal(got[~near], ref[~near])


def test_step_and_offset_key_the_draw(draws):
    s = _sizes((256, 256), 256)
    base = host_boxes(s)
    assert np.array_equal(base, host_boxes(s))                                  # same inputs reproduce
    assert np.array_equal(base, draws[(256, 256), SCALES[0], 0][0][:256])       # sample b does not depend on B
    assert (host_boxes(s, step=1) != base).any(1).mean() > 0.9
    assert (host_boxes(s, seed=SEED + 1) != base).any(1).mean() > 0.9
    off = host_boxes(s, sample_offset=256)
    assert (off != base).any(1).mean() > 0.9
    # rank r of a data-parallel run draws samples r*B .. r*B + B - 1 of the global batch
    assert np.array_equal(np.concatenate([base, off]), host_boxes(_sizes((256, 256), 512)))


def test_flip_probability_extremes():
    s = _sizes((64, 48), 512)
    assert (host_boxes(s, flip_p=0.0)[:, 4] == 0).all()
    assert (host_boxes(s, flip_p=1.0)[:, 4] == 1).all()


def test_full_scale_square_ratio_gives_the_whole_image():
    got = host_boxes(_sizes((96, 96), 64), scale=(1.0, 1.0), ratio=(1.0, 1.0))
    assert (got[:, :4] == np.asarray([0, 0, 96, 96])).all()
