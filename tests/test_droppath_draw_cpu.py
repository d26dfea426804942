"""The drop-path draw, checked without a GPU: maeclip_droppath_scales_host runs
the very function the two kernels run (droppath.hip dp_scale) on the CPU, and
scales_ref below restates include/maeclip.h "Stochastic depth" in numpy on
oracle.maskrng.hash4. No transcendental is involved (a 24-bit integer times
2^-24, one fp32 compare, one fp32 division), so the two are exactly equal."""
import numpy as np
import pytest
import torch

from oracle.maskrng import hash4

SEED = 1234 * 1000003 + 43
STEP_MULT = 0x9E3779B97F4A7C15
FIELD = 32
M64 = (1 << 64) - 1


def scales_ref(B, k, p, seed=SEED, step=0, sample_offset=0):
    step_seed = (seed + step * STEP_MULT) & M64
    b = np.arange(B, dtype=np.uint64) + np.uint64(sample_offset)
    u = (hash4(np.uint64(step_seed), b, np.uint64(k), np.uint64(FIELD)) >> np.uint32(8)).astype(np.float32) \
        * np.float32(2.0 ** -24)
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(u >= np.float32(p), inv, np.float32(0.0)).astype(np.float32)


def host(B, k, p, seed=SEED, step=0, sample_offset=0):
    from mae_clip_amd import kernels as K
    return K.droppath_scales_host(B, k, p, seed=seed, step=step, sample_offset=sample_offset).numpy()


@pytest.mark.parametrize("step", [0, 1, 7])
@pytest.mark.parametrize("offset", [0, 5])
@pytest.mark.parametrize("B", [1, 5, 8])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_host_equals_restatement(step, offset, B, p):
    for k in (0, 1, 23):
        got = host(B, k, p, step=step, sample_offset=offset)
        ref = scales_ref(B, k, p, step=step, sample_offset=offset)
        assert got.dtype == np.float32 and got.shape == (B,)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (step, offset, B, p, k, got, ref)
    # several keys in one call: the rows are the single-key draws
    many = host(B, [0, 1, 23], p, step=step, sample_offset=offset)
    assert many.shape == (3, B)
    for i, k in enumerate((0, 1, 23)):
        assert np.array_equal(many[i], host(B, k, p, step=step, sample_offset=offset))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_offset_is_a_window_of_the_whole_batch(p):
    """a rank / micro-batch that starts at sample 5 draws what one whole-batch launch would"""
    for k in (0, 1, 23):
        for step in (0, 7):
            whole = host(8, k, p, step=step)
            assert np.array_equal(host(3, k, p, step=step, sample_offset=5), whole[5:8])


def test_masks_differ_between_steps_and_keys():
    B, p = 256, 0.5
    base = host(B, 0, p, step=0)
    assert not np.array_equal(base, host(B, 0, p, step=1))
    assert not np.array_equal(base, host(B, 1, p, step=0))
    assert not np.array_equal(host(B, 2, p, step=3), host(B, 3, p, step=3))      # the two branches of block 1
    assert not np.array_equal(base, host(B, 0, p, step=0, seed=SEED + 1))
    assert np.array_equal(base, host(B, 0, p, step=0))


def test_rate_zero_keeps_everything_at_scale_one():
    for step in (0, 7):
        s = host(64, 5, 0.0, step=step)
        assert np.array_equal(s, np.ones(64, dtype=np.float32))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_share(p):
    """N Bernoulli(1 - p) draws: the kept share is within 4 standard deviations of 1 - p"""
    N = 20000
    s = host(N, 3, p, step=2)
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    kept = s != 0
    assert np.all(s[kept] == inv)
    share = kept.mean()
    print(f"kept share at p = {p}: {share:.5f}")
    assert abs(share - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / N), share


def test_per_block_rates_follow_timm():
    from mae_clip_amd.modules import drop_path_rates
    assert drop_path_rates(0.1, 12) == [float(v) for v in torch.linspace(0, 0.1, 12)]
    assert drop_path_rates(0.1, 12)[0] == 0.0 and drop_path_rates(0.1, 12)[-1] == float(torch.tensor(0.1))
    assert drop_path_rates(0.3, 1) == [0.0]
    assert drop_path_rates(0.0, 3) == [0.0, 0.0, 0.0]
