"""The Mixup / CutMix draw, checked without a GPU: maeclip_mix_params_host runs
the very function the device kernel runs (mix.hip mc_mix_draw) on the CPU, and
tests/mix_ref.py restates it in numpy float64.

Against the restatement: kind and partner are equal; both lams agree to 1e-6
relative (log / exp / cos of the C library and numpy's may differ in the last
bit); boxes are equal except where the restatement flags a near tie (H sqrt(1 -
lam), W sqrt(1 - lam), u H or u W within 1e-6 of an integer), and those are
capped at 1 % of the samples. Expected share: ~4e-6 per value for a smooth lam
density. A cutmix alpha of 0.2 piles lam up at 0: lam < 9e-9 puts 224 sqrt(1 -
lam) within 1e-6 of 224 (the box is the whole image on both sides), which is
~1 % of Beta(0.2, 0.2) (measured: 41 of 4000), so that alpha is a quarter of
the configurations below and no more.

Distribution: 20000 lams per alpha in elem mode against
numpy.random.default_rng(0).beta(alpha, alpha, 200000), two-sample
Kolmogorov-Smirnov at the 0.001 critical value 1.949 sqrt((n + m) / (n m)) =
0.01445. A record carries lam as float32, so the reference sample is rounded to
float32 as well, the same numbers in the record's format: of Beta(0.2, 0.2),
1.6 % lies within 2^-25 of 1 and is exactly 1.0f in ANY float32 record (of the
numpy sample: 1.648 %), which alone is a KS distance of 0.016 to the unrounded
sample. Measured at seed 4 (alpha: D against the float32 sample / against the
float64 sample): 0.2: 0.0048 / 0.0161, 0.8: 0.0050, 1.0: 0.0055, 2.0: 0.0041
(rounding changes nothing there). Both are printed.
"""
import numpy as np
import pytest

from oracle.maskrng import hash4
from tests.mix_ref import CUTMIX, MIXUP, NONE, lams, mix_params_ref, step_seed

SEED = 4
STEPS = [0, 1, 7]
OFFSETS = [0, 5]
BS = [1, 5, 8]
ALPHAS = [(0.8, 1.0), (0.2, 0.4), (2.0, 0.0), (0.0, 0.2)]      # (mixup, cutmix); both samplers, boost and no boost
SIZES = [(224, 224), (37, 200)]                                # (H, W)
PROB, SWITCH = 0.9, 0.5
N = 20000


def host(B, H=224, W=224, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode=1, seed=SEED, step=0,
         sample_offset=0):
    from mae_clip_amd import data
    return data.mix_params_host(B, H, W, mixup_alpha, cutmix_alpha, prob, switch_prob, mode, seed, step,
                                sample_offset).numpy()


def check_against(got, ref, near, what):
    """the comparison rule of this file (and of the device test): -> excluded samples"""
    assert np.array_equal(got[:, :2], ref[:, :2]), (what, "kind / partner")
    for g, r, name in zip(lams(got), lams(ref), ("lam_pixel", "lam_target")):
        keep = ~near if name == "lam_target" else np.ones_like(near)      # a cutmix lam_target follows its box
        assert np.all(np.abs(g[keep].astype(np.float64) - r[keep]) <= 1e-6 * np.abs(r[keep].astype(np.float64))), (what, name)
    keep = ~near
    assert np.array_equal(got[keep, 2:6], ref[keep, 2:6]), (what, "box")
    return int(near.sum())


@pytest.fixture(scope="module")
def draws():
    """every (alphas, size, mode, step, offset, B) once: (library records, restated records, near_tie)"""
    out = {}
    for al in ALPHAS:
        for hw in SIZES:
            for mode in (0, 1):
                for step in STEPS:
                    for off in OFFSETS:
                        for B in BS:
                            ref, near = mix_params_ref(B, hw[0], hw[1], al[0], al[1], PROB, SWITCH, mode, SEED, step, off)
                            got = host(B, hw[0], hw[1], al[0], al[1], PROB, SWITCH, mode, SEED, step, off)
                            out[al, hw, mode, step, off, B] = (got, ref, near)
    return out


def test_records_match_the_restatement(draws):
    excluded = total = 0
    kinds = set()
    for key, (got, ref, near) in draws.items():
        excluded += check_against(got, ref, near, key)
        total += near.size
        kinds |= set(got[:, 0].tolist())
    print(f"near-tie samples excluded: {excluded} of {total}")
    assert kinds == {NONE, MIXUP, CUTMIX}
    assert excluded <= 0.01 * total, (excluded, total)


def test_near_tie_share_of_the_restatement_alone():
    """the 1 % cap on a larger sample of the restatement alone, at the recipe's alphas"""
    _, near = mix_params_ref(4000, 224, 224, 0.8, 1.0, 1.0, 0.5, 1, SEED, 0, 0)
    print(f"near ties at alphas (0.8, 1.0): {int(near.sum())} of {near.size}")
    assert near.sum() <= 0.01 * near.size


def _ks(a, b):
    a, b = np.sort(a), np.sort(b)
    allv = np.concatenate([a, b])
    return np.abs(np.searchsorted(a, allv, side="right") / a.size - np.searchsorted(b, allv, side="right") / b.size).max()


@pytest.mark.parametrize("alpha", [0.2, 0.8, 1.0, 2.0])
def test_lam_is_beta_distributed(alpha):
    rec = host(N, mixup_alpha=alpha, cutmix_alpha=0.0)
    assert (rec[:, 0] == MIXUP).all() and np.array_equal(rec[:, 6], rec[:, 7])
    lam = lams(rec)[0]
    assert ((lam >= 0) & (lam <= 1)).all()
    ref = np.random.default_rng(0).beta(alpha, alpha, 200000)
    n, m = lam.size, ref.size
    crit = 1.949 * np.sqrt((n + m) / (n * m))
    d32, d64 = _ks(lam, ref.astype(np.float32)), _ks(lam.astype(np.float64), ref)
    z = (lam.astype(np.float64).mean() - 0.5) / np.sqrt(1.0 / (4 * (2 * alpha + 1)) / n)
    print(f"alpha {alpha}: KS D {d32:.5f} (float32 sample) / {d64:.5f} (float64 sample), critical {crit:.5f}; mean z {z:+.2f}")
    assert d32 < crit, (alpha, d32, crit)
    assert abs(z) < 4, (alpha, z)


def test_alpha_one_is_the_plain_uniform():
    rec = host(512, mixup_alpha=1.0, cutmix_alpha=0.0, step=3, sample_offset=9)
    gb = np.arange(512, dtype=np.uint64) + np.uint64(9)
    u = (hash4(step_seed(SEED, 3), gb, np.uint64(0), np.uint64(18)) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    assert np.array_equal(lams(rec)[0], u.astype(np.float32))


def test_switch_and_mix_shares():
    rec = host(N)
    z = ((rec[:, 0] == CUTMIX).mean() - 0.5) / np.sqrt(0.25 / N)
    assert set(rec[:, 0].tolist()) == {MIXUP, CUTMIX} and abs(z) < 4, z
    rec = host(N, prob=0.3)
    z = ((rec[:, 0] != NONE).mean() - 0.3) / np.sqrt(0.3 * 0.7 / N)
    assert abs(z) < 4, z
    none = rec[rec[:, 0] == NONE]
    assert (none[:, 2:6] == 0).all() and (lams(none)[0] == 1).all() and (lams(none)[1] == 1).all()
    assert (host(64, prob=0.0)[:, 0] == NONE).all()
    assert (host(64, mixup_alpha=0.0, cutmix_alpha=0.0)[:, 0] == NONE).all()
    assert (host(64, switch_prob=0.0)[:, 0] == MIXUP).all() and (host(64, switch_prob=1.0)[:, 0] == CUTMIX).all()
    assert (host(64, mixup_alpha=0.0)[:, 0] == CUTMIX).all() and (host(64, cutmix_alpha=0.0)[:, 0] == MIXUP).all()


@pytest.mark.parametrize("hw", SIZES + [(1, 1)])
@pytest.mark.parametrize("alpha", [1.0, 0.2])
def test_cutmix_invariants(hw, alpha):
    H, W = hw
    rec = host(4096, H, W, mixup_alpha=0.0, cutmix_alpha=alpha)
    assert (rec[:, 0] == CUTMIX).all() and np.array_equal(rec[:, 1], 4095 - np.arange(4096))
    x0, y0, x1, y1 = (rec[:, i].astype(np.int64) for i in range(2, 6))
    assert ((0 <= x0) & (x0 <= x1) & (x1 <= W)).all() and ((0 <= y0) & (y0 <= y1) & (y1 <= H)).all()
    lam_p, lam_t = lams(rec)
    assert (lam_p == 1).all()
    assert np.array_equal(lam_t, (1.0 - ((x1 - x0) * (y1 - y0)).astype(np.float64) / np.float64(H * W)).astype(np.float32))
    if H > 1:
        assert len({tuple(r) for r in rec[:, 2:6].tolist()}) > 1000


def test_batch_mode_draws_once_and_steps_differ():
    for step in STEPS:
        rec = host(64, mode=0, step=step, sample_offset=0)
        cols = [0, 2, 3, 4, 5, 6, 7]                        # everything but the partner
        assert (rec[:, cols] == rec[0, cols]).all(), step
        assert np.array_equal(rec[:, 1], 63 - np.arange(64))
        # the same draw on every data-parallel rank
        assert np.array_equal(rec, host(64, mode=0, step=step, sample_offset=640))
    seen = {tuple(host(1, mode=0, step=s)[0, [0, 2, 3, 4, 5, 6, 7]].tolist()) for s in range(16)}
    assert len(seen) == 16


def test_step_seed_and_offset_key_the_elem_draw():
    base = host(256)
    assert np.array_equal(base, host(256))
    cols = [0, 2, 3, 4, 5, 6, 7]
    for other in (host(256, step=1), host(256, seed=SEED + 1), host(256, sample_offset=256)):
        assert (other[:, cols] != base[:, cols]).any(1).mean() > 0.9
    # rank r of a data-parallel run draws samples r B .. r B + B - 1 of the global batch
    both = host(512)
    assert np.array_equal(both[:256, cols], base[:, cols])
    assert np.array_equal(both[256:, cols], host(256, sample_offset=256)[:, cols])


def test_independent_of_the_crop_draw_at_equal_seed():
    """alpha = 1 shows the draw's uniform itself: it is none of the crop draw's (fields 0 .. 4)"""
    lam = lams(host(4096, mixup_alpha=1.0, cutmix_alpha=0.0, seed=3))[0].astype(np.float64)
    gb = np.arange(4096, dtype=np.uint64)
    for k, f in ((0, 0), (0, 1), (0, 2), (0, 3), (10, 4)):
        u = (hash4(step_seed(3, 0), gb, np.uint64(k), np.uint64(f)) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        assert (u == lam).mean() < 0.01, (k, f)
        assert abs(np.corrcoef(u, lam)[0, 1]) < 4 / np.sqrt(4096), (k, f)
