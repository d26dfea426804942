"""CPU restatement of the device-side Mixup / CutMix (test infrastructure
only): timm's Mixup(correct_lam=True) with partner = B-1-b.

mix_params_ref is the draw of maeclip_mix_params in numpy float64. It follows
the order of operations written at maeclip_mix_params in include/maeclip.h
line by line, with oracle.maskrng.hash4 as the counter hash. log / exp / cos
here may differ from the library's in the last bit: the lams then agree to a
few ulp, and a box can move only where H sqrt(1 - lam) or W sqrt(1 - lam) lies
on an integer to ~1e-13; the draw therefore also reports, per sample, whether
one of them (or u H, u W, which are exact) came within 1e-6 of an integer
(`near_tie`), and the tests leave those samples' boxes out.

mix_images_ref / mix_targets_ref are the pixel and target kernels in numpy
float32, one rounding per operation as the header writes them.
"""
import numpy as np

from oracle.maskrng import hash4

STEP_MULT = 0x9E3779B97F4A7C15
BATCH_KEY = 0x4D49584261746368
TIE_EPS = 1e-6
TRIES = 16
NONE, MIXUP, CUTMIX = 0, 1, 2
F_MIX, F_SWITCH, F_N1, F_N2, F_ACC, F_BOOST, F_CY, F_CX = range(16, 24)


def step_seed(seed, step):
    return np.uint64((int(seed) + int(step) * STEP_MULT) & 0xFFFFFFFFFFFFFFFF)


def _h24(sseed, key, k, f):
    return int(hash4(sseed, np.uint64(key), np.uint64(k), np.uint64(f)) >> np.uint32(8))


def _u(sseed, key, k, f):
    return np.float64(_h24(sseed, key, k, f)) * 2.0 ** -24


def _uo(sseed, key, k, f):
    return np.float64(_h24(sseed, key, k, f) + 1) * 2.0 ** -24


def _gamma(sseed, key, a, g):
    a1 = a + 1.0 if a < 1.0 else a
    d = a1 - np.float64(1.0) / np.float64(3.0)
    c = 1.0 / np.sqrt(9.0 * d)
    G = d
    for t in range(TRIES):
        k = TRIES * g + t
        x = np.sqrt(-2.0 * np.log(_uo(sseed, key, k, F_N1))) * np.cos(6.283185307179586 * _u(sseed, key, k, F_N2))
        t1 = 1.0 + c * x
        if t1 <= 0.0:
            continue
        v = (t1 * t1) * t1
        rhs = (((0.5 * x) * x + d) - d * v) + d * np.log(v)
        if np.log(_uo(sseed, key, k, F_ACC)) < rhs:
            G = d * v
            break
    if a < 1.0:
        G = G * np.exp(np.log(_uo(sseed, key, TRIES * g, F_BOOST)) / a)
    return G


def _near_int(x):
    return abs(x - np.rint(x)) < TIE_EPS


def _clip(v, lo, hi):
    return min(max(v, lo), hi)


def _draw(sseed, key, H, W, mixup_alpha, cutmix_alpha, prob, switch_prob):
    """-> (kind, x0, y0, x1, y1, lam_pixel f32, lam_target f32, near_tie)"""
    none = (NONE, 0, 0, 0, 0, np.float32(1), np.float32(1), False)
    if not _u(sseed, key, 0, F_MIX) < prob:
        return none
    if mixup_alpha > 0 and cutmix_alpha > 0:
        cutmix = bool(_u(sseed, key, 0, F_SWITCH) < switch_prob)
        alpha = cutmix_alpha if cutmix else mixup_alpha
    elif mixup_alpha > 0:
        cutmix, alpha = False, mixup_alpha
    elif cutmix_alpha > 0:
        cutmix, alpha = True, cutmix_alpha
    else:
        return none
    if alpha == 1.0:
        lam = _u(sseed, key, 0, F_N1)
    else:
        X, Y = _gamma(sseed, key, alpha, 0), _gamma(sseed, key, alpha, 1)
        lam = X / (X + Y)
    if not cutmix:
        return (MIXUP, 0, 0, 0, 0, np.float32(lam), np.float32(lam), False)
    r = np.sqrt(1.0 - lam)
    hr, wr = np.float64(H) * r, np.float64(W) * r
    ch, cw = int(hr), int(wr)
    fy, fx = _u(sseed, key, 0, F_CY) * np.float64(H), _u(sseed, key, 0, F_CX) * np.float64(W)
    cy, cx = int(np.floor(fy)), int(np.floor(fx))
    near = bool(_near_int(hr) or _near_int(wr) or _near_int(fy) or _near_int(fx))
    y0, y1 = _clip(cy - ch // 2, 0, H), _clip(cy + ch // 2, 0, H)
    x0, x1 = _clip(cx - cw // 2, 0, W), _clip(cx + cw // 2, 0, W)
    lam_t = np.float32(1.0 - np.float64((x1 - x0) * (y1 - y0)) / (np.float64(H) * np.float64(W)))
    return (CUTMIX, x0, y0, x1, y1, np.float32(1), lam_t, near)


def mix_params_ref(B, H, W, mixup_alpha, cutmix_alpha, prob, switch_prob, mode, seed, step=0, sample_offset=0):
    """-> (records int32 [B, 8] as the library lays them out, near_tie bool [B]).
    mode: 0 batch, 1 elem. The alphas and probabilities cross the ABI as fp32."""
    ma, ca, pr, sp = (np.float64(np.float32(v)) for v in (mixup_alpha, cutmix_alpha, prob, switch_prob))
    sseed = step_seed(seed, step)
    rec = np.zeros((B, 8), dtype=np.int32)
    near = np.zeros(B, dtype=bool)
    shared = _draw(sseed, BATCH_KEY, H, W, ma, ca, pr, sp) if mode == 0 else None
    for b in range(B):
        d = shared if mode == 0 else _draw(sseed, (int(sample_offset) + b) & 0xFFFFFFFFFFFFFFFF, H, W, ma, ca, pr, sp)
        rec[b, 0], rec[b, 1] = d[0], B - 1 - b
        rec[b, 2:6] = d[1:5]
        rec[b, 6:8] = np.asarray(d[5:7], dtype=np.float32).view(np.int32)
        near[b] = d[7]
    return rec, near


def make_records(rows):
    """rows of (kind, partner, x0, y0, x1, y1, lam_pixel, lam_target) -> int32 [B, 8]"""
    rec = np.zeros((len(rows), 8), dtype=np.int32)
    for b, r in enumerate(rows):
        rec[b, :6] = r[:6]
        rec[b, 6:8] = np.asarray(r[6:8], dtype=np.float32).view(np.int32)
    return rec


def lams(rec):
    """(lam_pixel, lam_target) float32 [B] of int32 [B, 8] records"""
    f = np.ascontiguousarray(np.asarray(rec)[:, 6:8]).view(np.float32)
    return f[:, 0], f[:, 1]


def mix_images_ref(images, rec):
    """images: uint8 [B, S, S, 3] or float32 [B, 3, S, S] -> the mixed batch, as
    maeclip_mix_images writes it (partner and box clamped)."""
    images = np.asarray(images)
    u8 = images.dtype == np.uint8
    B, S = images.shape[0], images.shape[2]
    lam_p, _ = lams(rec)
    out = images.copy()
    for b in range(B):
        kind, partner, x0, y0, x1, y1 = (int(v) for v in rec[b, :6])
        p = images[_clip(partner, 0, B - 1)]
        if kind == CUTMIX:
            x0, x1, y0, y1 = (_clip(v, 0, S) for v in (x0, x1, y0, y1))
            if x1 > x0 and y1 > y0:
                if u8:
                    out[b, y0:y1, x0:x1, :] = p[y0:y1, x0:x1, :]
                else:
                    out[b, :, y0:y1, x0:x1] = p[:, y0:y1, x0:x1]
        elif kind == MIXUP:
            lam = np.float32(lam_p[b])
            oml = np.float32(1) - lam
            with np.errstate(all="ignore"):
                v = (lam * images[b].astype(np.float32)).astype(np.float32) + (oml * p.astype(np.float32)).astype(np.float32)
            v = v.astype(np.float32)
            if u8:
                v = np.rint(v)                                   # ties to even
                v = np.where(np.isnan(v), np.float32(0), np.clip(v, 0, 255))
                out[b] = v.astype(np.uint8)
            else:
                out[b] = v
    return out


def mix_targets_ref(labels, rec, C, ld_t=None):
    """float32 [B, ld_t] (ld_t = C when None), columns >= C zero"""
    labels = np.asarray(labels).astype(np.int64)
    B = labels.shape[0]
    ld_t = C if ld_t is None else ld_t
    _, lam_t = lams(rec)
    t = np.zeros((B, ld_t), dtype=np.float32)
    for b in range(B):
        ya, yp = int(labels[b]), int(labels[_clip(int(rec[b, 1]), 0, B - 1)])
        lam = np.float32(lam_t[b])
        if ya == yp:
            if 0 <= ya < C:
                t[b, ya] = 1
            continue
        if 0 <= ya < C:
            t[b, ya] = lam
        if 0 <= yp < C:
            t[b, yp] = np.float32(1) - lam
    return t
