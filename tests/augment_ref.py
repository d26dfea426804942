"""CPU restatement of the device-side training augmentation (test
infrastructure only): A.RandomResizedCrop(S, S, scale, ratio, INTER_LINEAR) ->
A.HorizontalFlip(p) -> A.Normalize + permute.

crop_params_ref is the box draw of maeclip_crop_params in numpy float64. It
follows the order of operations written at maeclip_crop_params in
include/maeclip.h line by line, with oracle.maskrng.hash4 as the counter
hash. exp / log here may differ from the library's in the last bit, which can
move a box only where a pre-rounding w or h lies on a half-integer to ~1e-13;
the draw therefore also reports, per sample, whether any attempt it examined
came within 1e-6 of one (`near_tie`), and the tests leave those samples out.

augment_ref is the pixel path: crop, oracle.input_ref's restated cv2.resize,
mirror, normalize.
"""
import numpy as np

from oracle.input_ref import normalize_u8_ref, resize_u8_linear_ref
from oracle.maskrng import hash4

STEP_MULT = 0x9E3779B97F4A7C15
TIE_EPS = 1e-6


def step_seed(seed, step):
    return np.uint64((int(seed) + int(step) * STEP_MULT) & 0xFFFFFFFFFFFFFFFF)


def _u(sseed, gb, k, f):
    return (hash4(sseed, gb, np.uint64(k), np.uint64(f)) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def _near_half(x):
    return np.abs(x - np.floor(x) - 0.5) < TIE_EPS


def crop_params_ref(sizes, scale, ratio, flip_p, seed, step=0, sample_offset=0):
    """sizes int [B, 2] = (h, w) -> (boxes int32 [B, 5] = x0, y0, w, h, flip;
    near_tie bool [B]; fallback bool [B])."""
    sizes = np.asarray(sizes, dtype=np.int64)
    B = sizes.shape[0]
    H, W = sizes[:, 0].astype(np.float64), sizes[:, 1].astype(np.float64)
    s0, s1 = (np.float64(np.float32(v)) for v in scale)          # the ABI carries fp32, widened
    r0, r1 = (np.float64(np.float32(v)) for v in ratio)
    p = np.float64(np.float32(flip_p))
    sseed = step_seed(seed, step)
    gb = np.arange(B, dtype=np.uint64) + np.uint64(sample_offset)
    lr0, lr1 = np.log(r0), np.log(r1)
    hw = H * W
    w, h, x0, y0 = (np.zeros(B, dtype=np.int64) for _ in range(4))
    done = np.zeros(B, dtype=bool)
    near = np.zeros(B, dtype=bool)
    for k in range(10):
        ua, ur = _u(sseed, gb, k, 0), _u(sseed, gb, k, 1)
        area = hw * (s0 + ua * (s1 - s0))
        ar = np.exp(lr0 + ur * (lr1 - lr0))
        wf, hf = np.sqrt(area * ar), np.sqrt(area / ar)
        near |= ~done & (_near_half(wf) | _near_half(hf))
        wd, hd = np.rint(wf), np.rint(hf)
        ok = ~done & (wd > 0) & (wd <= W) & (hd > 0) & (hd <= H)
        uy, ux = _u(sseed, gb, k, 2), _u(sseed, gb, k, 3)
        ys = np.floor(uy * (H - hd + 1))
        xs = np.floor(ux * (W - wd + 1))
        for dst, val in ((w, wd), (h, hd), (y0, ys), (x0, xs)):
            dst[ok] = val[ok].astype(np.int64)
        done |= ok
    fb = ~done
    if fb.any():
        in_ratio = W / H
        hf, wf = W / r0, H * r1
        near |= fb & (((in_ratio < r0) & _near_half(hf)) | ((in_ratio > r1) & _near_half(wf)))
        fh = np.where(in_ratio < r0, np.minimum(np.maximum(np.rint(hf), 1.0), H), H).astype(np.int64)
        fw = np.where((in_ratio >= r0) & (in_ratio > r1), np.minimum(np.maximum(np.rint(wf), 1.0), W), W).astype(np.int64)
        Hi, Wi = sizes[:, 0], sizes[:, 1]
        w[fb], h[fb] = fw[fb], fh[fb]
        y0[fb], x0[fb] = ((Hi - fh) // 2)[fb], ((Wi - fw) // 2)[fb]
    flip = (_u(sseed, gb, 10, 4) < p).astype(np.int64)
    return np.stack([x0, y0, w, h, flip], axis=1).astype(np.int32), near, fb


def clamp_boxes(boxes, sizes):
    """every box clamped into its (h, w) image as maeclip_image_augment_u8 does"""
    b = np.asarray(boxes, dtype=np.int64).copy()
    for i, (H, W) in enumerate(np.asarray(sizes)):
        b[i, 0] = min(max(b[i, 0], 0), W - 1)
        b[i, 1] = min(max(b[i, 1], 0), H - 1)
        b[i, 2] = min(max(b[i, 2], 1), W - b[i, 0])
        b[i, 3] = min(max(b[i, 3], 1), H - b[i, 1])
    return b


def augment_ref(images, boxes, S, **norm):
    """images: list of uint8 HWC arrays; boxes [B, 5] inside their images ->
    (uint8 [B, S, S, 3], float32 [B, 3, S, S] = normalize_u8_ref of it)."""
    out = []
    for im, (x0, y0, w, h, flip) in zip(images, np.asarray(boxes)):
        assert 0 <= x0 and 0 <= y0 and w >= 1 and h >= 1 and x0 + w <= im.shape[1] and y0 + h <= im.shape[0]
        r = resize_u8_linear_ref(np.ascontiguousarray(im[y0:y0 + h, x0:x0 + w]), S)
        out.append(r[:, ::-1] if flip else r)
    u8 = np.ascontiguousarray(np.stack(out))
    return u8, normalize_u8_ref(u8, **norm)
