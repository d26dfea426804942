"""Device-side RandomResizedCrop + flip (input.hip maeclip_crop_params /
maeclip_image_augment_u8, data.TrainAugment, graph.CapturedStep(transform=)).

Pixels are compared bit for bit with tests/augment_ref.py (crop -> restated
cv2.resize -> mirror -> normalize) on hand-written boxes; the draw is compared
with the library's own host evaluation of the same function; the captured step
must feed the model the images the eager step feeds it."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.augment_ref import augment_ref, clamp_boxes, crop_params_ref
from tests.test_augment_draw_cpu import B as DRAW_B, RATIO, SCALES, SEED, SIZES, STEPS, _sizes, host_boxes

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _same(got, ref_np):
    ref = torch.from_numpy(np.ascontiguousarray(ref_np))
    return got.shape == ref.shape and torch.equal(_bits(got), _bits(ref))


def _cases(S):
    """(H, W, box) per sample: every path and edge of the pixel kernel"""
    return [
        (50, 70, (70 - 23, 50 - 17, 23, 17, 0)),          # touches the right and bottom borders
        (40, 40, (5, 6, 1, 20, 1)),                       # w = 1
        (40, 44, (3, 7, 25, 1, 0)),                       # h = 1
        (S + 9, S + 5, (3, 4, S, S, 1)),                  # exactly S x S: copy, mirrored
        (S + 9, S + 5, (5, 9, S, S, 0)),                  # copy
        (2 * S + 3, 2 * S + 6, (2, 1, 2 * S, 2 * S, 0)),  # exactly 2S x 2S: INTER_AREA
        (2 * S + 3, 2 * S + 6, (6, 3, 2 * S, 2 * S, 1)),  # INTER_AREA, mirrored
        (31, 29, (1, 2, 11, 13, 1)),                      # smaller than S: upscales
        (45, 61, (0, 0, 61, 45, 1)),                      # the whole image, not square
        (57, 66, (4, 3, 41, 37, 0)),                      # general downscale
    ]


def _sources(cases, dev, seed):
    """The same images in both source forms, every one a view inside a larger
    allocation of random bytes: a list (the first a row-strided view: rows
    wider than the image) and a padded batch whose slots exceed their images.
    -> (list, batch, sizes tensor, numpy images)"""
    g = torch.Generator().manual_seed(seed)
    Hm = max(c[0] for c in cases) + 5
    Wm = max(c[1] for c in cases) + 7
    batch = torch.randint(0, 256, (len(cases), Hm, Wm, 3), generator=g, dtype=torch.uint8)
    arena = torch.randint(0, 256, (len(cases), Hm + 4, Wm + 6, 3), generator=g, dtype=torch.uint8).to(dev)
    imgs_np, views = [], []
    for i, (H, W, _) in enumerate(cases):
        imgs_np.append(batch[i, :H, :W].numpy().copy())
        v = arena[i, 2:2 + H, 3:3 + W]                    # row stride (Wm + 6) * 3, offset into the allocation
        v.copy_(batch[i, :H, :W])
        assert v.stride(0) != W * 3
        views.append(v)
    sizes = torch.tensor([[c[0], c[1]] for c in cases], dtype=torch.int32, device=dev)
    return views, batch.to(dev), sizes, imgs_np


def _check_both_outputs(src, boxes_dev, S, sizes, ref_u8, ref_f32, what):
    from mae_clip_amd import data
    u8 = data.augment_images(src, boxes_dev, S, torch.uint8, sizes=sizes)
    f32 = data.augment_images(src, boxes_dev, S, torch.float32, sizes=sizes)
    bad = [i for i in range(len(ref_u8)) if not _same(u8[i], ref_u8[i])]
    assert not bad, (what, "uint8 samples differ", bad)
    bad = [i for i in range(len(ref_f32)) if not _same(f32[i], ref_f32[i])]
    assert not bad, (what, "fp32 samples differ", bad)
    assert torch.equal(_bits(f32), _bits(data.normalize_u8(u8))), what


@pytest.mark.parametrize("S", [32, 30])
def test_pixels_bit_exact(dev, S):
    """S = 32: four pixels per thread, vector stores; S = 30: the scalar kernel"""
    cases = _cases(S)
    views, batch, sizes, imgs_np = _sources(cases, dev, seed=S)
    boxes = np.asarray([c[2] for c in cases], dtype=np.int32)
    ref_u8, ref_f32 = augment_ref(imgs_np, boxes, S)
    assert len({tuple(r.ravel()[:64]) for r in ref_u8}) == len(cases)
    bd = torch.from_numpy(boxes).to(dev)
    _check_both_outputs(views, bd, S, None, ref_u8, ref_f32, "descriptor form")
    _check_both_outputs(batch, bd, S, sizes, ref_u8, ref_f32, "padded form with sizes")
    # without sizes every slot is a whole image
    slot_np = [b.cpu().numpy() for b in batch]
    ref_u8, ref_f32 = augment_ref(slot_np, boxes, S)
    _check_both_outputs(batch, bd, S, None, ref_u8, ref_f32, "padded form, whole slots")


def test_unaligned_output_takes_the_scalar_kernel(dev):
    """S % 4 == 0 but the destination is not 16-B / 4-B aligned"""
    from mae_clip_amd import data
    S = 32
    cases = _cases(S)[:4]
    views, _, _, imgs_np = _sources(cases, dev, seed=5)
    boxes = np.asarray([c[2] for c in cases], dtype=np.int32)
    ref_u8, ref_f32 = augment_ref(imgs_np, boxes, S)
    bd = torch.from_numpy(boxes).to(dev)
    raw = torch.zeros(len(cases) * S * S * 3 + 1, dtype=torch.uint8, device=dev)
    out = raw[1:].view(len(cases), S, S, 3)
    assert out.data_ptr() % 4 == 1
    assert _same(data.augment_images(views, bd, S, torch.uint8, out=out), ref_u8)
    rawf = torch.zeros(len(cases) * 3 * S * S + 1, dtype=torch.float32, device=dev)
    outf = rawf[1:].view(len(cases), 3, S, S)
    assert outf.data_ptr() % 16 == 4
    assert _same(data.augment_images(views, bd, S, torch.float32, out=outf), ref_f32)


@pytest.mark.parametrize("S", [32, 30])
def test_boxes_are_clamped_into_their_images(dev, S):
    """Boxes that overrun their image by a few pixels equal the reference on
    the clamped box. Every image is a view inside a larger allocation of other
    random bytes, so a kernel that did not clamp would read those (mapped)
    bytes and differ."""
    hw = [(50, 70), (40, 44), (31, 29), (2 * S + 3, 2 * S + 6), (S + 2, S + 2), (45, 61)]
    over = [(70 - 10, 50 - 8, 20, 20, 0), (-3, -2, 15, 15, 1), (29 + 5, 2, 4, 4, 0),
            (9, 6, 2 * S, 2 * S, 1), (1, 1, S + 6, S + 6, 0), (10, 40, 0, 9, 1)]
    cases = [(h, w, b) for (h, w), b in zip(hw, over)]
    views, batch, sizes, imgs_np = _sources(cases, dev, seed=100 + S)
    boxes = np.asarray(over, dtype=np.int32)
    clamped = clamp_boxes(boxes, hw)
    assert (clamped[:, :4] != boxes[:, :4]).any(1).all()
    ref_u8, ref_f32 = augment_ref(imgs_np, clamped, S)
    bd = torch.from_numpy(boxes).to(dev)
    _check_both_outputs(views, bd, S, None, ref_u8, ref_f32, "descriptor form")
    _check_both_outputs(batch, bd, S, sizes, ref_u8, ref_f32, "padded form")
    # sizes beyond the slot are clamped to the slot
    big = sizes + 1000
    slot_np = [b.cpu().numpy() for b in batch]
    hm, wm = batch.shape[1:3]
    ref_u8, ref_f32 = augment_ref(slot_np, clamp_boxes(boxes, [(hm, wm)] * len(over)), S)
    _check_both_outputs(batch, bd, S, big, ref_u8, ref_f32, "padded form, oversized sizes")


def _device_boxes(dev, hw, scale, counter, n=DRAW_B, sample_offset=0, flip_p=0.5):
    """maeclip_crop_params with every sample H x W (no pixels are needed to draw)"""
    from mae_clip_amd import _lib as L, kernels as K
    out = torch.empty((n, 5), dtype=torch.int32, device=dev)
    a = L.CropParamsArgs(H=hw[0], W=hw[1], boxes=out.data_ptr(), B=n, scale=(C.c_float * 2)(*scale),
                         ratio=(C.c_float * 2)(*RATIO), flip_p=flip_p, seed=SEED, sample_offset=sample_offset,
                         step_ptr=counter.data_ptr())
    K._call("maeclip_crop_params", C.byref(a), K._stream())
    return out


def test_device_draw_matches_host_draw(dev):
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    excluded = total = 0
    for hw in SIZES:
        for scale in SCALES:
            for step in STEPS:
                counter.fill_(step)
                got = _device_boxes(dev, hw, scale, counter).cpu().numpy()
                want = host_boxes(_sizes(hw), scale, step=step)
                _, near, _ = crop_params_ref(_sizes(hw), scale, RATIO, 0.5, SEED, step, 0)
                keep = ~near
                assert np.array_equal(got[keep], want[keep]), (hw, scale, step,
                                                               np.nonzero((got != want).any(1) & keep)[0][:8])
                assert np.array_equal(got[:, 4], want[:, 4])
                excluded += int(near.sum())
                total += near.size
    print(f"near-tie samples excluded: {excluded} of {total}")
    assert excluded <= 1e-3 * total


def test_crop_params_wrapper_both_source_forms(dev):
    """data.crop_params reads per-sample sizes from either source form"""
    from mae_clip_amd import data
    cases = _cases(32)
    views, batch, sizes, _ = _sources(cases, dev, seed=9)
    counter = torch.full((1,), 5, dtype=torch.int64, device=dev)
    hw = np.asarray([[c[0], c[1]] for c in cases], dtype=np.int32)
    want = host_boxes(hw, step=5, sample_offset=40)
    _, near, _ = crop_params_ref(hw, SCALES[0], RATIO, 0.5, SEED, 5, 40)
    for src, sz in ((views, None), (batch, sizes)):
        got = data.crop_params(src, sz, SCALES[0], RATIO, 0.5, SEED, counter, 40).cpu().numpy()
        assert np.array_equal(got[~near], want[~near])
    slot = np.tile(np.asarray(batch.shape[1:3], dtype=np.int32), (len(cases), 1))
    got = data.crop_params(batch, None, SCALES[0], RATIO, 0.5, SEED, counter, 40).cpu().numpy()
    _, near, _ = crop_params_ref(slot, SCALES[0], RATIO, 0.5, SEED, 5, 40)
    assert np.array_equal(got[~near], host_boxes(slot, step=5, sample_offset=40)[~near])


def _raw_batch(dev, B=4, Hm=48, Wm=56):
    from tests.helpers import make_batch
    g = torch.Generator().manual_seed(11)
    b = make_batch(B, 32, seed=3)
    sizes = torch.tensor([[48, 56], [40, 33], [17, 50], [48, 20]], dtype=torch.int32)
    return {"image": torch.randint(0, 256, (B, Hm, Wm, 3), generator=g, dtype=torch.uint8).to(dev),
            "image_sizes": sizes.to(dev), "input_ids": b["input_ids"].to(dev),
            "attention_mask": b["attention_mask"].to(dev)}, sizes.numpy()


def _train(dev, captured, batches, transform):
    from tests.helpers import product_config, C0
    from mae_clip_amd.CLIP import CLIPModel
    from mae_clip_amd.optim import AdamW
    from mae_clip_amd.graph import CapturedStep
    kw = {k: v for k, v in C0.items() if k != "batch_size"}
    with product_config(precision="bf16", **kw):
        torch.manual_seed(0)
        m = CLIPModel().to(dev).train()
    opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3)
    runner = CapturedStep(m, opt, enabled=captured, transform=transform)
    losses, images, boxes = [], [], []
    for batch in batches:
        losses.append(runner.step(batch).item())
        if transform is not None:
            images.append(transform.out.clone())
            boxes.append(transform.boxes.cpu().numpy().copy())
    assert runner.captures == (1 if captured else 0)
    return losses, images, boxes


def test_captured_step_draws_inside_the_graph(dev):
    """C0 model, uint8 padded batch, B = 4: the replayed graph feeds the model
    the very images the eager steps feed it, new ones every step."""
    from mae_clip_amd import data
    raw, sizes = _raw_batch(dev)
    steps = 4
    runs = []
    for captured in (False, True):
        aug = data.TrainAugment(32, seed=SEED)
        runs.append(_train(dev, captured, [raw] * steps, aug))
    (le, ie, be), (lg, ig, bg) = runs
    for s in range(steps):
        assert ie[s].dtype == torch.uint8 and ie[s].shape == (4, 32, 32, 3)
        assert torch.equal(ie[s], ig[s]), s
        assert np.array_equal(be[s], bg[s]), s
        # the boxes of step s can be learnt on the host
        _, near, _ = crop_params_ref(sizes, (0.08, 1.0), RATIO, 0.5, SEED, s, 0)
        assert np.array_equal(bg[s][~near], host_boxes(sizes, step=s)[~near]), s
        ref_u8, _ = augment_ref([raw["image"][i, :h, :w].cpu().numpy() for i, (h, w) in enumerate(sizes)],
                                bg[s][:, :5], 32)
        assert _same(ig[s], ref_u8), s
    for s in range(1, steps):
        assert (bg[s] != bg[s - 1]).any() and not torch.equal(ig[s], ig[s - 1]), s
    assert all(np.isfinite(v) for v in lg) and le == lg, (le, lg)
    # transform=None: the step is today's. Fed the images the transform produced,
    # it gives the same losses bit for bit, eagerly and replayed
    fed = [{"image": im, "input_ids": raw["input_ids"], "attention_mask": raw["attention_mask"]} for im in ig]
    for captured in (False, True):
        ln, _, _ = _train(dev, captured, fed, None)
        assert ln == lg, (captured, ln, lg)
