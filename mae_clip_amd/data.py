"""Device-side input pipeline.

The reference's CLIPDataset.__getitem__ (dataset.py:24-37) decodes each image
with cv2 (BGR -> RGB), runs albumentations Resize + Normalize
(get_transforms, dataset.py:44-58) and permutes HWC -> CHW float32 on the host;
main.py:55 then copies the fp32 batch to the GPU. Here decoding stays on the
host (cv2 / PIL, unchanged); the decoded uint8 HWC images cross PCIe as they
are (any sizes, 4x fewer bytes than the fp32 batch), and libmaeclip resizes,
normalises and transposes them in HBM in one pass
(maeclip_image_preprocess_u8 = Resize + Normalize + permute), producing
exactly the tensor the model takes. normalize_u8 is the resize-free variant
for batches already at the model's size.

Training augmentation (nothing in the reference): TrainAugment =
A.RandomResizedCrop + A.HorizontalFlip on the device, box and coin drawn from
the model's device step counter (maeclip_crop_params), pixels by
maeclip_image_augment_u8; crop_params / crop_params_host / augment_images are
its parts.

Mixup / CutMix (timm's Mixup; nothing in the reference): MixAugment, drawn the
same way (maeclip_mix_params), pixels by maeclip_mix_images, class-probability
targets by maeclip_mix_targets; mix_params / mix_params_host / mix_images /
mix_targets are its parts, Chain puts it behind TrainAugment.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .kernels import _dev, _call, _stream

# ImageNet statistics of albumentations' A.Normalize defaults (dataset.py:49)
from .kernels import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402


def normalize_u8(images: torch.Tensor, mean=IMAGENET_MEAN, std=IMAGENET_STD, max_pixel_value=255.0,
                 out: torch.Tensor = None) -> torch.Tensor:
    """uint8 [B, H, W, 3] (RGB, HWC) on the device -> float32 [B, 3, H, W]:
    (x - mean * max_pixel_value) / (std * max_pixel_value), albumentations'
    normalize() arithmetic in fp32 (dataset.py:49, 34)."""
    _dev(images, out)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        raise ValueError(f"normalize_u8: expected uint8 [B, H, W, 3], got {images.dtype} {tuple(images.shape)}")
    images = images.contiguous()
    B, H, W, _ = images.shape
    if out is None:
        out = torch.empty((B, 3, H, W), device=images.device, dtype=torch.float32)
    elif out.shape != (B, 3, H, W) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("normalize_u8: out must be a dense float32 [B, 3, H, W]")
    a = L.ImageU8Args(src=images.data_ptr(), dst=out.data_ptr(), B=B, H=H, W=W,
                      mean=(C.c_float * 3)(*mean), std=(C.c_float * 3)(*std), max_pixel=max_pixel_value)
    _call("maeclip_image_normalize_u8", C.byref(a), _stream())
    return out


def preprocess_images(images, size, mean=IMAGENET_MEAN, std=IMAGENET_STD, max_pixel_value=255.0, out=None):
    """get_transforms() of dataset.py:44-58 (+ the permute of :34) on the device:
    a list of uint8 HWC RGB images of any sizes (device tensors; row-strided
    views allowed) -> float32 [B, 3, size, size]: A.Resize(size, size) with
    cv2.INTER_LINEAR semantics, then A.Normalize."""
    descs = _descriptors(images, "preprocess_images")
    dev, B = images[0].device, len(images)
    if out is None:
        out = torch.empty((B, 3, size, size), device=dev, dtype=torch.float32)
    elif out.shape != (B, 3, size, size) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("preprocess_images: out must be a dense float32 [B, 3, size, size]")
    d = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    a = L.PreprocessArgs(images=d.data_ptr(), dst=out.data_ptr(), B=B, S=size, mean=(C.c_float * 3)(*mean),
                         std=(C.c_float * 3)(*std), max_pixel=max_pixel_value)
    _call("maeclip_image_preprocess_u8", C.byref(a), _stream())
    return out


def _descriptors(images, who):
    """maeclip_image_src array (host) of a list of uint8 [H, W, 3] device images."""
    if not images:
        raise ValueError(f"{who}: empty image list")
    dev = images[0].device
    descs = (L.ImageSrc * len(images))()
    for i, im in enumerate(images):
        _dev(im)
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.stride(2) != 1 or im.stride(1) != 3:
            raise ValueError(f"{who}: image {i} must be uint8 [H, W, 3] with packed pixels")
        if im.device != dev:
            raise ValueError(f"{who}: images on different devices")
        descs[i].src, descs[i].H, descs[i].W, descs[i].row_stride = im.data_ptr(), im.shape[0], im.shape[1], im.stride(0)
    return descs


# ------------------------------------------------- RandomResizedCrop + flip
def _source(src, sizes, who):
    """The two source forms of the augmentation entry points: a list of uint8
    [H, W, 3] device images (descriptor array, uploaded here) or one padded
    uint8 [B, Hmax, Wmax, 3] device batch with optional int32 [B, 2] valid
    (h, w) per slot. -> (B, device, struct fields, tensors to keep alive)."""
    if isinstance(src, (list, tuple)):
        if sizes is not None:
            raise ValueError(f"{who}: sizes belongs to the padded-batch form; a list carries its own sizes")
        descs = _descriptors(src, who)
        d = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(src[0].device)
        return len(src), src[0].device, dict(images=d.data_ptr()), (d,)
    _dev(src, sizes)
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[-1] != 3 or not src.is_contiguous():
        raise ValueError(f"{who}: expected a list of images or a dense uint8 [B, Hmax, Wmax, 3] batch")
    B, Hm, Wm, _ = src.shape
    if sizes is not None and (sizes.dtype != torch.int32 or sizes.shape != (B, 2) or not sizes.is_contiguous()
                              or sizes.device != src.device):
        raise ValueError(f"{who}: sizes must be a dense int32 [B, 2] of (h, w) on the batch's device")
    return B, src.device, dict(batch=src.data_ptr(), sizes=None if sizes is None else sizes.data_ptr(),
                               Hmax=Hm, Wmax=Wm), ()


def _boxes_out(out, B, dev, who):
    if out is None:
        return torch.empty((B, 5), device=dev, dtype=torch.int32)
    if out.shape != (B, 5) or out.dtype != torch.int32 or not out.is_contiguous():
        raise ValueError(f"{who}: boxes must be a dense int32 [B, 5]")
    return out


def crop_params(src, sizes=None, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip_p=0.5, seed=0, step_ptr=None,
                sample_offset=0, out=None):
    """A.RandomResizedCrop.get_params + the HorizontalFlip coin for every
    sample of `src` (either source form of augment_images), drawn on the
    device from (seed, *step_ptr, sample_offset + b): int32 [B, 5] =
    (x0, y0, w, h, flip). step_ptr: device int64 step counter (None: step 0)."""
    B, dev, fields, keep = _source(src, sizes, "crop_params")
    _dev(step_ptr, out)
    out = _boxes_out(out, B, dev, "crop_params")
    if "batch" in fields:
        fields = dict(sizes=fields["sizes"], H=fields["Hmax"], W=fields["Wmax"])
    a = L.CropParamsArgs(boxes=out.data_ptr(), B=B, scale=(C.c_float * 2)(*scale), ratio=(C.c_float * 2)(*ratio),
                         flip_p=flip_p, seed=int(seed), sample_offset=int(sample_offset),
                         step_ptr=None if step_ptr is None else step_ptr.data_ptr(), **fields)
    _call("maeclip_crop_params", C.byref(a), _stream())
    return out


def crop_params_host(sizes, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip_p=0.5, seed=0, step=0, sample_offset=0):
    """The boxes crop_params draws at device step `step`, evaluated on the CPU
    by the same function (no device needed): for logging, or to crop the box
    annotations of step s. sizes: CPU int32 [B, 2] of (h, w). -> CPU int32 [B, 5]."""
    sizes = torch.as_tensor(sizes, dtype=torch.int32).contiguous()
    if sizes.is_cuda or sizes.dim() != 2 or sizes.shape[1] != 2:
        raise ValueError("crop_params_host: sizes must be a CPU int32 [B, 2] of (h, w)")
    B = sizes.shape[0]
    out = torch.empty((B, 5), dtype=torch.int32)
    step_v = C.c_int64(int(step))
    lim = 2 ** 31 - 1
    a = L.CropParamsArgs(sizes=sizes.data_ptr(), H=lim, W=lim, boxes=out.data_ptr(), B=B,
                         scale=(C.c_float * 2)(*scale), ratio=(C.c_float * 2)(*ratio), flip_p=flip_p, seed=int(seed),
                         sample_offset=int(sample_offset), step_ptr=C.addressof(step_v))
    _call("maeclip_crop_params_host", C.byref(a))
    return out


def augment_images(src, boxes, size, out_dtype=torch.uint8, sizes=None, out=None, mean=IMAGENET_MEAN,
                   std=IMAGENET_STD, max_pixel_value=255.0):
    """crop -> cv2.resize(INTER_LINEAR) to size x size -> horizontal flip of
    every sample by its row of `boxes` (device int32 [B, 5] = x0, y0, w, h,
    flip; crop_params' or the caller's own, clamped into the image).
    src: a list of uint8 [H, W, 3] device images of any sizes (row-strided
    views allowed), or a padded uint8 [B, Hmax, Wmax, 3] batch with optional
    `sizes` int32 [B, 2] = valid (h, w) per slot. out_dtype: torch.uint8 ->
    [B, size, size, 3] pixels the model consumes as they are; torch.float32 ->
    A.Normalize'd [B, 3, size, size] (the floats of normalize_u8)."""
    B, dev, fields, keep = _source(src, sizes, "augment_images")
    _dev(boxes, out)
    if boxes is None:
        raise ValueError("augment_images: boxes is required (crop_params draws them)")
    boxes = _boxes_out(boxes, B, dev, "augment_images")
    if out_dtype not in (torch.uint8, torch.float32):
        raise ValueError("augment_images: out_dtype must be torch.uint8 or torch.float32")
    shape = (B, size, size, 3) if out_dtype == torch.uint8 else (B, 3, size, size)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=out_dtype)
    elif out.shape != shape or out.dtype != out_dtype or not out.is_contiguous():
        raise ValueError(f"augment_images: out must be a dense {out_dtype} {list(shape)}")
    dst = dict(dst_u8=out.data_ptr()) if out_dtype == torch.uint8 else dict(dst_f32=out.data_ptr())
    a = L.AugmentArgs(boxes=boxes.data_ptr(), B=B, S=size, mean=(C.c_float * 3)(*mean), std=(C.c_float * 3)(*std),
                      max_pixel=max_pixel_value, **fields, **dst)
    _call("maeclip_image_augment_u8", C.byref(a), _stream())
    return out


class TrainAugment:
    """MAE's / CLIP's training augmentation on the device:
    A.RandomResizedCrop(size, size, scale, ratio) -> A.HorizontalFlip(flip_p)
    (-> A.Normalize + permute for out_dtype=torch.float32), with box and coin
    drawn on the device from the step counter, so it can run inside a captured
    step (graph.CapturedStep(transform=...)) and still change every replay.

    __call__(batch, step_ptr, sample_offset=0) returns a new dict whose
    "image" is the augmented batch; batch["image"] is either source form of
    augment_images, an "image_sizes" entry gives the padded form's valid sizes
    and is dropped, every other key passes through. Box and output buffers
    are allocated once per batch size and reused: stable storage for capture
    (`boxes` / `out` hold the last call's)."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip_p=0.5, seed=None, out_dtype=torch.uint8):
        from . import config as CFG
        self.size, self.scale, self.ratio, self.flip_p = int(size), tuple(scale), tuple(ratio), float(flip_p)
        self.seed = int(CFG.augment_seed if seed is None else seed)
        self.out_dtype = out_dtype
        self._bufs = {}
        self.boxes = self.out = None

    def __call__(self, batch, step_ptr, sample_offset=0):
        src, sizes = batch["image"], batch.get("image_sizes")
        B = len(src)
        dev = src[0].device
        if (B, dev) not in self._bufs:
            shape = (B, self.size, self.size, 3) if self.out_dtype == torch.uint8 else (B, 3, self.size, self.size)
            self._bufs[B, dev] = (torch.empty((B, 5), device=dev, dtype=torch.int32),
                                  torch.empty(shape, device=dev, dtype=self.out_dtype))
        self.boxes, self.out = self._bufs[B, dev]
        crop_params(src, sizes, self.scale, self.ratio, self.flip_p, self.seed, step_ptr, sample_offset, out=self.boxes)
        augment_images(src, self.boxes, self.size, self.out_dtype, sizes, out=self.out)
        out = {k: v for k, v in batch.items() if k not in ("image", "image_sizes")}
        out["image"] = self.out
        return out


def train_augment_from_config():
    """TrainAugment of the config.augment_* flags, or None when config.augment is off."""
    from . import config as CFG
    if not CFG.augment:
        return None
    return TrainAugment(CFG.size, CFG.augment_scale, CFG.augment_ratio, CFG.augment_flip_p, CFG.augment_seed)


# ------------------------------------------------------------ Mixup / CutMix
_MIX_MODES = {"batch": L.MIX_BATCH, "elem": L.MIX_ELEM, L.MIX_BATCH: L.MIX_BATCH, L.MIX_ELEM: L.MIX_ELEM}


def _mix_mode(mode, who):
    if mode not in _MIX_MODES:
        raise ValueError(f"{who}: mode must be 'batch' or 'elem' (timm's 'pair' is not built), got {mode!r}")
    return _MIX_MODES[mode]


def _mix_records(params, B, who):
    if params is None or params.dtype != torch.int32 or params.shape != (B, 8) or not params.is_contiguous():
        raise ValueError(f"{who}: params must be a dense int32 [B, 8] (B = {B})")
    return params


def mix_params(B, H, W, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", seed=0,
               step_ptr=None, sample_offset=0, out=None, device=None):
    """timm's Mixup draw (correct_lam, partner = B-1-b) for B samples of H x W
    pixels, on the device from (seed, *step_ptr, and in mode "elem"
    sample_offset + b; mode "batch": one draw for all, the same on every
    data-parallel rank): int32 [B, 8] = (kind, partner, x0, y0, x1, y1, bits of
    f32 lam_pixel, bits of f32 lam_target); kind 0 none, 1 mixup, 2 cutmix
    (include/maeclip.h maeclip_mix_params). step_ptr: device int64 step counter
    (None: step 0). The records live on `out`'s / step_ptr's / `device`."""
    mode = _mix_mode(mode, "mix_params")
    if out is not None:
        _mix_records(out, B, "mix_params")
    _dev(step_ptr, out)
    if out is None:
        dev = step_ptr.device if step_ptr is not None else device
        if dev is None:
            raise ValueError("mix_params: one of out, step_ptr or device says where to draw")
        out = torch.empty((B, 8), device=dev, dtype=torch.int32)
        _dev(out)
    a = L.MixParamsArgs(params=out.data_ptr(), B=B, H=H, W=W, mixup_alpha=mixup_alpha, cutmix_alpha=cutmix_alpha,
                        prob=prob, switch_prob=switch_prob, mode=mode, seed=int(seed), sample_offset=int(sample_offset),
                        step_ptr=None if step_ptr is None else step_ptr.data_ptr())
    _call("maeclip_mix_params", C.byref(a), _stream())
    return out


def mix_params_host(B, H, W, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", seed=0,
                    step=0, sample_offset=0):
    """The records mix_params draws at device step `step`, evaluated on the CPU
    by the same function (no device needed): for logging, or to know step s's
    mix on the host. -> CPU int32 [B, 8]; columns 6 and 7 .view(torch.float32)
    are the two lams."""
    mode = _mix_mode(mode, "mix_params_host")
    out = torch.empty((B, 8), dtype=torch.int32)
    step_v = C.c_int64(int(step))
    a = L.MixParamsArgs(params=out.data_ptr(), B=B, H=H, W=W, mixup_alpha=mixup_alpha, cutmix_alpha=cutmix_alpha,
                        prob=prob, switch_prob=switch_prob, mode=mode, seed=int(seed), sample_offset=int(sample_offset),
                        step_ptr=C.addressof(step_v))
    _call("maeclip_mix_params_host", C.byref(a))
    return out


def _mix_form(images, who):
    """(B, S, library dtype) of a batch in one of the two forms the model takes"""
    ok = torch.is_tensor(images) and images.dim() == 4 and images.is_contiguous()
    if ok and images.dtype == torch.uint8 and images.shape[3] == 3 and images.shape[1] == images.shape[2]:
        return images.shape[0], images.shape[1], 0
    if ok and images.dtype == torch.float32 and images.shape[1] == 3 and images.shape[2] == images.shape[3]:
        return images.shape[0], images.shape[2], 1
    raise ValueError(f"{who}: images must be a dense uint8 [B, S, S, 3] or float32 [B, 3, S, S] batch")


def mix_images(images, params, out=None):
    """The batch mixed by `params` (device int32 [B, 8]; mix_params' or the
    caller's own): kind 0 copies, 1 (mixup) writes lam a + (1 - lam) p in fp32
    (uint8: rounded half to even), 2 (cutmix) takes the partner's pixels inside
    the box (clamped into the image). images: uint8 [B, S, S, 3] or float32
    [B, 3, S, S]; out: the same form, not overlapping `images` (out of place)."""
    B, S, dt = _mix_form(images, "mix_images")
    _mix_records(params, B, "mix_images")
    if out is not None and (out.shape != images.shape or out.dtype != images.dtype or not out.is_contiguous()):
        raise ValueError(f"mix_images: out must be a dense {images.dtype} {list(images.shape)}")
    _dev(images, params, out)
    if out is None:
        out = torch.empty_like(images)
    a = L.MixImagesArgs(src=images.data_ptr(), dst=out.data_ptr(), params=params.data_ptr(), B=B, S=S, dtype=dt)
    _call("maeclip_mix_images", C.byref(a), _stream())
    return out


def mix_targets(labels, params, num_classes, out=None):
    """Class-probability targets of the mix: float32 [B, num_classes] with
    lam_target at the own label and 1 - lam_target at the partner's (exactly 1
    where they coincide; a label outside [0, num_classes) contributes nothing).
    No label smoothing here: ClassifierModel(label_smoothing=eps) / xent apply
    it to soft targets, which is timm's mixup_target + SoftTargetCrossEntropy.
    out: a dense float32 [B, ld_t], ld_t >= num_classes; its columns from
    num_classes on get zeros."""
    if not torch.is_tensor(labels) or labels.dim() != 1 or labels.dtype not in (torch.int64, torch.int32):
        raise ValueError("mix_targets: labels must be int64 or int32 [B]")
    labels = labels.contiguous()
    B, Cn = labels.shape[0], int(num_classes)
    _mix_records(params, B, "mix_targets")
    if out is not None and (out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.shape[1] < Cn
                            or not out.is_contiguous()):
        raise ValueError(f"mix_targets: out must be a dense float32 [B, ld_t] with ld_t >= C = {Cn}")
    _dev(labels, params, out)
    if out is None:
        out = torch.empty((B, Cn), device=labels.device, dtype=torch.float32)
    a = L.MixTargetsArgs(labels=labels.data_ptr(), label_dtype=int(labels.dtype == torch.int64),
                         params=params.data_ptr(), targets=out.data_ptr(), ld_t=out.shape[1], B=B, C=Cn)
    _call("maeclip_mix_targets", C.byref(a), _stream())
    return out


class MixAugment:
    """timm's Mixup(mixup_alpha, cutmix_alpha, prob, switch_prob, mode,
    correct_lam=True) on the device, drawn from the step counter like
    TrainAugment, so it runs inside a captured step and mixes anew on every
    replay. Label smoothing is the model's (ClassifierModel(label_smoothing=)).

    __call__(batch, step_ptr, sample_offset=0) reads batch["image"] (uint8
    [B, S, S, 3] or float32 [B, 3, S, S]) and batch["label"] and returns a new
    dict with the mixed "image" and a "target" (float32 [B, num_classes]);
    "label" and every other key pass through. Record, image and target buffers
    are allocated once per (B, S, device, dtype) and reused: stable storage for
    capture (`params` / `out` / `target` hold the last call's)."""

    def __init__(self, num_classes, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch",
                 seed=None):
        from . import config as CFG
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError(f"MixAugment: num_classes must be >= 1, got {num_classes}")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        self.mode = _mix_mode(mode, "MixAugment")
        self.seed = int(CFG.mix_seed if seed is None else seed)
        self._bufs = {}
        self.params = self.out = self.target = None

    def __call__(self, batch, step_ptr, sample_offset=0):
        img, labels = batch["image"], batch["label"]
        B, S, _ = _mix_form(img, "MixAugment")
        key = (B, S, img.device, img.dtype)
        if key not in self._bufs:
            cpad = (self.num_classes + 3) // 4 * 4        # rows of whole 16-byte pieces
            self._bufs[key] = (torch.empty((B, 8), device=img.device, dtype=torch.int32), torch.empty_like(img),
                               torch.empty((B, cpad), device=img.device, dtype=torch.float32))
        self.params, self.out, tpad = self._bufs[key]
        mix_params(B, S, S, self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob, self.mode, self.seed,
                   step_ptr, sample_offset, out=self.params)
        mix_images(img, self.params, out=self.out)
        mix_targets(labels, self.params, self.num_classes, out=tpad)
        self.target = tpad[:, :self.num_classes]
        out = dict(batch)
        out["image"], out["target"] = self.out, self.target
        return out


class Chain:
    """Transforms applied in order under TrainAugment's call contract:
    Chain(TrainAugment(S), MixAugment(C))(batch, step_ptr, sample_offset)."""

    def __init__(self, *transforms):
        self.transforms = tuple(t for t in transforms if t is not None)

    def __call__(self, batch, step_ptr, sample_offset=0):
        for t in self.transforms:
            batch = t(batch, step_ptr, sample_offset)
        return batch


def mix_augment_from_config():
    """MixAugment of the config.mix* / *_alpha flags, or None when both alphas are 0 (the default)."""
    from . import config as CFG
    if not (CFG.mixup_alpha > 0 or CFG.cutmix_alpha > 0):
        return None
    return MixAugment(CFG.num_classes, CFG.mixup_alpha, CFG.cutmix_alpha, CFG.mix_prob, CFG.mix_switch_prob,
                      CFG.mix_mode, CFG.mix_seed)


def to_device_batch(images_u8, input_ids, attention_mask, device, non_blocking=True, augment=None, step_ptr=None,
                    sample_offset=0):
    """The dict main.train_epoch feeds the model (main.py:55), built from a
    host uint8 HWC batch: upload uint8, normalise on the device. augment (a
    TrainAugment): the uploaded pixels go through it instead, drawn at
    *step_ptr (the model's step_counter)."""
    imgs = images_u8.to(device, non_blocking=non_blocking)
    batch = {"image": imgs if augment is not None else normalize_u8(imgs),
             "input_ids": input_ids.to(device, non_blocking=non_blocking),
             "attention_mask": attention_mask.to(device, non_blocking=non_blocking)}
    return batch if augment is None else augment(batch, step_ptr, sample_offset)
