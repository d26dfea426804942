"""Supervised evaluation of a pretrained image encoder: linear probe and
fine-tuning, the two numbers an MAE / CLIP encoder is judged by.

ClassifierModel = ImageEncoder (the CLIPModel's `image_encoder`, same
state_dict keys) + `head` (one nn.Linear, timm's name), trained with softmax
cross-entropy on the fused kernel (kernels.xent_fwd / xent_bwd):

    model = ClassifierModel(num_classes=1000, trainable_encoder=False)   # linear probe
    load_image_encoder(model, "pretrain/checkpoint.pt")
    opt = AdamW([p for p in model.parameters() if p.requires_grad], ...)
    runner = CapturedStep(model.cuda(), opt, transform=TrainAugment(size))
    for batch in loader:                   # {"image": ..., "label": int64 [B]}
        runner.step(batch)
    evaluate(model.eval(), val_batches)    # {"loss", "top1", "top5", "n"}

forward(batch) is the training contract of CLIPModel: a 0-d loss, with
step_counter / step_snaps / step / last_losses / process_group / grad_arena as
CLIPModel has them, so graph.CapturedStep, data.TrainAugment, checkpoint and
distributed.DataParallel take it unchanged. batch["target"] (class
probabilities [B, num_classes], e.g. from Mixup / CutMix) replaces
batch["label"] when present.

Mixup / CutMix are data.MixAugment (a CapturedStep transform that writes
batch["target"]; label_smoothing here then gives timm's smoothed mix targets),
layer-wise learning-rate decay is optim.layer_decay_param_groups (DESIGN.md
Round 16), drop-path is ClassifierModel(drop_path_rate=...) / config.drop_path_rate
(fine-tuning only). Not here: MAE's BatchNorm1d in front of
the probe head and LARS.
"""
from __future__ import annotations

import torch
from torch import nn

from . import config as CFG
from . import functions as Fn
from . import kernels as K
from . import modules as Mo
from .modules import ImageEncoder, WeightCache, compute_dtype, _trunc_normal_


class ClassifierModel(nn.Module):
    def __init__(self, num_classes=None, trainable_encoder=None, label_smoothing=None, drop_path_rate=None):
        super().__init__()
        num_classes = CFG.num_classes if num_classes is None else int(num_classes)
        trainable_encoder = CFG.classifier_trainable_encoder if trainable_encoder is None else trainable_encoder
        label_smoothing = CFG.label_smoothing if label_smoothing is None else float(label_smoothing)
        if num_classes < 1:
            raise ValueError(f"num_classes must be >= 1, got {num_classes}")
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")
        # stochastic depth regularises a trained encoder: a frozen one (linear probe) has none.
        # config.drop_path_rate is a setting of the run and is ignored here for a probe; asking
        # this model for it (the argument) is a mistake and raises
        if drop_path_rate is not None and float(drop_path_rate) > 0 and not trainable_encoder:
            raise ValueError("drop_path_rate > 0 needs trainable_encoder=True (fine-tuning); the linear probe's "
                             "encoder is frozen")
        self.image_encoder = ImageEncoder(trainable=bool(trainable_encoder),
                                          drop_path_rate=drop_path_rate if trainable_encoder else 0.0)
        self.drop_path_seed = (CFG.dropout_seed * 1000003 + 43) & 0x7FFFFFFFFFFFFFFF
        self.head = nn.Linear(self.image_encoder.model.embed_dim, num_classes)
        _trunc_normal_(self.head.weight, std=CFG.head_init_std)
        nn.init.zeros_(self.head.bias)
        self.num_classes = num_classes
        self.trainable_encoder = bool(trainable_encoder)
        self.label_smoothing = label_smoothing
        self.precision = CFG.precision
        self.step = 0
        # as CLIPModel: the device step (TrainAugment draws from it, CapturedStep
        # picks its loss slot by it), advanced by a kernel of every training forward
        self.register_buffer("step_counter", torch.zeros(1, dtype=torch.int64), persistent=False)
        self.register_buffer("step_snaps", torch.zeros(8, dtype=torch.int64), persistent=False)
        self.last_losses = {}
        self.process_group = None
        self.grad_arena = None     # set by distributed.DataParallel
        self._cache = None
        self._head_pad = None

    # ------------------------------------------------------------------
    def _weight_cache(self):
        if self._cache is None:
            c = WeightCache(fp8=self.precision == "fp8")
            self.image_encoder.model.register_weights(c)
            self._cache = c
        return self._cache

    def _world(self):
        pg = self.process_group
        if pg is None or not torch.distributed.is_initialized():
            return 1, 0
        return torch.distributed.get_world_size(pg), torch.distributed.get_rank(pg)

    def _head_spec(self):
        """The head's GEMM operands: the parameters themselves when num_classes is
        a multiple of 4, else zero-padded copies refreshed from them (the pad
        rows / entries stay zero; VisionTransformer.forward_tokens' kpad trick)."""
        w, b = self.head.weight, self.head.bias
        C, D = w.shape
        cpad = (C + 3) // 4 * 4
        if cpad == C:
            return Fn.HeadSpec(C=C, w_pad=w.detach(), b_pad=b.detach())
        pad = self._head_pad
        if pad is None or pad[0].shape != (cpad, D) or pad[0].device != w.device:
            pad = (torch.zeros((cpad, D), device=w.device, dtype=torch.float32),
                   torch.zeros((cpad,), device=w.device, dtype=torch.float32))
            self._head_pad = pad
        pad[0][:C].copy_(w.detach())
        pad[1][:C].copy_(b.detach())
        return Fn.HeadSpec(C=C, w_pad=pad[0], b_pad=pad[1])

    def _padded_logits(self, img, world=1, rank=0, snap=None):
        """[B, Cpad] fp32 logits (columns >= num_classes are padding). snap: the
        step snapshot slot of a training forward (drop-path's backward reads it)."""
        Mo._require_device(img, "image batch")
        dtype = compute_dtype(self.precision)
        vit = self.image_encoder.model
        cache = self._weight_cache()
        cache.refresh(dtype)
        # the drop-path seed is the same on every rank: the sample offset tells the ranks apart
        tokens = vit.forward_tokens(img, dtype, cache, world=world, dp_seed=self.drop_path_seed,
                                    step_ptr=self.step_counter, bwd_step_ptr=snap, sample_offset=rank * img.shape[0])
        feat = Fn.EncoderHeadFn.apply(tokens, dtype, vit.fc_norm.weight, vit.fc_norm.bias, None, None)
        return Fn.ClassifierHeadFn.apply(feat, self._head_spec(), self.head.weight, self.head.bias)

    def logits(self, images):
        """[B, num_classes] fp32 class logits, no autograd."""
        with torch.no_grad():
            return self._padded_logits(images)[:, :self.num_classes]

    def forward(self, batch):
        """batch["image"]: fp32 NCHW normalised images or uint8 RGB HWC pixels, as
        CLIPModel takes them; batch["label"]: int64 / int32 [B] class indices, or
        batch["target"]: fp32 [B, num_classes] class probabilities (then the
        loss is theirs). Returns the 0-d loss, mean over the batch (over the
        global batch under data parallelism: loss_scale = 1 / world, so a SUM
        all-reduce of the parameter gradients is the global-batch gradient)."""
        img = batch["image"]
        Mo._require_device(img, "image batch")
        sc = self.step_counter
        Mo._require_device(sc, "ClassifierModel.step_counter (call .to(device))")
        world, rank = self._world()
        Fn.set_grad_arena(self.grad_arena if torch.is_grad_enabled() else None)
        snap = self.step_snaps[self.step % 8:self.step % 8 + 1] if self.training else None
        logits = self._padded_logits(img, world, rank, snap)
        targets = batch.get("target")
        labels = None
        if targets is None:
            labels = batch["label"]
            if labels.dtype not in (torch.int64, torch.int32):
                raise TypeError(f"batch['label'] must be int64 or int32, got {labels.dtype}")
            labels = labels.contiguous()
        else:
            if targets.dim() != 2 or targets.shape[1] != self.num_classes:
                raise ValueError(f"batch['target'] must be [B, {self.num_classes}], got {tuple(targets.shape)}")
            targets = targets.float() if targets.dtype != torch.float32 else targets
            targets = targets if targets.stride(1) == 1 else targets.contiguous()
        spec = Fn.XentSpec(C=self.num_classes, label_smoothing=self.label_smoothing, loss_scale=1.0 / world)
        loss = Fn.SoftmaxXentFn.apply(logits, labels, targets, spec)
        self.last_losses = {"xent": loss.detach()}
        if self.training:
            K.counter_add_snap(sc, snap, 1)
            self.step += 1
        return loss


def load_image_encoder(model, state_dict_or_path):
    """Copy the `image_encoder.*` entries of a CLIPModel state dict -- or of a
    file written by checkpoint.save_checkpoint or torch.save(model.state_dict())
    -- into model.image_encoder. Every encoder key must be there with the
    model's shape (a checkpoint of another model_name / size raises); the head
    keeps its initialisation. Returns the keys that were not used (the text
    tower, the projections, the MAE decoder, ...)."""
    sd = state_dict_or_path
    if not isinstance(sd, dict):
        sd = torch.load(sd, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and isinstance(sd.get("model"), dict) and "format" in sd:
        sd = sd["model"]
    prefix = "image_encoder."
    enc = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    skipped = [k for k in sd if not k.startswith(prefix)]
    own = model.image_encoder.state_dict()
    missing = [k for k in own if k not in enc]
    extra = [k for k in enc if k not in own]
    bad = [f"{k}: {tuple(enc[k].shape)} vs {tuple(own[k].shape)}" for k in own if k in enc and enc[k].shape != own[k].shape]
    if missing or extra or bad:
        raise RuntimeError(f"load_image_encoder: the checkpoint's image encoder does not fit the model: "
                           f"missing {missing[:4]}, unexpected {extra[:4]}, shape mismatch {bad[:4]}")
    model.image_encoder.load_state_dict(enc, strict=True)
    return skipped


def evaluate(model, batches, ks=(1, 5)):
    """Mean cross-entropy (no label smoothing, as validation reports it) and
    top-k accuracies over `batches` (dicts with "image" and "label"), from the
    loss kernel's rank output: a sample is a top-k hit iff fewer than k classes
    rank before its label (ties broken by class index). Forward launches only;
    the sums stay on the device and are read once at the end. Returns
    {"loss", "top<k>" for k in ks, "n"}."""
    C = model.num_classes
    tot = None
    n = 0
    with torch.no_grad():
        for batch in batches:
            labels = batch["label"].contiguous()
            out = K.xent_fwd(model._padded_logits(batch["image"]), labels, C=C, want_rank=True)
            B = labels.shape[0]
            part = torch.stack([out.loss.double() * B] + [(out.rank < k).sum().double() for k in ks])
            tot = part if tot is None else tot + part
            n += B
    if n == 0:
        raise ValueError("evaluate: no batches")
    vals = tot.cpu().tolist()
    res = {"loss": vals[0] / n, "n": n}
    for k, v in zip(ks, vals[1:]):
        res[f"top{k}"] = v / n
    return res
