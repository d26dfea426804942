"""Fused multi-tensor AdamW on the libmaeclip kernel.

Same update as torch.optim.AdamW (main.py:101-103: lr 1e-3, weight_decay 1e-3,
betas (0.9, 0.999), eps 1e-8), one kernel launch for all parameters.

The step count t lives on the device as well (`_step_dev`, advanced by a
kernel before the update and read by it for the bias corrections), so the
optimizer step can be captured into a HIP graph together with the forward and
backward (mae_clip_amd.graph.CapturedStep). The per-parameter host
state["step"] is kept equal to it (state_dict / load_state_dict compatible
with torch.optim.AdamW).

Two options, both off by default, keep a normal training recipe inside one
captured graph:

device_lr=True   one device f32 array holds the learning rate of every
                 parameter group and the AdamW launch reads its group's slot.
                 group["lr"] stays the Python float schedulers, state_dict and
                 get_last_lr see; push_lr() sends it to the device when it
                 changed. Same fp32 value, same kernel arithmetic: bit-identical
                 to the by-value path.
max_grad_norm=c  torch.nn.utils.clip_grad_norm_(params, c) fused into the step:
                 a deterministic global norm over every parameter of every
                 group that has a gradient (two launches per step plus one per
                 group), and the AdamW kernel multiplies the gradient it reads
                 by min(1, c / (norm + 1e-6)). Unlike clip_grad_norm_, p.grad
                 itself is NOT rescaled. `grad_norm` and `clip_coef` are device
                 f32 [1] tensors refreshed by every step (stable storage).
                 Under data parallelism step() runs after sync_gradients(), so
                 every rank computes the same coefficient from the same reduced
                 gradients: no collective is added.
"""
from __future__ import annotations

import re

import torch

from . import kernels as K
from . import _lib as L
from .modules import shadow_of

_STORE_MAX = 32   # values of one maeclip_store_f32 launch


class AdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
                 device_lr=False):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"max_grad_norm must be > 0 or None, got {max_grad_norm}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._stager = K.PinnedStager(slots=2)
        self._step_dev = None     # device int64[1]: step count t of the uniform-step path
        self._dev_mirror = 0      # host copy of the value *_step_dev will hold when the stream gets there
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.device_lr = bool(device_lr)
        self._lr_dev = None       # device f32[len(param_groups)]
        self._lr_mirror = None    # the values the stream's last store wrote there
        self.grad_norm = None     # device f32[1]: global gradient norm of the last step
        self.clip_coef = None     # device f32[1]: factor the last step applied to the gradients
        self._partials = None     # device f32: per-workgroup sums of squares
        self._retired = []

    def _plan(self, entries, device):
        """Entry array staged through the pinned stager (async H2D, capturable)."""
        chunk = int(L.lib().maeclip_mt_chunk())
        n = len(entries)
        host = (L.MtEntry * n)()
        start = 0
        for i, e in enumerate(entries):
            h = host[i]
            h.p0, h.p1, h.p2, h.p3, h.p4 = e[:5]
            h.n = e[5]
            h.chunk_start = start
            start += (e[5] + chunk - 1) // chunk
        plan = K.MultiTensorPlan.__new__(K.MultiTensorPlan)
        plan.host, plan.dev, plan.n = host, self._stager.stage(host, device), n
        return plan

    def _device_step(self, t, device):
        """Advance the device step counter to t (normally +1) on the stream."""
        if self._step_dev is None or self._step_dev.device != device:
            self._step_dev = torch.zeros(1, dtype=torch.int64, device=device)
            self._dev_mirror = 0
        K.counter_add(self._step_dev, t - self._dev_mirror)
        self._dev_mirror = t
        return self._step_dev

    def push_lr(self):
        """device_lr: write every group["lr"] into the device array when one of
        them differs from what the stream last stored there (one launch per 32
        groups, none when nothing changed). Never call it on a capturing stream:
        a store captured into a graph would reset the rate on every replay.
        graph.CapturedStep calls it before each capture and replay."""
        if not self.device_lr:
            return
        lrs = [float(g["lr"]) for g in self.param_groups]
        device = next((p.device for g in self.param_groups for p in g["params"]), None)
        if device is None:
            return
        if self._lr_dev is None or self._lr_dev.numel() != len(lrs) or self._lr_dev.device != device:
            if K._capturing():
                raise L.MaeClipNativeError("AdamW(device_lr=True): run one eager step (or push_lr()) before a capture")
            self._lr_dev = torch.zeros(len(lrs), dtype=torch.float32, device=device)
            self._lr_mirror = None
        if lrs == self._lr_mirror:
            return
        if K._capturing():
            raise L.MaeClipNativeError("AdamW.push_lr() on a capturing stream: the rate would be baked into the graph")
        for i in range(0, len(lrs), _STORE_MAX):
            K.store_f32(self._lr_dev[i:i + _STORE_MAX], lrs[i:i + _STORE_MAX])
        self._lr_mirror = lrs

    def _clip(self, plans, device):
        """Global gradient norm over `plans` and the clip coefficient (device)."""
        need = sum(K.mt_blocks(pl) for pl in plans)
        if self._partials is None or self._partials.numel() < need or self._partials.device != device:
            if K._capturing():
                raise L.MaeClipNativeError(
                    "AdamW(max_grad_norm): clip buffers first needed inside a graph capture; run the step eagerly first")
            # an outgrown buffer is kept alive: a captured graph may still address it
            if self._partials is not None:
                self._retired.append(self._partials)
            self._partials = torch.zeros(need, dtype=torch.float32, device=device)
            if self.grad_norm is None or self.grad_norm.device != device:
                self.grad_norm = torch.zeros(1, dtype=torch.float32, device=device)
                self.clip_coef = torch.ones(1, dtype=torch.float32, device=device)
        off = 0
        for pl in plans:
            off += K.sumsq_multi(pl, self._partials, off)
        K.clip_coef(self._partials, off, self.max_grad_norm, self.grad_norm, self.clip_coef)
        return self.clip_coef

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.device_lr:
            if not K._capturing():
                self.push_lr()
            elif self._lr_dev is None:
                raise L.MaeClipNativeError("AdamW(device_lr=True): run one eager step (or push_lr()) before a capture")
        work = []     # (group index, plan, step count t, t is uniform over the group)
        device = None
        for gi, group in enumerate(self.param_groups):
            entries = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                K._dev(p)   # ROCm device parameters only (raises otherwise)
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] = int(st["step"]) + 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                # the bf16 GEMM shadow of p (if any) is written in the same pass
                sh = shadow_of(p)
                sh = sh.data_ptr() if sh is not None and sh.numel() == p.numel() else None
                entries.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                sh, p.numel(), st["step"]))
                device = p.device
            if not entries:
                continue
            steps = sorted({e[6] for e in entries})
            if len(steps) == 1:
                # every parameter at the same t (the training loop's case): t on the device
                work.append((gi, self._plan([e[:6] for e in entries], device), steps[0], True))
            else:
                for s in steps:
                    work.append((gi, self._plan([e[:6] for e in entries if e[6] == s], device), s, False))
        if not work:
            return loss
        # the norm is global (clip_grad_norm_(model.parameters())): every group's
        # gradients are summed before the first update
        coef = self._clip([w[1] for w in work], device) if self.max_grad_norm is not None else None
        for gi, plan, t, uniform in work:
            group = self.param_groups[gi]
            b1, b2 = group["betas"]
            lr_ptr = self._lr_dev[gi:gi + 1] if self.device_lr else None
            if uniform:
                step_ptr = self._device_step(t, device)
            else:
                # mixed step counts (parameters that joined later): t by value, or,
                # for the kernel to pair it with the device lr, in a device scalar
                step_ptr = torch.full((1,), t, dtype=torch.int64, device=device) if self.device_lr else None
            K.adamw_multi(plan, group["lr"], b1, b2, group["eps"], group["weight_decay"], t, step_ptr=step_ptr,
                          lr_ptr=lr_ptr, grad_scale_ptr=coef)
        return loss

    def _advance_host_steps(self, delta):
        """Host bookkeeping for graph replays / capture (no kernel launched)."""
        for st in self.state.values():
            if "step" in st:
                st["step"] = int(st["step"]) + delta
        self._dev_mirror += delta


_BLOCK = re.compile(r"(?:^|\.)blocks\.(\d+)\.")
_EMBED = re.compile(r"(?:^|\.)(?:cls_token$|pos_embed$|patch_embed\.)")
_NO_DECAY = re.compile(r"(?:^|\.)(?:cls_token|pos_embed)$")


def layer_decay_param_groups(model, lr, weight_decay, layer_decay):
    """Parameter groups with layer-wise learning-rate decay, as MAE's
    param_groups_lrd (BEiT's recipe): a parameter of layer id k trains at
    lr * layer_decay ** (depth + 1 - k). Layer ids by parameter name, under any
    prefix (ClassifierModel's `image_encoder.model.`): 0 for cls_token,
    pos_embed and patch_embed.*; i + 1 for blocks.i.*; depth + 1 for everything
    else (fc_norm, head), depth = the number of blocks. 1-D parameters (biases,
    norm scales), cls_token and pos_embed go into groups with weight_decay 0.
    Only parameters with requires_grad are included (a frozen encoder leaves
    the head's groups); empty groups are not returned.

    Every group carries "lr" (already scaled), "lr_scale", "weight_decay" and
    "name" ("layer_<k>_decay" / "layer_<k>_no_decay"), ordered by layer id. A
    scheduler sets group["lr"] = base_lr(step) * group["lr_scale"]. With
    AdamW(device_lr=True) the rates live in one device array; a ViT-B gives
    2 * 14 = 28 groups, one push_lr launch (<= 32)."""
    if not 0.0 < float(layer_decay) <= 1.0:
        raise ValueError(f"layer_decay must be in (0, 1], got {layer_decay}")
    named = list(model.named_parameters())
    blocks = [int(m.group(1)) for m in (_BLOCK.search(n) for n, _ in named) if m]
    depth = max(blocks) + 1 if blocks else 0
    groups = {}
    for name, p in named:
        if not p.requires_grad:
            continue
        m = _BLOCK.search(name)
        k = int(m.group(1)) + 1 if m else (0 if _EMBED.search(name) else depth + 1)
        no_decay = p.ndim == 1 or bool(_NO_DECAY.search(name))
        key = (k, no_decay)
        if key not in groups:
            scale = float(layer_decay) ** (depth + 1 - k)
            groups[key] = {"params": [], "lr": lr * scale, "lr_scale": scale,
                           "weight_decay": 0.0 if no_decay else weight_decay,
                           "name": f"layer_{k}_{'no_decay' if no_decay else 'decay'}"}
        groups[key]["params"].append(p)
    return [groups[key] for key in sorted(groups)]
