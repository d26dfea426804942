"""Cost of a per-step LR schedule and of gradient clipping in the captured step.

usage: python tools/optim_probe.py [--batch 256] [--steps 20] [--rounds 3] [--warmup 5]
       python tools/optim_probe.py --trace [--steps 4]

C2 model shapes (ViT-B/16 @224, mask .75, 8x512 decoder, 6-layer text, T = 25),
bf16, the whole step (forward, backward, fused AdamW) as a captured HIP graph
(graph.CapturedStep). Three optimizers on three models side by side:

  default    optim.AdamW(...), constant lr
  device_lr  optim.AdamW(device_lr=True), lr changed before EVERY step (a
             per-batch scheduler): one store launch + one replay per step
  clip       optim.AdamW(max_grad_norm=1.0), constant lr

timed in alternating blocks of `--steps` steps (HIP events around each block),
`--rounds` times, after `--warmup` steps each (the eager step and the capture
among them), so that clock and thermal drift hit all alike. Prints every block,
the medians, the differences from `default` and each runner's capture count.
(The default optimizer under a per-step schedule is not timed: it re-captures
every step, which `--recapture N` shows by its capture count over N steps.)

--trace: `--steps` eager steps of `default` and then of device_lr + clip, and
nothing else, for a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o op -- python tools/optim_probe.py --trace
The stats list adamw_multi_kernel (both variants are the one kernel: compare
the first and the second half of its launches in the trace), sumsq_multi_kernel,
clip_coef_kernel and store_f32_kernel per launch.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C2 = dict(model_name="vit_base_patch16_224", size=224, image_embedding=768, mask_ratio=0.75)


def build(dev, **opt_kw):
    from mae_clip_amd import config as CFG
    from mae_clip_amd.CLIP import CLIPModel
    from mae_clip_amd.optim import AdamW
    old = {k: getattr(CFG, k) for k in list(C2) + ["precision"]}
    try:
        for k, v in dict(C2, precision="bf16").items():
            setattr(CFG, k, v)
        torch.manual_seed(0)
        m = CLIPModel().to(dev).train()
    finally:
        for k, v in old.items():
            setattr(CFG, k, v)
    opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3, **opt_kw)
    return m, opt


def batch(B, dev):
    g = torch.Generator().manual_seed(1)
    return {"image": torch.randn((B, 3, 224, 224), generator=g).to(dev),
            "input_ids": torch.randint(5, 300, (B, 25), generator=g).to(dev),
            "attention_mask": torch.ones((B, 25), dtype=torch.int64).to(dev)}


def schedule(opt, k):
    """a new rate before every step (what a per-batch scheduler does)"""
    for g in opt.param_groups:
        g["lr"] = 1e-3 * (0.5 + 0.5 * ((k * 37) % 101) / 101.0)


MODES = (("default", {}, False), ("device_lr", dict(device_lr=True), True), ("clip", dict(max_grad_norm=1.0), False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--recapture", type=int, default=0, metavar="N",
                    help="also run N steps of the default optimizer under the per-step schedule and print its captures")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    from mae_clip_amd import _lib
    from mae_clip_amd.graph import CapturedStep
    _lib.load()
    dev = torch.device("cuda:0")
    b = batch(a.batch, dev)
    if a.trace:
        n = a.steps or 4
        for name, kw in (("default", {}), ("device_lr + clip", dict(device_lr=True, max_grad_norm=1.0))):
            m, opt = build(dev, **kw)
            run = CapturedStep(m, opt, enabled=False)
            for k in range(n):
                if kw:
                    schedule(opt, k)
                run.step(b)
            torch.cuda.synchronize()
            print(f"traced {n} eager steps of {name}, loss {run.loss_value():.4f}")
            del run, m, opt
        return
    steps = a.steps or 20
    runs, count = {}, {}
    for name, kw, sched in MODES:
        m, opt = build(dev, **kw)
        r = CapturedStep(m, opt)
        count[name] = 0
        for _ in range(a.warmup):
            if sched:
                schedule(opt, count[name])
            r.step(b)
            count[name] += 1
        torch.cuda.synchronize()
        print(f"{name}: captures {r.captures} after {a.warmup} warm-up steps, loss {r.loss_value():.4f}")
        runs[name] = (r, opt, sched)
    ms = {k: [] for k in runs}
    for rd in range(a.rounds):
        for name, (r, opt, sched) in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                if sched:
                    schedule(opt, count[name])
                r.step(b)
                count[name] += 1
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / steps)
            print(f"round {rd} {name:9s} {ms[name][-1]:8.3f} ms/step over {steps} steps")
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(f"C2 shapes, B = {a.batch}, T = 25, bf16, captured step, {a.rounds} alternating rounds of {steps} steps")
    for name, (r, opt, _) in runs.items():
        d = med[name] - med["default"]
        extra = ""
        if opt.max_grad_norm is not None:
            extra = f"  grad_norm {opt.grad_norm.item():.4f} clip_coef {opt.clip_coef.item():.4f}"
        print(f"{name:9s} median {med[name]:8.3f} ms/step  vs default {d:+.3f} ms ({100 * d / med['default']:+.2f} %)  "
              f"captures {r.captures} over {count[name]} steps{extra}")
    if a.recapture > 0:
        m, opt = build(dev)
        r = CapturedStep(m, opt)
        for k in range(a.recapture):
            schedule(opt, k)
            r.step(b)
        torch.cuda.synchronize()
        print(f"default under the per-step schedule: captures {r.captures} over {a.recapture} steps")


if __name__ == "__main__":
    main()
