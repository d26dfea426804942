"""Cost of the learnable CLIP temperature in the captured step.

usage: python tools/temperature_probe.py [--batch 256] [--steps 20] [--rounds 3] [--warmup 5]

C2 model shapes (ViT-B/16 @224, mask .75, 8x512 decoder, 6-layer text, T = 25),
bf16, the whole step (forward, backward, fused AdamW) as a captured HIP graph
(graph.CapturedStep). Two models side by side:

  default    config.learnable_temperature = False: tau a float in the loss
             launch's arguments, one parameter group
  learnable  config.learnable_temperature = True: theta = ln tau on the device,
             d loss / d theta from the loss call (the other instantiation of
             the gradient kernel + a one-workgroup sum), theta in a second
             parameter group with weight_decay = 0 (one more AdamW launch and
             one more step-counter launch per step)

timed in alternating blocks of `--steps` steps (HIP events around each block),
`--rounds` times, after `--warmup` steps each (the eager step and the capture
among them), so that clock and thermal drift hit both alike. Prints every
block, the medians, the difference, each runner's capture count and theta
before and after.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C2 = dict(model_name="vit_base_patch16_224", size=224, image_embedding=768, mask_ratio=0.75)


def build(dev, learnable):
    from mae_clip_amd import config as CFG
    from mae_clip_amd.CLIP import CLIPModel
    from mae_clip_amd.optim import AdamW
    over = dict(C2, precision="bf16", learnable_temperature=learnable)
    old = {k: getattr(CFG, k) for k in over}
    try:
        for k, v in over.items():
            setattr(CFG, k, v)
        torch.manual_seed(0)
        m = CLIPModel().to(dev).train()
    finally:
        for k, v in old.items():
            setattr(CFG, k, v)
    rest = [p for n, p in m.named_parameters() if p.requires_grad and n != "log_temperature"]
    groups = [dict(params=rest, weight_decay=1e-3)]
    if learnable:
        groups.append(dict(params=[m.log_temperature], weight_decay=0.0))
    return m, AdamW(groups, lr=1e-3)


def batch(B, dev):
    g = torch.Generator().manual_seed(1)
    return {"image": torch.randn((B, 3, 224, 224), generator=g).to(dev),
            "input_ids": torch.randint(5, 300, (B, 25), generator=g).to(dev),
            "attention_mask": torch.ones((B, 25), dtype=torch.int64).to(dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from mae_clip_amd import _lib
    from mae_clip_amd.graph import CapturedStep
    _lib.load()
    dev = torch.device("cuda:0")
    b = batch(a.batch, dev)
    runs, count = {}, {}
    for name, learnable in (("default", False), ("learnable", True)):
        m, opt = build(dev, learnable)
        r = CapturedStep(m, opt)
        t0 = m.current_temperature()
        for _ in range(a.warmup):
            r.step(b)
        torch.cuda.synchronize()
        count[name] = a.warmup
        print(f"{name}: captures {r.captures} after {a.warmup} warm-up steps, loss {r.loss_value():.4f}")
        runs[name] = (r, m, t0)
    ms = {k: [] for k in runs}
    for rd in range(a.rounds):
        for name, (r, m, _) in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                r.step(b)
            e1.record()
            e1.synchronize()
            count[name] += a.steps
            ms[name].append(e0.elapsed_time(e1) / a.steps)
            print(f"round {rd} {name:9s} {ms[name][-1]:8.3f} ms/step over {a.steps} steps")
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(f"C2 shapes, B = {a.batch}, T = 25, bf16, captured step, {a.rounds} alternating rounds of {a.steps} steps")
    for name, (r, m, t0) in runs.items():
        d = med[name] - med["default"]
        print(f"{name:9s} median {med[name]:8.3f} ms/step  vs default {d:+.3f} ms ({100 * d / med['default']:+.2f} %)  "
              f"captures {r.captures} over {count[name]} steps  tau {t0:.6f} -> {m.current_temperature():.6f}")


if __name__ == "__main__":
    main()
