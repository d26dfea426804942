"""Cost of training the text tower: frozen vs trainable DistilBERT, same box.

usage: python tools/text_trainable_probe.py [--batch 256] [--steps 20] [--rounds 3] [--warmup 5]
       python tools/text_trainable_probe.py --trace [--steps 4]

C1 model shapes (ViT-B/16 @224, mask 0, 6-layer text, T = 25), bf16, the whole
step (forward, backward, fused AdamW) as a captured HIP graph
(graph.CapturedStep). The two models live side by side and are timed in
alternating blocks of `--steps` steps (HIP events around each block), `--rounds`
times, after `--warmup` steps each (the eager step and the capture among them),
so that clock and thermal drift hit both alike. Prints every block, the medians
and the difference.

--trace: the trainable model only, `--steps` eager steps and nothing else, for
a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -o tt -- python tools/text_trainable_probe.py --trace
    python tools/step_kernels.py DIR/.../tt_kernel_trace.csv 2
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C1 = dict(model_name="vit_base_patch16_224", size=224, image_embedding=768, text_layers=6, mask_ratio=0.0)


def build(trainable, dev):
    from mae_clip_amd import config as CFG
    from mae_clip_amd.CLIP import CLIPModel
    from mae_clip_amd.optim import AdamW
    old = {k: getattr(CFG, k) for k in list(C1) + ["precision", "text_trainable"]}
    try:
        for k, v in dict(C1, precision="bf16", text_trainable=trainable).items():
            setattr(CFG, k, v)
        torch.manual_seed(0)
        m = CLIPModel().to(dev).train()
    finally:
        for k, v in old.items():
            setattr(CFG, k, v)
    opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3)
    return m, opt


def batch(B, dev):
    g = torch.Generator().manual_seed(1)
    return {"image": torch.randn((B, 3, 224, 224), generator=g).to(dev),
            "input_ids": torch.randint(5, 300, (B, 25), generator=g).to(dev),
            "attention_mask": torch.ones((B, 25), dtype=torch.int64).to(dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    from mae_clip_amd import _lib
    from mae_clip_amd.graph import CapturedStep
    _lib.load()
    dev = torch.device("cuda:0")
    b = batch(a.batch, dev)
    if a.trace:
        m, opt = build(True, dev)
        run = CapturedStep(m, opt, enabled=False)
        for _ in range(a.steps or 4):
            run.step(b)
        torch.cuda.synchronize()
        print(f"traced {a.steps or 4} eager trainable steps, loss {run.loss_value():.4f}")
        return
    steps = a.steps or 20
    runs = {}
    for name, tr in (("frozen", False), ("trainable", True)):
        m, opt = build(tr, dev)
        r = CapturedStep(m, opt)
        for _ in range(a.warmup):
            r.step(b)
        torch.cuda.synchronize()
        n = sum(p.numel() for p in m.parameters() if p.requires_grad)
        print(f"{name}: {n / 1e6:.1f} M trainable parameters, captures {r.captures}, loss {r.loss_value():.4f}")
        runs[name] = r
    ms = {k: [] for k in runs}
    for rd in range(a.rounds):
        for name, r in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                r.step(b)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / steps)
            print(f"round {rd} {name:9s} {ms[name][-1]:8.3f} ms/step over {steps} steps")
    f, t = statistics.median(ms["frozen"]), statistics.median(ms["trainable"])
    print(f"C1 shapes, B = {a.batch}, T = 25, bf16, captured step, {a.rounds} alternating rounds of {steps} steps")
    print(f"median ms/step: frozen {f:.3f}  trainable {t:.3f}  difference {t - f:+.3f} ms ({100 * (t - f) / f:+.1f} %)")
    print(f"images/s: frozen {a.batch / f * 1e3:.0f}  trainable {a.batch / t * 1e3:.0f}")


if __name__ == "__main__":
    main()
