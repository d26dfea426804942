"""Drop-path: the two kernels against maeclip_rows_colsum (the existing kernel
that moves the same bytes as the backward: fp32 rows in, a bf16 copy and column
partials out), and the fine-tuning step with and without drop-path.

Kernels, at the fine-tuning shape M = 256 x 197, D = 768, bf16 compute dtype,
timed the way bench.py's launch timer times a launch inside the captured step:
ONE launch between two maeclip_timestamp launches on its stream (the device's
REALTIME counter, maeclip_wallclock_khz ticks per ms), so a span is the kernel
plus its two launch boundaries. (bench.py's timer itself hangs on
kernels.LAUNCH_HOOK, which only the GEMM wrappers call.) The kernels take turns,
SAMPLES spans each after WARMUP untimed rounds; before every span a 512 MiB
buffer is overwritten, so every launch starts from cold caches (the inputs of a
launch fit the 256 MiB Infinity Cache), and the in-place forward gets its
branch buffer restored. Per kernel: the median, min and max span and the bytes
the algorithm needs over the median (forward 12 M D: two fp32 reads, one fp32
write; backward and rows_colsum 6 M D: one fp32 read, one bf16 write; the
partials are < 2 % more).

Step: classifier.ClassifierModel(ViT-B/16 @224, 1000 classes, trainable
encoder), B = 256, bf16, AdamW, graph.CapturedStep, at drop_path_rate 0 and
0.1, alternating windows of STEPS replays between device events.

    python tools/droppath_bench.py [--samples 30] [--repeats 9] [--no-step] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mae_clip_amd import _lib                 # noqa: E402
from mae_clip_amd import config as CFG        # noqa: E402
from mae_clip_amd import kernels as K         # noqa: E402

B, N, D = 256, 197, 768
STEPS = 5


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


class Stamps:
    """spans of single launches between two device timestamps on the current stream"""

    def __init__(self, slots):
        self.ts = torch.zeros(2 * slots, dtype=torch.int64, device="cuda")
        self.keys = []

    def span(self, key, fn):
        lib, st, i = _lib.lib(), torch.cuda.current_stream().cuda_stream, len(self.keys)
        _lib.check(lib.maeclip_timestamp(self.ts.data_ptr() + 16 * i, st), "maeclip_timestamp")
        fn()
        _lib.check(lib.maeclip_timestamp(self.ts.data_ptr() + 16 * i + 8, st), "maeclip_timestamp")
        self.keys.append(key)

    def us(self):
        """{key: [span in us, ...]} (one device-to-host read)"""
        khz = float(_lib.lib().maeclip_wallclock_khz()) or 100000.0
        t = self.ts.cpu().view(-1, 2)
        out = {}
        for i, key in enumerate(self.keys):
            out.setdefault(key, []).append(1e3 * float(t[i, 1] - t[i, 0]) / khz)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    M = B * N
    say(f"# {torch.cuda.get_device_name(0)}; M = {B} x {N} = {M}, D = {D}; {args.samples} spans per kernel, the kernels "
        f"taking turns, after {args.warmup} warm-up rounds; one launch between two device timestamps, cold caches, us")
    gen = torch.Generator().manual_seed(0)
    g = torch.randn((M, D), generator=gen).cuda()
    resid = torch.randn((M, D), generator=gen).cuda()
    branch = torch.randn((M, D), generator=gen).cuda()
    gT = torch.empty((M, D), device="cuda", dtype=torch.bfloat16)
    gs = torch.empty((M, D), device="cuda", dtype=torch.bfloat16)
    part = torch.empty((K.droppath_partial_rows(M), D), device="cuda")
    counter = torch.full((1,), 3, dtype=torch.int64, device="cuda")
    kw = dict(seed=7, step_ptr=counter)
    paths = {
        "rows_colsum+bf16": (lambda: K.rows_colsum(g, out_bf16=gT), 6),
        "droppath_bwd p=0.1": (lambda: K.droppath_bwd(g, N, 0.1, 3, torch.bfloat16, out=gs, partial=part, **kw), 6),
        "droppath_bwd p=0": (lambda: K.droppath_bwd(g, N, 0.0, 3, torch.bfloat16, out=gs, partial=part, **kw), 6),
        "droppath_fwd p=0.1": (lambda: K.droppath_fwd(resid, branch, N, 0.1, 2, **kw), 12),
        "droppath_fwd p=0": (lambda: K.droppath_fwd(resid, branch, N, 0.0, 2, **kw), 12),
    }
    branch0 = branch.clone()
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    stamps = Stamps(args.samples * len(paths))
    for r in range(args.warmup + args.samples):
        for k, (fn, _) in paths.items():
            if "fwd" in k:
                branch.copy_(branch0)
            flush.zero_()
            if r < args.warmup:
                fn()
            else:
                stamps.span(k, fn)
    torch.cuda.synchronize()
    t = stamps.us()
    med = {k: statistics.median(v) for k, v in t.items()}
    say("# kernel | med min max us | TB/s over the algorithm's bytes (at p = 0.1 a tenth of the rows reads nothing)")
    for k, (_, nb) in paths.items():
        say(f"{k} | {med[k]:.2f} {min(t[k]):.2f} {max(t[k]):.2f} | {nb * M * D / (med[k] * 1e-6) / 1e12:.2f}")
    y = "rows_colsum+bf16"
    say(f"# droppath_bwd p=0 / rows_colsum = {med['droppath_bwd p=0'] / med[y]:.3f}, p=0.1: "
        f"{med['droppath_bwd p=0.1'] / med[y]:.3f}; rows_colsum's own min-max spread {(max(t[y]) - min(t[y])) / med[y]:.3f}")
    del g, resid, branch, branch0, flush, gT, gs, part
    torch.cuda.empty_cache()

    if not args.no_step:
        from mae_clip_amd.classifier import ClassifierModel
        from mae_clip_amd.graph import CapturedStep
        from mae_clip_amd.optim import AdamW
        CFG.model_name, CFG.size, CFG.image_embedding, CFG.precision = "vit_base_patch16_224", 224, 768, "bf16"
        gen = torch.Generator().manual_seed(1)
        batch = {"image": torch.randn((B, 3, 224, 224), generator=gen).cuda(),
                 "label": torch.randint(0, 1000, (B,), generator=gen).cuda()}
        runners = {}
        for rate in (0.0, 0.1):
            torch.manual_seed(0)
            m = ClassifierModel(num_classes=1000, trainable_encoder=True, label_smoothing=0.1, drop_path_rate=rate).cuda().train()
            opt = AdamW(list(m.parameters()), lr=1e-4, weight_decay=0.05)
            r = CapturedStep(m, opt)
            for _ in range(4):      # one eager step, the capture, replays
                r.step(batch)
            torch.cuda.synchronize()
            runners[rate] = r
        ts = {rate: [] for rate in runners}
        for _ in range(args.repeats):
            for rate, r in runners.items():
                ts[rate].append(timed(lambda: r.step(batch), STEPS))
        say(f"# fine-tuning step, ViT-B/16 @224, B = {B}, bf16, captured; median of {args.repeats} alternating windows of "
            f"{STEPS} replays, ms per step")
        for rate in runners:
            say(f"drop_path_rate {rate} | {statistics.median(ts[rate]):.3f} {min(ts[rate]):.3f} {max(ts[rate]):.3f}")
        d = statistics.median(ts[0.1]) - statistics.median(ts[0.0])
        say(f"# rate 0.1 - rate 0 = {d * 1e3:+.0f} us per step (11 dropping blocks x 4 launches)")
        runners.clear()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
