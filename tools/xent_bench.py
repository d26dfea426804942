"""Softmax cross-entropy forward + backward: the fused kernels (K.xent_fwd +
K.xent_bwd) against torch's F.cross_entropy forward + backward on the same
device and inputs, in one process.

Per shape (M, C, ld), hard labels, label_smoothing = 0.1: the two paths run
alternately, REPEATS timed repeats each after WARMUP untimed ones, timed with
device events; the median and the min / max of each are printed, and for the
fused path the bytes the algorithm needs (the logits read twice, the gradient
written once: 3 * 4 * M * C) over the median time.

    python tools/xent_bench.py [--repeats 7] [--warmup 2] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mae_clip_amd import kernels as K         # noqa: E402

SHAPES = [(256, 1000, 1000), (1024, 1000, 1000), (4096, 21843, 21844)]
EPS = 0.1


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}, median of {args.repeats} alternating repeats after {args.warmup} warm-up, "
        f"device events, ms; forward + backward, hard labels, label_smoothing {EPS}")
    say("# M C ld | path med min max ... | fused GB/s over 12 M C bytes")
    for M, C, ld in SHAPES:
        gen = torch.Generator().manual_seed(M + C)
        buf = torch.zeros((M, ld), device="cuda")
        buf[:, :C] = torch.randn((M, C), generator=gen).cuda()
        y = torch.randint(0, C, (M,), generator=gen).cuda()
        out = torch.empty_like(buf)
        xt = buf[:, :C].detach().requires_grad_(True)     # torch reads the same strided rows

        def fused():
            o = K.xent_fwd(buf, y, C=C, label_smoothing=EPS)
            K.xent_bwd(buf, o.lse, y, C=C, label_smoothing=EPS, lse_lo=o.lse_lo, out=out)

        def eager():
            xt.grad = None
            F.cross_entropy(xt, y, label_smoothing=EPS).backward()

        paths = {"fused": fused, "torch": eager}
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        # same numbers first: faster and different is not faster
        o = K.xent_fwd(buf, y, C=C, label_smoothing=EPS)
        ref = F.cross_entropy(xt, y, label_smoothing=EPS)
        err = abs(o.loss.item() - ref.item()) / abs(ref.item())
        gerr = ((out[:, :C] - xt.grad).abs().max() / xt.grad.abs().max()).item()
        t = {k: [] for k in paths}
        for _ in range(args.repeats):
            for k, fn in paths.items():
                t[k].append(timed(fn))
        row = f"{M} {C} {ld}"
        for k in paths:
            row += f" | {k} {statistics.median(t[k]):.4f} {min(t[k]):.4f} {max(t[k]):.4f}"
        gbs = 12.0 * M * C / (statistics.median(t["fused"]) * 1e-3) / 1e9
        say(row + f" | {gbs:.0f}")
        margin = max(max(t["fused"]) - min(t["fused"]), max(t["torch"]) - min(t["torch"]))
        d = statistics.median(t["fused"]) - statistics.median(t["torch"])
        say(f"#   fused - torch = {d:+.4f} ms, margin (larger min-max spread) {margin:.4f} ms: "
            f"{'no slower' if d <= margin else 'SLOWER'}; loss rel diff {err:.1e}, grad diff / max {gerr:.1e}")
        del buf, out, xt
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
