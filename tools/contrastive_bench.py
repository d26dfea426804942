"""InfoNCE and SigLIP (K.contrastive_loss) against the soft-target loss
(K.clip_loss) on the same inputs, in one process.

Per shape (N, gradient rows) at P = 256: the paths run alternately, REPEATS
timed repeats each after WARMUP untimed ones, timed with device events; the
median and the min / max of each path and the workspace each asks for are
printed. Inputs are L2-normalised LayerNorm'd rows, tau = 0.07 (SigLIP: 0.1,
b = -10), every gradient asked for (d theta; d b for SigLIP). Shapes past the
soft loss's N limit, or marked so, time the new kinds alone.

    python tools/contrastive_bench.py [--repeats 7] [--warmup 2] [--out FILE] [--big]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mae_clip_amd import _lib as L            # noqa: E402
from mae_clip_amd import kernels as K         # noqa: E402

P = 256
SHARED = [(256, 256), (2048, 256)]
ALONE = [(8192, 1024)]
BIG = [(32768, 4096)]


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
    ap.add_argument("--big", action="store_true", help="also (32768, 4096), the new kinds alone")
    args = ap.parse_args()
    assert args.repeats >= 5
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}, P = {P}, median of {args.repeats} alternating repeats after "
        f"{args.warmup} warm-up, device events, ms; loss + dI + dT + d theta (+ d b) of the gradient rows")
    say("# N rows | path med min max workspace_MB ...")
    for N, rows in SHARED + ALONE + (BIG if args.big else []):
        gen = torch.Generator().manual_seed(N)
        I = K.l2_normalize(torch.nn.functional.layer_norm(torch.randn((N, P), generator=gen), (P,)).cuda())
        T = K.l2_normalize(torch.nn.functional.layer_norm(torch.randn((N, P), generator=gen), (P,)).cuda())
        th7 = torch.tensor([math.log(0.07)], device="cuda")
        th1 = torch.tensor([math.log(0.1)], device="cuda")
        b = torch.tensor([-10.0], device="cuda")
        gr = (N - rows, rows)
        paths = {}
        if (N, rows) in SHARED:
            paths["soft"] = lambda: K.clip_loss(I, T, 1.0, grad_rows=gr, log_temperature=th7, want_dtemp=True)
        paths["infonce"] = lambda: K.contrastive_loss(I, T, "infonce", 1.0, grad_rows=gr, log_temperature=th7,
                                                      want_dtemp=True)
        paths["siglip"] = lambda: K.contrastive_loss(I, T, "siglip", 1.0, grad_rows=gr, log_temperature=th1,
                                                     logit_bias=b, want_dtemp=True, want_dbias=True)
        lib = L.lib()
        ws = {"soft": lib.maeclip_clip_loss_workspace(N, P, rows), "infonce": lib.maeclip_contrastive_workspace(N, P, rows, 0),
              "siglip": lib.maeclip_contrastive_workspace(N, P, rows, 1)}
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        t = {k: [] for k in paths}
        for _ in range(args.repeats):
            for k, fn in paths.items():
                t[k].append(timed(fn))
        row = f"{N} {rows}"
        for k in paths:
            row += f" | {k} {statistics.median(t[k]):.3f} {min(t[k]):.3f} {max(t[k]):.3f} {ws[k] / 2**20:.2f}"
        say(row)
        if "soft" in paths:
            ms = statistics.median(t["soft"])
            for k in ("infonce", "siglip"):
                margin = max(max(t[k]) - min(t[k]), max(t["soft"]) - min(t["soft"]))
                d = statistics.median(t[k]) - ms
                say(f"#   {k} - soft = {d:+.3f} ms, margin (larger min-max spread) {margin:.3f} ms: "
                    f"{'no slower' if d <= margin else 'SLOWER'}")
        del I, T
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
