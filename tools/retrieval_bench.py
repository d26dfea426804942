"""Fused similarity + top-k (retrieval.similarity_topk) against the unfused
pair topk_rows(similarity(...)) on the same inputs, in one process.

Per shape (Q, N, k) at P = 256: both paths run alternately, REPEATS timed
repeats each after WARMUP untimed ones, timed with device events; the median
and the min / max of each path, the split count the fused call took and the
peak memory each path added on top of its inputs are printed.

    python tools/retrieval_bench.py [--repeats 7] [--warmup 2] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mae_clip_amd import _lib as L                                           # noqa: E402
from mae_clip_amd.retrieval import similarity, similarity_topk, topk_rows    # noqa: E402

SHAPES = [(25000, 5000, 10), (5000, 25000, 10), (1, 100000, 45), (10000, 1000, 5)]
P = 256


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    del out
    return grown


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

    say(f"# {torch.cuda.get_device_name(0)}, P = {P}, median of {args.repeats} alternating repeats after "
        f"{args.warmup} warm-up, device events, ms (normalisation included in both paths)")
    say("# Q N k splits | fused med min max | unfused med min max | unfused/fused | peak MB fused unfused")
    for Q, N, k in SHAPES:
        gen = torch.Generator().manual_seed(Q + N)
        q = torch.randn((Q, P), generator=gen).cuda()
        g = torch.randn((N, P), generator=gen).cuda()
        fused = lambda: similarity_topk(q, g, k)
        unfused = lambda: topk_rows(similarity(q, g), k)
        S = L.lib().maeclip_sim_topk_splits(Q, N, P, k, 0)
        fv, fi = fused()
        uv, ui = unfused()
        same = (fi == ui).float().mean().item()
        dv = (fv - uv).abs().max().item()
        del fv, fi, uv, ui
        for _ in range(args.warmup):
            fused()
            unfused()
        tf, tu = [], []
        for _ in range(args.repeats):
            tf.append(timed(fused))
            tu.append(timed(unfused))
        pf, pu = peak(fused), peak(unfused)
        mf, mu = statistics.median(tf), statistics.median(tu)
        say(f"{Q} {N} {k} {S} | {mf:.3f} {min(tf):.3f} {max(tf):.3f} | {mu:.3f} {min(tu):.3f} {max(tu):.3f} | "
            f"{mu / mf:.2f} | {pf / 2**20:.1f} {pu / 2**20:.1f}   (indices equal {same:.4f}, max |dval| {dv:.1e})")
        del q, g
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
