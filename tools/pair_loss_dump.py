"""Every output of the three pair losses, the fused similarity top-k and the
L2 normalisation on fixed seeded inputs, as .npy files in one directory.

Run once per build of libmaeclip.so (MAECLIP_LIB selects the library), each in
a process of its own, then compare the two directories: a refactor of these
kernels must leave every array bit-equal.

    python tools/pair_loss_dump.py DIR
    python tools/pair_loss_dump.py --compare DIR_A DIR_B      (no GPU needed)
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NS = (1, 17, 40, 300)          # partial last tile, several tiles per wave, several j-splits
PS = (64, 128, 256, 512)
NAMES = ("loss", "dI", "dT", "row_loss", "dtheta", "dbias")


def dump(out):
    import torch
    from mae_clip_amd import kernels as K
    from mae_clip_amd.retrieval import similarity_topk
    os.makedirs(out, exist_ok=True)

    def save(tag, names, tensors):
        for n, t in zip(names, tensors):
            np.save(os.path.join(out, f"{tag}.{n}.npy"), t.detach().cpu().numpy())

    def rows(N, P, seed):
        g = torch.Generator().manual_seed(seed)
        return torch.nn.functional.layer_norm(torch.randn((N, P), generator=g), (P,)).cuda()

    theta = torch.tensor([math.log(0.07)], device="cuda")
    bias = torch.tensor([-10.0], device="cuda")
    for N in NS:
        for P in PS:
            I, T = K.l2_normalize(rows(N, P, 1000 * N + P)), K.l2_normalize(rows(N, P, 1000 * N + P + 1))
            for sl in (None,) + (((16, 20),) if N == 40 else ()):
                tag = f"N{N}_P{P}_{'all' if sl is None else 'slice'}"
                kw = dict(grad_rows=sl, row_loss=True)
                # theta by value, then by pointer with its gradient
                save(f"soft_val_{tag}", NAMES, K.clip_loss(I, T, 0.07, **kw))
                save(f"soft_ptr_{tag}", NAMES, K.clip_loss(I, T, 1.0, log_temperature=theta, want_dtemp=True, **kw))
                save(f"infonce_val_{tag}", NAMES, K.contrastive_loss(I, T, "infonce", 0.07, **kw))
                save(f"infonce_ptr_{tag}", NAMES,
                     K.contrastive_loss(I, T, "infonce", 1.0, log_temperature=theta, want_dtemp=True, **kw))
                save(f"siglip_val_{tag}", NAMES, K.contrastive_loss(I, T, "siglip", 0.1, **kw))
                save(f"siglip_ptr_bias_{tag}", NAMES,
                     K.contrastive_loss(I, T, "siglip", 1.0, log_temperature=theta, logit_bias=bias, want_dtemp=True,
                                        want_dbias=True, **kw))
    # the guarded k-group path (P = 48 < 64) and the full one; one slice and three
    ql, gl = torch.arange(70, device="cuda") % 7, torch.arange(100, device="cuda") % 7
    for P in (48, 64):
        q, g = rows(70, P, 7000 + P), rows(100, P, 7100 + P)
        for S in (1, 3):
            save(f"topk_P{P}_S{S}", ("vals", "idx", "first_hit"),
                 similarity_topk(q, g, 5, query_labels=ql, gallery_labels=gl, splits=S))
    for P in (64, 100):
        x, gy = rows(5, P, 9000 + P), rows(5, P, 9100 + P)
        x[3] = 0.0   # the eps branch
        save(f"l2_P{P}", ("y", "dx"), (K.l2_normalize(x), K.l2_normalize_bwd(x, gy)))
    torch.cuda.synchronize()
    print(f"{len(os.listdir(out))} arrays -> {out}")


def compare(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    bad = sorted(set(fa) ^ set(fb))
    for f in sorted(set(fa) & set(fb)):
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        # bit-equal: same dtype and shape, same bytes (NaN payloads and zero signs included)
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes() or not np.array_equal(x, y, equal_nan=True):
            bad.append(f)
    print(f"{len(fa)} / {len(fb)} arrays, {len(bad)} differ or are missing" + "".join("\n  " + f for f in bad))
    return 1 if bad or not fa else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(sys.argv[1])
