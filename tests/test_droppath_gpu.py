"""Drop-path on the GPU: the two kernels bit for bit against torch on the scales
of kernels.droppath_scales_host, and classifier.ClassifierModel with
drop_path_rate = 0.5 against the float64 restatement of tests/droppath_ref.py
(loss and every gradient within 1e-3, the project's fp32 parity tolerance),
across micro-batches, in eval mode and in a captured step."""
import gc

import pytest
import torch

from tests.helpers import C0, product_config, same_bits
from tests import droppath_ref

pytestmark = pytest.mark.gpu
KW = {k: v for k, v in C0.items() if k != "batch_size"}      # vit_tiny_patch16 at size 32: n = 5, D = 192, 3 heads
S_IMG, DEPTH, RATE = 32, 3, 0.5
OFFSET, KEY = 5, 7


# ------------------------------------------------------------------- kernels
def pick_seed(B, p, step, k=KEY, offset=OFFSET):
    """(seed, scales [B]) with a kept and a dropped sample among the B (p > 0),
    found on the CPU with the host twin of the draw"""
    from mae_clip_amd import kernels as K
    for seed in range(1000):
        s = K.droppath_scales_host(B, k, p, seed=seed, step=step, sample_offset=offset)
        if p == 0 or (bool((s == 0).any()) and bool((s != 0).any())):
            return seed, s
    raise AssertionError("no seed with a kept and a dropped sample")


def rows(B, n, D, seed, pad=0):
    """f32 [B n, D] values (row stride D + pad)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B * n, D + pad), generator=g)[:, :D]


CASES = [(B, n, D, p, "dense") for B, n, D in ((3, 5, 64), (8, 50, 768), (2, 197, 1024)) for p in (0.0, 0.1, 0.5)]
CASES += [(8, 50, 768, 0.5, "strided"), (3, 5, 64, 0.5, "inplace"), (2, 197, 1024, 0.1, "inplace")]


@pytest.mark.parametrize("B,n,D,p,layout", CASES)
def test_droppath_fwd(dev, B, n, D, p, layout):
    from mae_clip_amd import kernels as K
    step = 3
    seed, s = pick_seed(B, p, step)
    srow = s.repeat_interleave(n)[:, None]                       # [M, 1]
    dropped = (srow == 0).expand(-1, D)
    pad = 12 if layout == "strided" else 0
    resid, branch = rows(B, n, D, 1, pad), rows(B, n, D, 2, pad)
    want = torch.where(dropped, resid, resid + srow * branch)    # two roundings on the CPU
    branch_in = torch.where(dropped, torch.full_like(branch, float("nan")), branch)   # must not be read there
    counter = torch.full((1,), step, dtype=torch.int64, device=dev)
    r_d, b_d = (t.to(dev) if pad == 0 else torch.empty((B * n, D + pad), device=dev).copy_(
        torch.nn.functional.pad(t, (0, pad)))[:, :D] for t in (resid, branch_in))
    assert r_d.stride(0) == D + pad
    out = None if layout == "inplace" else torch.full((B * n, D + pad), 7.0, device=dev)[:, :D]
    got = K.droppath_fwd(r_d, b_d, n, p, KEY, seed=seed, sample_offset=OFFSET, step_ptr=counter, out=out)
    torch.cuda.synchronize()
    assert (got.data_ptr() == b_d.data_ptr()) == (layout == "inplace")
    assert same_bits(got, want), (got.cpu() - want).abs().max()
    assert same_bits(got.cpu()[dropped], resid[dropped])
    if layout != "inplace":      # inputs untouched, and nothing written past a row's D columns
        assert same_bits(r_d, resid) and torch.equal(b_d.cpu().isnan(), dropped)
        if pad:
            assert bool((out.as_strided((B * n, pad), (D + pad, 1), D) == 7.0).all())


@pytest.mark.parametrize("B,n,D,p,layout", [c for c in CASES if c[4] != "inplace"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_droppath_bwd(dev, B, n, D, p, layout, dtype):
    from mae_clip_amd import kernels as K
    step = 5
    seed, s = pick_seed(B, p, step)
    M = B * n
    srow = s.repeat_interleave(n)[:, None]
    dropped = (srow == 0).expand(-1, D)
    pad = 12 if layout == "strided" else 0
    g = rows(B, n, D, 3, pad)
    prod = torch.where(dropped, torch.zeros_like(g), g * srow)            # the fp32 products
    g_in = torch.where(dropped, torch.full_like(g, float("nan")), g)      # must not be read there
    g_d = g_in.to(dev) if pad == 0 else torch.empty((M, D + pad), device=dev).copy_(
        torch.nn.functional.pad(g_in, (0, pad)))[:, :D]
    out = torch.full((M, D + pad), 7.0, device=dev, dtype=dtype)[:, :D] if pad else None
    counter = torch.full((1,), step, dtype=torch.int64, device=dev)
    gs, part = K.droppath_bwd(g_d, n, p, KEY, dtype, seed=seed, sample_offset=OFFSET, step_ptr=counter, out=out)
    torch.cuda.synchronize()
    assert gs.dtype == dtype and part.shape == (K.droppath_partial_rows(M), D) == (-(-M // 64), D)
    assert same_bits(gs, prod.to(dtype)), (gs.float().cpu() - prod).abs().max()
    assert bool((gs.cpu()[dropped] == 0).all())
    if pad:
        assert bool((out.as_strided((M, pad), (D + pad, 1), D) == 7.0).all())
    # column sums: sequential-summation worst case M u sum |x| against the float64 sum, u = 2^-24
    want = prod.double().sum(0)
    bound = M * 2.0 ** -24 * prod.double().abs().sum(0)
    err = (part.double().sum(0).cpu() - want).abs()
    print(f"[droppath_bwd] M{M} D{D} p{p} {dtype}: colsum err / bound max {(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert bool((err <= bound).all())


def test_droppath_bwd_row_ranges_fill_the_same_partials(dev):
    """two launches on the halves of a batch (64-row multiples, whole samples) == one launch: what MicroBatches needs"""
    from mae_clip_amd import kernels as K
    B, n, D, p = 128, 5, 192, 0.5
    seed, s = pick_seed(B, p, 2, offset=0)
    g = rows(B, n, D, 9).to(dev)
    counter = torch.full((1,), 2, dtype=torch.int64, device=dev)
    gs, part = K.droppath_bwd(g, n, p, KEY, torch.bfloat16, seed=seed, step_ptr=counter)
    h = B // 2 * n
    for lo, off in ((0, 0), (h, B // 2)):
        gs_h, part_h = K.droppath_bwd(g[lo:lo + h], n, p, KEY, torch.bfloat16, seed=seed, sample_offset=off, step_ptr=counter)
        assert same_bits(gs_h, gs[lo:lo + h]) and same_bits(part_h, part[lo // 64:(lo + h) // 64])


# --------------------------------------------------------------------- model
def build(dev, precision="fp32", rate=RATE, num_classes=10, seed=0, **cfg):
    from mae_clip_amd.classifier import ClassifierModel
    torch.manual_seed(seed)
    with product_config(precision=precision, **KW, **cfg):
        m = ClassifierModel(num_classes=num_classes, trainable_encoder=True, label_smoothing=0.1, drop_path_rate=rate)
    m.image_encoder.model.blocks = m.image_encoder.model.blocks[:DEPTH]
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():     # a head of unit-size logits, no bias / LayerNorm parameter at its init value
        m.head.weight.normal_(0, 0.5, generator=g)
        for name, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn(p.shape, generator=g))
    return m.to(dev)


def images(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    px = torch.randint(0, 256, (B, 3, S_IMG, S_IMG), generator=g).float() / 255.0
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    return (px - mean) / std


def labels(B, C=10, seed=0):
    return torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(100 + seed))


def model_scales(m, B, step, offset=0):
    """[DEPTH, 2, B] float64 branch scales of model m at device step `step`"""
    from mae_clip_amd import kernels as K
    from mae_clip_amd.modules import drop_path_rates
    rates = drop_path_rates(m.image_encoder.model.drop_path_rate, DEPTH)
    return torch.stack([K.droppath_scales_host(B, [2 * i, 2 * i + 1], rates[i], seed=m.drop_path_seed, step=step,
                                               sample_offset=offset) for i in range(DEPTH)]).double()


def test_fine_tune_matches_float64_restatement(dev):
    """B = 8 at device step 3 (counter and host step advanced before the measured
    step): a backward that read the advanced counter (4) instead of the snapshot
    would scale its gradients by the masks of another step."""
    B, step = 8, 3
    m = build(dev).train()
    m.step_counter.fill_(step)
    m.step = step
    sc = model_scales(m, B, step)
    assert sc.shape == (DEPTH, 2, B) and bool((sc[0] == 1).all())                    # block 0 never drops
    assert bool((sc[1:] == 0).any()) and bool((sc[1:] > 1).any())                    # both outcomes occur
    assert not torch.equal(sc, model_scales(m, B, step + 1))
    img, y = images(B), labels(B)
    loss = m({"image": img.to(dev), "label": y.to(dev)})
    loss.backward()
    torch.cuda.synchronize()
    assert int(m.step_counter.item()) == step + 1 and int(m.step_snaps[step % 8].item()) == step
    P = droppath_ref.params_of(m.state_dict())
    rloss, _ = droppath_ref.classifier_loss(P, img.double(), y, sc, DEPTH, m.image_encoder.model.num_heads, 16, 0.1)
    rloss.backward()
    print(f"[droppath] loss {loss.item():.6f} vs float64 {rloss.item():.6f}")
    assert abs(loss.item() - rloss.item()) < 1e-3, (loss.item(), rloss.item())
    worst = (0.0, None)
    for name, p in m.named_parameters():
        rg = P[name].grad
        assert p.grad is not None and rg is not None, name
        err = (p.grad.double().cpu() - rg).abs().max().item() / (rg.abs().max().item() + 1e-30)
        worst = max(worst, (err, name))
        assert err < 1e-3, (name, err)
    print(f"[droppath] worst gradient error {worst[0]:.2e} ({worst[1]})")
    # without the scales the restatement is somewhere else: the comparison above sees the masks
    # (fc2.bias of the last block: its gradient is the sum of s_b g over the rows)
    P0 = droppath_ref.params_of(m.state_dict())
    l0, _ = droppath_ref.classifier_loss(P0, img.double(), y, torch.ones_like(sc), DEPTH, 3, 16, 0.1)
    l0.backward()
    name = f"image_encoder.model.blocks.{DEPTH - 1}.mlp.fc2.bias"
    assert (P0[name].grad - P[name].grad).abs().max() > 0.1 * P[name].grad.abs().max()


def test_micro_batches_match_whole_batch(dev, opts):
    """bf16, B = 128 (two micro-batches of 64 x 5 rows): stack_microbatches 2 == 1 as
    functions.MicroBatches documents it and test_model_gpu.py checks it without
    drop-path: loss and every weight gradient bitwise equal; bias / LayerNorm
    gradients, whose column partials are summed in another grouping, within
    1e-5 relative L2 -- except proj.bias and fc2.bias of the dropping blocks,
    which come from the drop-path partials (64-row groups in both) and are
    bitwise equal too. Stream-K off as there."""
    opts(GEMM_SK=0)
    from mae_clip_amd import functions as Fn
    B = 128
    batch = {"image": images(B, 5).to(dev), "label": labels(B, seed=5).to(dev)}
    res = {}
    for S in (1, 2):
        with product_config(stack_microbatches=S):
            m = build(dev, "bf16").train()
            assert Fn.microbatch_count(Fn.StackSpec(B=B, n=5, D=192, H=3, eps=1e-6, dtype=torch.bfloat16, wT=[])) == S
            m.step_counter.fill_(2)
            loss = m(batch)
            loss.backward()
            torch.cuda.synchronize()
            res[S] = (loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()})
    (l1, g1), (l2, g2) = res[1], res[2]
    assert same_bits(l1, l2), (l1.item(), l2.item())
    for n, a in g1.items():
        exact = a.dim() >= 2 and "pos_embed" not in n and "token" not in n
        exact = exact or any(n.endswith(f"blocks.{i}.{b}.bias") for i in (1, 2) for b in ("attn.proj", "mlp.fc2"))
        if exact:
            assert torch.equal(a, g2[n]), n
        else:
            e = ((a - g2[n]).norm() / (a.norm() + 1e-30)).item()
            assert e < 1e-5, (n, e)


def test_eval_mode_equals_rate_zero(dev):
    B = 8
    img = images(B, 2).to(dev)
    a = build(dev, rate=RATE).eval().logits(img)
    b = build(dev, rate=0.0).eval().logits(img)
    assert same_bits(a, b)
    c = build(dev, rate=RATE).train().logits(img)      # and training mode does drop
    assert not torch.equal(a, c)


def test_captured_step_redraws(dev):
    """One eager step and three replays of the captured step == four eager steps,
    bit for bit (the comparison of test_classifier_gpu.py); and the three
    replayed losses differ from those of a run whose masks stay those of step 0
    (its forward_tokens gets no step counter): a replay draws anew."""
    from mae_clip_amd import kernels as K
    from mae_clip_amd.graph import CapturedStep
    from mae_clip_amd.optim import AdamW
    B = 8
    batch = {"image": images(B, 4).to(dev), "label": labels(B, seed=4).to(dev)}
    runs = {}
    m = opt = runner = loss = None
    try:
        for mode in ("eager", "captured", "frozen"):
            m = build(dev).train()
            if mode == "frozen":
                vit = m.image_encoder.model
                vit.forward_tokens = lambda *a, _f=vit.forward_tokens, **k: _f(*a, **dict(k, step_ptr=None, bwd_step_ptr=None))
            opt = AdamW(list(m.parameters()), lr=1e-4, weight_decay=1e-3)
            runner = CapturedStep(m, opt, enabled=mode == "captured")
            hist = []
            for _ in range(4):
                loss = runner.step(batch)
                hist.append(loss.detach().clone().cpu())
            loss = None
            runs[mode] = (hist, runner.captures, int(m.step_counter.item()))
    finally:
        m = opt = runner = loss = None
        torch.cuda.synchronize()
        gc.collect()
    sc = [model_scales(build(torch.device("cpu")), B, s) for s in range(4)]
    assert all(not torch.equal(sc[0], s) for s in sc[1:])
    assert runs["captured"][1] == 1 and runs["eager"][1] == 0
    assert runs["eager"][2] == runs["captured"][2] == runs["frozen"][2] == 4
    for k, (le, lc) in enumerate(zip(runs["eager"][0], runs["captured"][0])):
        assert same_bits(le, lc), (k, le.item(), lc.item())
    print("[droppath] captured", [l.item() for l in runs["captured"][0]], "frozen", [l.item() for l in runs["frozen"][0]])
    assert same_bits(runs["captured"][0][0], runs["frozen"][0][0])          # step 0: the same masks
    for k in (1, 2, 3):
        assert not torch.equal(runs["captured"][0][k], runs["frozen"][0][k]), k
