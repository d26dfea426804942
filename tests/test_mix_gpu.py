"""Mixup / CutMix on the device (mix.hip maeclip_mix_params / maeclip_mix_images
/ maeclip_mix_targets, data.MixAugment, data.Chain, graph.CapturedStep).

Pixels and targets are compared bit for bit with tests/mix_ref.py on
hand-written records; the device draw with the library's own host evaluation
of the same function under the rule of test_mix_draw_cpu.py; the transform with
its parts; the captured step with the eager one."""
import gc

import numpy as np
import pytest
import torch

from tests.mix_ref import CUTMIX, MIXUP, NONE, lams, make_records, mix_images_ref, mix_params_ref, mix_targets_ref
from tests.test_mix_draw_cpu import ALPHAS, OFFSETS, PROB, SEED, SIZES, STEPS, SWITCH, check_against, host

pytestmark = pytest.mark.gpu
B = 5


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _same(got, ref_np):
    ref = torch.from_numpy(np.ascontiguousarray(ref_np))
    return got.shape == ref.shape and torch.equal(_bits(got), _bits(ref))


def _record_sets(S):
    """hand-written records, five samples a set (B = 5 is odd: sample 2 pairs with itself)"""
    third = float(np.float32(1.0) / np.float32(3.0))
    flip = [4, 3, 2, 1, 0]
    return {
        "none and mixup": [(NONE, 4, 0, 0, 0, 0, 1.0, 1.0), (MIXUP, 3, 0, 0, 0, 0, 0.0, 0.0),
                           (MIXUP, 2, 0, 0, 0, 0, 1.0, 1.0), (MIXUP, 1, 0, 0, 0, 0, 0.5, 0.5),
                           (MIXUP, 0, 0, 0, 0, 0, 0.3, 0.3)],
        # 0.5 again with another partner (odd sums round half to even), 1/3, 0.5 with itself
        "mixup": [(MIXUP, 1, 0, 0, 0, 0, 0.5, 0.5), (MIXUP, 3, 0, 0, 0, 0, third, third), (MIXUP, 2, 0, 0, 0, 0, 0.5, 0.5),
                  (MIXUP, 0, 3, 3, 9, 9, 0.7, 0.1), (NONE, 0, 1, 1, 9, 9, 0.25, 0.25)],   # box / lam of no concern there
        "cutmix shapes": [(CUTMIX, 4, 7, 9, 7, 20, 1.0, 1.0),              # empty (x1 == x0)
                          (CUTMIX, 3, 0, 0, S, S, 1.0, 0.0),              # the whole image
                          (CUTMIX, 2, 3, 3, 9, 9, 1.0, 0.9),              # with itself
                          (CUTMIX, 1, 13, 2, 14, S - 3, 1.0, 0.9),        # one pixel wide
                          (CUTMIX, 0, 5, 11, S - 2, 12, 1.0, 0.9)],       # one pixel high
        "cutmix borders": [(CUTMIX, 4, 0, 0, 7, 5, 1.0, 0.9),             # left and top
                           (CUTMIX, 3, S - 6, S - 9, S, S, 1.0, 0.9),     # right and bottom
                           (CUTMIX, 2, 0, 6, S, 19, 1.0, 0.9),            # full rows
                           (CUTMIX, 1, 5, 3, 11, S - 1, 1.0, 0.9),        # edges at 5 and 11: inside a 16-byte piece
                           (CUTMIX, 0, 1, 1, 2, 2, 1.0, 0.9)],            # a single pixel
        "clamped": [(CUTMIX, 4, -5, -3, 9, 8, 1.0, 0.9),                  # over the left / top border
                    (CUTMIX, 3, S - 4, S - 5, S + 40, S + 7, 1.0, 0.9),   # over the right / bottom border
                    (CUTMIX, 2, 9, 9, 3, 3, 1.0, 0.9),                    # x1 < x0: empty
                    (CUTMIX, 77, 2, 2, 12, 12, 1.0, 0.9),                 # partner past B - 1: the last sample
                    (MIXUP, -3, 0, 0, 0, 0, 0.25, 0.25)],                 # partner < 0: sample 0
    }, flip


def _arena(shape, dtype, dev, offset_elems, seed):
    """(view of `shape` at offset_elems inside a larger allocation of random bytes, the allocation)"""
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        raw = torch.randint(0, 256, (n + 2 * offset_elems + 64,), generator=g, dtype=torch.uint8)
    else:   # finite floats of every sign and size the normalised pixels take
        raw = (torch.randint(0, 256, (n + 2 * offset_elems + 64,), generator=g).float() / 255.0 - 0.45) / 0.225
    raw = raw.to(dev)
    return raw[offset_elems:offset_elems + n].view(shape), raw


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("S,offset", [(32, 64), (30, 64), (32, 3)], ids=["S32", "S30", "S32-unaligned"])
def test_pixels_bit_exact(dev, dtype, S, offset):
    """S = 32 at a 16-byte offset: the 16-byte path; S = 30: uint8 samples of
    2700 bytes take single elements, fp32 samples of 10800 bytes 16-byte pieces
    that cross rows and planes; offset 3 elements: single elements at S = 32."""
    from mae_clip_amd import data
    shape = (B, S, S, 3) if dtype == torch.uint8 else (B, 3, S, S)
    src, _ = _arena(shape, dtype, dev, offset, seed=S + offset)
    esz = src.element_size()
    assert (src.data_ptr() % 16 == 0) == ((offset * esz) % 16 == 0)
    src_np = src.cpu().numpy()
    sets, _ = _record_sets(S)
    for name, rows in sets.items():
        rec = make_records(rows)
        ref = mix_images_ref(src_np, rec)
        dst, raw = _arena(shape, dtype, dev, offset, seed=1000 + S)
        before = raw.clone()
        out = data.mix_images(src, torch.from_numpy(rec).to(dev), out=dst)
        assert out.data_ptr() == dst.data_ptr()
        bad = [b for b in range(B) if not _same(dst[b], ref[b])]
        assert not bad, (name, "samples differ", bad)
        n = dst.numel()
        assert torch.equal(_bits(raw[:offset]), _bits(before[:offset])), (name, "bytes before dst changed")
        assert torch.equal(_bits(raw[offset + n:]), _bits(before[offset + n:])), (name, "bytes behind dst changed")
        assert torch.equal(_bits(src), torch.from_numpy(src_np).view(_bits(src).dtype)), (name, "src changed")
    # the reference itself distinguishes the cases
    whole = mix_images_ref(src_np, make_records(sets["cutmix shapes"]))
    assert np.array_equal(whole[1], src_np[3]) and np.array_equal(whole[0], src_np[0])
    if dtype == torch.uint8:
        half = mix_images_ref(src_np, make_records(sets["mixup"]))[0].astype(np.int64)
        s = src_np[0].astype(np.int64) + src_np[1]
        odd = s % 2 == 1
        assert odd.sum() > 100 and np.array_equal(half[odd] % 2, np.zeros(odd.sum(), dtype=np.int64))   # ties went to even


def test_two_calls_give_the_same_bits_and_default_out(dev):
    from mae_clip_amd import data
    sets, _ = _record_sets(32)
    src, _ = _arena((B, 3, 32, 32), torch.float32, dev, 64, seed=7)
    rec = torch.from_numpy(make_records(sets["none and mixup"])).to(dev)
    a, b = data.mix_images(src, rec), data.mix_images(src, rec)
    assert a.data_ptr() != b.data_ptr() and torch.equal(_bits(a), _bits(b))
    with pytest.raises(Exception, match="dst overlaps src"):
        data.mix_images(src, rec, out=src)


@pytest.mark.parametrize("C", [5, 10, 1000])
@pytest.mark.parametrize("label_dtype", [torch.int64, torch.int32], ids=["i64", "i32"])
def test_targets_bit_exact(dev, C, label_dtype):
    from mae_clip_amd import data
    third = float(np.float32(1.0) / np.float32(3.0))
    #          own == partner's label (samples 0 and 4), itself (2), a label out of range (3 -> partner 1 sees it)
    labels = np.asarray([3, C - 1, 0, C + 1, 3], dtype=np.int64)
    rec = make_records([(MIXUP, 4, 0, 0, 0, 0, 0.3, 0.3), (CUTMIX, 3, 0, 0, 4, 4, 1.0, 0.8125),
                        (MIXUP, 2, 0, 0, 0, 0, third, third), (NONE, 1, 0, 0, 0, 0, 1.0, 1.0),
                        (CUTMIX, 9, 0, 0, 4, 4, 1.0, third)])       # partner 9 -> 4: itself
    for ld_t in (C, (C + 3) // 4 * 4 + 4):
        ref = mix_targets_ref(labels, rec, C, ld_t)
        assert ref[0, 3] == 1 and ref[4, 3] == 1 and ref[2, 0] == 1
        assert ref[3].sum() == np.float32(0) and ref[1, C - 1] == np.float32(0.8125) and ref[1].sum() == np.float32(0.8125)
        assert (ref[:, C:] == 0).all()
        raw = torch.full((B * ld_t + 32,), 7.0, device=dev)
        out = raw[16:16 + B * ld_t].view(B, ld_t)
        y = torch.from_numpy(labels).to(dev, label_dtype)
        got = data.mix_targets(y, torch.from_numpy(rec).to(dev), C, out=out)
        assert _same(got, ref), (C, ld_t)
        assert (raw[:16] == 7).all() and (raw[16 + B * ld_t:] == 7).all()
    # default out is [B, C]; an odd base address takes the scalar stores
    assert _same(data.mix_targets(y, torch.from_numpy(rec).to(dev), C), mix_targets_ref(labels, rec, C))
    raw = torch.full((B * C + 8,), 7.0, device=dev)
    got = data.mix_targets(y, torch.from_numpy(rec).to(dev), C, out=raw[1:1 + B * C].view(B, C))
    assert _same(got, mix_targets_ref(labels, rec, C)) and raw[0] == 7 and (raw[1 + B * C:] == 7).all()


def test_device_draw_matches_host_draw(dev):
    """device libm against host libm, under the rule of the CPU test"""
    from mae_clip_amd import data
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    excluded = total = 0
    n = 512
    for al in ALPHAS:
        for hw in SIZES:
            for mode in (0, 1):
                for step in STEPS:
                    counter.fill_(step)
                    off = OFFSETS[step % 2]
                    got = data.mix_params(n, hw[0], hw[1], al[0], al[1], PROB, SWITCH, mode, SEED, counter, off).cpu().numpy()
                    want = host(n, hw[0], hw[1], al[0], al[1], PROB, SWITCH, mode, SEED, step, off)
                    k = 1 if mode == 0 else n          # batch mode: one draw, flagged once
                    _, near = mix_params_ref(k, hw[0], hw[1], al[0], al[1], PROB, SWITCH, mode, SEED, step, off)
                    near = np.repeat(near, n) if mode == 0 else near
                    excluded += check_against(got, want, near, (al, hw, mode, step))
                    total += n
    print(f"near-tie samples excluded: {excluded} of {total}")
    assert excluded <= 0.01 * total, (excluded, total)
    # step_ptr None is step 0; `device` says where
    a = data.mix_params(8, 32, 32, seed=SEED, mode="elem", device=dev).cpu().numpy()
    assert np.array_equal(a[:, :2], host(8, 32, 32, seed=SEED)[:, :2])


# ------------------------------------------------------------------ end to end
C, EPS, S = 10, 0.1, 32


def _raw(dev):
    from tests.test_classifier_gpu import labels
    g = torch.Generator().manual_seed(21)
    sizes = torch.tensor([[48, 56], [40, 33], [17, 50], [48, 20], [33, 33]], dtype=torch.int32)
    return {"image": torch.randint(0, 256, (B, 48, 56, 3), generator=g, dtype=torch.uint8).to(dev),
            "image_sizes": sizes.to(dev), "label": labels(C, 8).to(dev)}


def _chain(mode, **kw):
    from mae_clip_amd import data
    aug = data.TrainAugment(S, seed=3)
    mix = data.MixAugment(C, 0.8, 1.0, kw.get("prob", 1.0), 0.5, mode, seed=SEED)
    return data.Chain(aug, mix), aug, mix


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_transform_is_only_its_parts(dev, mode):
    from mae_clip_amd import data
    from tests.test_classifier_gpu import build
    raw = _raw(dev)
    m, _ = build(dev, C, True, EPS)
    m.train()
    m.step_counter.fill_(2)
    chain, aug, mix = _chain(mode)
    fed = chain(raw, m.step_counter, 0)
    assert set(fed) == {"image", "label", "target"} and fed["label"] is raw["label"]
    assert fed["image"].dtype == torch.uint8 and fed["image"].shape == (B, S, S, 3) and fed["target"].shape == (B, C)
    loss = m(fed)
    loss.backward()
    rec = mix.params.clone()
    rec_np = rec.cpu().numpy()
    assert np.array_equal(rec_np[:, :2], host(B, S, S, mode=mix.mode, step=2)[:, :2])
    assert _same(mix.out, mix_images_ref(aug.out.cpu().numpy(), rec_np))
    assert _same(mix.target, mix_targets_ref(raw["label"].cpu().numpy(), rec_np, C))
    # the same model fed the parts
    m2, _ = build(dev, C, True, EPS)
    m2.train()
    m2.step_counter.fill_(2)
    parts = {"image": data.mix_images(aug.out, rec), "target": data.mix_targets(raw["label"], rec, C)}
    loss2 = m2(parts)
    loss2.backward()
    assert torch.equal(_bits(loss), _bits(loss2)), (loss.item(), loss2.item())
    for (n1, p1), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert p1.grad is not None and torch.equal(_bits(p1.grad), _bits(p2.grad)), n1
    # timm: mixup_target(smoothing) + SoftTargetCrossEntropy on the logits
    lg = m.logits(parts["image"]).double().cpu()
    y = raw["label"].cpu()
    lam = torch.from_numpy(lams(rec_np)[1].astype(np.float64)).view(B, 1)
    off, on = EPS / C, 1.0 - EPS + EPS / C
    partner = torch.from_numpy(rec_np[:, 1].astype(np.int64))
    y1 = torch.full((B, C), off, dtype=torch.float64).scatter_(1, y.view(-1, 1), on)
    y2 = torch.full((B, C), off, dtype=torch.float64).scatter_(1, y[partner].view(-1, 1), on)
    t = y1 * lam + y2 * (1.0 - lam)
    want = torch.sum(-t * torch.log_softmax(lg, -1), -1).mean().item()
    print(f"[mix] {mode}: loss {loss.item():.6f}, timm formula {want:.6f}, kinds {rec_np[:, 0].tolist()}")
    assert abs(loss.item() - want) < 1e-3, (loss.item(), want)


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_captured_step_matches_eager(dev, mode):
    """Four AdamW steps through Chain(TrainAugment, MixAugment): the replayed graph
    equals the eager steps bit for bit and mixes anew on every replay. (The
    runners leave through `finally`, as in test_classifier_gpu.py.)"""
    from mae_clip_amd.graph import CapturedStep
    from mae_clip_amd.optim import AdamW
    from tests.test_classifier_gpu import build
    raw = _raw(dev)
    runs = []
    m = opt = runner = loss = None
    try:
        for captured in (False, True):
            m, _ = build(dev, C, True, EPS)
            m.train()
            opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-3)
            chain, aug, mix = _chain(mode)
            runner = CapturedStep(m, opt, enabled=captured, transform=chain)
            hist = []
            for _ in range(4):
                loss = runner.step(raw)
                hist.append((loss.detach().clone().cpu(), m.head.weight.detach().clone().cpu(), mix.params.cpu().numpy().copy(),
                             mix.out.cpu().clone(), mix.target.cpu().clone()))
            loss = None
            runs.append((hist, runner.captures, (m.step, int(m.step_counter.item()))))
    finally:
        m = opt = runner = loss = None
        torch.cuda.synchronize()
        gc.collect()
    for (hist, captures, steps), captured in zip(runs, (False, True)):
        assert (captures == 1) == captured and steps == (4, 4)
    for k, (e, g) in enumerate(zip(runs[0][0], runs[1][0])):
        assert torch.equal(_bits(e[0]), _bits(g[0])), (k, e[0].item(), g[0].item())
        assert torch.equal(_bits(e[1]), _bits(g[1])), k
        assert np.array_equal(e[2], g[2]) and torch.equal(e[3], g[3]) and torch.equal(_bits(e[4]), _bits(g[4])), k
        assert np.array_equal(g[2][:, :2], host(B, S, S, mode=0 if mode == "batch" else 1, step=k)[:, :2]), k
    recs = [g[2] for g in runs[1][0]]
    for k in range(1, 4):
        assert not np.array_equal(recs[k], recs[k - 1]), k
    assert all(np.isfinite(g[0].item()) for g in runs[1][0])
