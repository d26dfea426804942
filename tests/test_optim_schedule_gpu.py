"""Device-resident learning rate and fused global-norm gradient clipping
(optim.AdamW(device_lr=..., max_grad_norm=...)) on the GPU: the
norm kernels against fp64, the clip and the device lr inside the AdamW kernel
without a tolerance, one captured graph under a per-batch schedule, and parity
with clip_grad_norm_ + torch.optim.AdamW on the fp64 oracle."""
import math

import pytest
import torch

from tests.test_model_gpu import build_pair
from tests.helpers import make_batch, product_config, C0

pytestmark = pytest.mark.gpu

# chunk edges of the 4096-element plan, a tail, several entries per search
SIZES = (1, 3, 4095, 4096, 4097, 3 * 4096 + 5, 70001)
UNALIGNED = 4      # SIZES[4] starts one element into its buffer: not 16-byte aligned


def _tensors(dev, seed, scale=1.0, zero=False):
    """f32 device tensors of SIZES, magnitudes spread over 1e-3 .. 1e3"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(SIZES):
        x = torch.randn(n, generator=g) * 10.0 ** (6.0 * torch.rand(n, generator=g) - 3.0) * scale
        if zero:
            x.zero_()
        if i == UNALIGNED:
            x = torch.cat([torch.zeros(1), x]).to(dev)[1:]
            assert x.data_ptr() % 16 == 4
        else:
            x = x.to(dev)
        out.append(x)
    return out


def _norm64(ts):
    return math.sqrt(sum(float(t.double().pow(2).sum().item()) for t in ts))


def _grad_plan(K, ts):
    return K.MultiTensorPlan([(None, t.data_ptr(), None, None, None, t.numel()) for t in ts], ts[0].device)


def _norm_and_coef(K, ts, max_norm):
    plan = _grad_plan(K, ts)
    nb = K.mt_blocks(plan)
    assert nb == sum((n + 4095) // 4096 for n in SIZES)
    # a second range of the same buffer: the offset argument, and nothing written outside [off, off + nb)
    partials = torch.full((2 * nb + 3,), -7.0, device=ts[0].device)
    norm = torch.empty(1, device=ts[0].device)
    coef = torch.empty(1, device=ts[0].device)
    assert K.sumsq_multi(plan, partials, nb + 2) == nb
    K.clip_coef(partials[nb + 2:], nb, max_norm, norm, coef)
    torch.cuda.synchronize()
    assert bool((partials[:nb + 2] == -7.0).all()) and bool((partials[2 * nb + 2:] == -7.0).all())
    return norm, coef, partials


def test_norm_kernels_against_fp64(dev):
    from mae_clip_amd import kernels as K
    ts = _tensors(dev, 0)
    ref = _norm64(ts)
    for max_norm, clipped in ((0.37 * ref, True), (1.5 * ref, False)):
        norm, coef, partials = _norm_and_coef(K, ts, max_norm)
        rel = abs(norm.item() - ref) / ref
        want = min(1.0, max_norm / (ref + 1e-6))
        print(f"norm {norm.item()!r} fp64 {ref!r} rel {rel:.3e}; coef {coef.item()!r} want {want!r}")
        assert rel < 1e-5, (norm.item(), ref)
        if clipped:
            assert want < 1.0 and abs(coef.item() - want) < 1e-5, (coef.item(), want)
        else:
            assert coef.item() == 1.0
        # a second run: bitwise equal partials, norm and coefficient
        norm2, coef2, partials2 = _norm_and_coef(K, ts, max_norm)
        assert torch.equal(partials, partials2) and torch.equal(norm, norm2) and torch.equal(coef, coef2)
    norm, coef, _ = _norm_and_coef(K, _tensors(dev, 0, zero=True), 1.0)
    assert norm.item() == 0.0 and coef.item() == 1.0


def _params_like(ts):
    """fresh parameters with the storage layout of `ts` (the unaligned view included)"""
    ps = []
    for i, t in enumerate(ts):
        if i == UNALIGNED:
            buf = torch.zeros(t.numel() + 1, device=t.device)
            buf[1:].copy_(t)
            ps.append(torch.nn.Parameter(buf[1:]))
            assert ps[-1].data_ptr() % 16 == 4
        else:
            ps.append(torch.nn.Parameter(t.clone()))
    return ps


def _assert_same_state(opt_a, ps_a, opt_b, ps_b, what):
    for i, (a, b) in enumerate(zip(ps_a, ps_b)):
        assert torch.equal(a, b), (what, "param", i)
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt_a.state[a][key], opt_b.state[b][key]), (what, key, i)


def test_clip_inside_adamw_is_exact(dev):
    """AdamW(max_grad_norm=c) on g == default AdamW on g * clip_coef (an fp32
    multiply in torch), bit for bit; the step that does not clip == the plain
    default path on g."""
    from mae_clip_amd.optim import AdamW
    init = _tensors(dev, 10, scale=1e-3)
    grads = [_tensors(dev, 11), _tensors(dev, 12, scale=0.1), _tensors(dev, 13, scale=2.0)]
    n64 = [_norm64(g) for g in grads]
    c = 0.5 * n64[0]
    # conditions on the inputs: step 1 and 3 clip, step 2 does not
    assert n64[0] > c * 1.01 and n64[1] + 1e-6 < c * 0.99 and n64[2] > c * 1.01, (n64, c)
    pa, pb = _params_like(init), _params_like(init)
    kw = dict(lr=1e-2, weight_decay=1e-2)
    oa, ob = AdamW(pa, max_grad_norm=c, **kw), AdamW(pb, **kw)
    for k, gs in enumerate(grads):
        for p, g in zip(pa, gs):
            p.grad = g
        before = [g.clone() for g in gs]
        oa.step()
        coef = oa.clip_coef.clone()
        # p.grad is not rescaled (the documented difference from clip_grad_norm_)
        assert all(torch.equal(g, b) for g, b in zip(gs, before))
        assert abs(oa.grad_norm.item() - n64[k]) / n64[k] < 1e-5
        if k == 1:
            assert coef.item() == 1.0
            for p, g in zip(pb, gs):
                p.grad = g                    # the plain default path
        else:
            assert coef.item() < 1.0
            for i, (p, g) in enumerate(zip(pb, gs)):
                p.grad = g * coef
                if i == UNALIGNED:            # same storage alignment on both sides
                    buf = torch.zeros(g.numel() + 1, device=dev)
                    buf[1:].copy_(g * coef)
                    p.grad = buf[1:]
        ob.step()
        _assert_same_state(oa, pa, ob, pb, f"step {k + 1}")
    assert not torch.equal(pa[-1], init[-1])


def test_device_lr_is_exact(dev):
    """two groups, both rates changed every step: device_lr == by-value lr, bit for bit"""
    from mae_clip_amd.optim import AdamW
    init = _tensors(dev, 20, scale=1e-3)
    pa, pb = _params_like(init), _params_like(init)

    def groups(ps):
        return [{"params": ps[:3], "lr": 3e-3}, {"params": ps[3:], "lr": 7e-4, "weight_decay": 0.05}]
    oa, ob = AdamW(groups(pa), weight_decay=1e-2, device_lr=True), AdamW(groups(pb), weight_decay=1e-2)
    for k in range(5):
        gs = _tensors(dev, 30 + k, scale=1e-2)
        for o in (oa, ob):
            o.param_groups[0]["lr"] = 3e-3 * (0.7 ** k) + 1e-7 * k
            o.param_groups[1]["lr"] = 7e-4 * (k + 1) / 3.0
        for ps in (pa, pb):
            for p, g in zip(ps, gs):
                p.grad = g
        oa.step()
        ob.step()
        _assert_same_state(oa, pa, ob, pb, f"step {k + 1}")
        want = torch.tensor([g["lr"] for g in oa.param_groups], dtype=torch.float32)
        assert torch.equal(oa._lr_dev.cpu(), want)
    assert isinstance(oa.param_groups[0]["lr"], float)
    assert not torch.equal(pa[-1], init[-1])


def _schedule(opt, steps=8, warm=3):
    def f(s):
        return (s + 1) / warm if s < warm else 0.5 * (1.0 + math.cos(math.pi * (s - warm) / (steps - warm)))
    return torch.optim.lr_scheduler.LambdaLR(opt, f)


def _scheduled_run(dev, precision, captured, steps=8, **opt_kw):
    from mae_clip_amd.CLIP import CLIPModel
    from mae_clip_amd.optim import AdamW
    from mae_clip_amd.graph import CapturedStep
    kw = {k: v for k, v in C0.items() if k != "batch_size"}
    with product_config(precision=precision, **kw):
        torch.manual_seed(0)
        m = CLIPModel().to(dev).train()
    opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3, **opt_kw)
    sched = _schedule(opt, steps)
    runner = CapturedStep(m, opt, enabled=captured)
    losses, lrs = [], []
    for it in range(steps):
        batch = {k: v.to(dev) for k, v in make_batch(8, 32, seed=it).items()}
        lrs.append(opt.param_groups[0]["lr"])
        losses.append(runner.step(batch).item())
        sched.step()     # per batch: the reference's `if step == "batch": lr_scheduler.step()`
    return losses, lrs, m, opt, runner


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_captured_step_under_per_batch_schedule(dev, precision):
    """warm-up + cosine stepped after every batch, with clipping: ONE capture,
    and the replays equal the eager run of the same sequence (losses step by
    step, final parameters and the last gradient norm bitwise). Control: the
    default optimizer re-captures under the same schedule."""
    feature = dict(device_lr=True, max_grad_norm=1.0)
    le, lrs_e, me, oe, _ = _scheduled_run(dev, precision, False, **feature)
    lg, lrs_g, mg, og, rg = _scheduled_run(dev, precision, True, **feature)
    # the rate changes before every step but one (end of warm-up == start of the cosine)
    assert len(set(lrs_e)) == 7 and lrs_e == lrs_g
    assert rg.captures == 1
    assert le == lg, (le, lg)
    assert len(set(le)) == 8, le
    for (n1, p1), (n2, p2) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(p1, p2), n1
    assert torch.equal(oe.grad_norm, og.grad_norm) and torch.equal(oe.clip_coef, og.clip_coef)
    assert math.isfinite(og.grad_norm.item()) and og.grad_norm.item() > 0.0
    # the behaviour this replaces, unchanged for the default optimizer
    _, _, _, _, rc = _scheduled_run(dev, precision, True)
    assert rc.captures > 1, rc.captures


def test_clipped_training_curve_vs_oracle(dev):
    """test_training_curve_fp32's set-up with clipping and a per-step lr: the
    oracle runs clip_grad_norm_(ref.parameters(), c) before torch.optim.AdamW."""
    from mae_clip_amd.optim import AdamW
    prod, ref = build_pair("fp32")
    prod.eval()
    ref.eval()
    ropt = torch.optim.AdamW([p for p in ref.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3)
    batch = make_batch(8, 32)
    bd = {k: v.to(dev) for k, v in batch.items()}
    rb = {"image": batch["image"].double(), "input_ids": batch["input_ids"], "attention_mask": batch["attention_mask"]}
    lrs = [1e-3, 8e-4, 6e-4, 4e-4, 2e-4]
    opt, c, active = None, None, 0
    for it in range(5):
        ropt.zero_grad()
        rl = ref(rb)
        rl.backward()
        if opt is None:
            # half the oracle's own first-step norm: clipping is active on step 0
            c = 0.5 * math.sqrt(sum(float(p.grad.pow(2).sum()) for p in ref.parameters() if p.grad is not None))
            opt = AdamW([p for p in prod.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3,
                        max_grad_norm=c, device_lr=True)
        for o in (opt, ropt):
            o.param_groups[0]["lr"] = lrs[it]
        rnorm = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), c))
        ropt.step()
        active += rnorm > c
        opt.zero_grad()
        l = prod(bd)
        l.backward()
        opt.step()
        gn = opt.grad_norm.item()
        print(f"step {it}: loss {l.item():.6f} oracle {rl.item():.6f}; norm {gn:.6f} oracle {rnorm:.6f} c {c:.6f}")
        assert abs(l.item() - rl.item()) < 1e-3, (it, l.item(), rl.item())
        assert abs(gn - rnorm) / rnorm < 1e-3, (it, gn, rnorm)
    assert active >= 1
