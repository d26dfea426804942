"""The trainable text tower (config.text_trainable / TextEncoder(trainable=True))
through the HIP kernels vs the fp64 CPU oracle, whose DistilBERT is plain
autograd torch frozen only by requires_grad = False: the tests flip that flag
on the oracle's text parameters. Runs on the GPU box only."""
import pytest
import torch

from tests.helpers import build_pair, make_batch, record_parity, product_config, C0

pytestmark = pytest.mark.gpu

VITB_C1 = dict(model_name="vit_base_patch16_224", size=224, image_embedding=768, text_layers=6, mask_ratio=0.0)


def _pair(precision, **kw):
    prod, ref = build_pair(precision, text_trainable=True, **kw)
    for p in ref.text_encoder.parameters():
        p.requires_grad_(True)
    assert all(p.requires_grad for p in prod.text_encoder.parameters())
    return prod, ref


def _run(prod, ref, batch, dev):
    loss = prod({k: v.to(dev) for k, v in batch.items()})
    loss.backward()
    rloss = ref({"image": batch["image"].double(), "input_ids": batch["input_ids"],
                 "attention_mask": batch["attention_mask"]})
    rloss.backward()
    return loss, rloss


def _scale_ref(rp, name):
    """The oracle gradient whose size an error in `name` is measured against:
    its own, except for a k_lin.bias. That gradient is identically zero
    (softmax is invariant to a per-query constant; the product returns exact
    zeros), so the oracle holds only fp64 rounding noise there and a relative
    error has no meaning: it is measured on the scale of the layer's q_lin.bias
    gradient, as the image tower's fused qkv.bias does for its k third."""
    if name.endswith("attention.k_lin.bias"):
        return rp[name.replace("k_lin.bias", "q_lin.bias")].grad
    return rp[name].grad


def _grad_errs(prod, ref):
    """max-abs relative error of every trainable gradient (vs the oracle's)."""
    rp = dict(ref.named_parameters())
    out = []
    for name, p in prod.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None and rp[name].grad is not None, name
        rg = rp[name].grad
        scale = _scale_ref(rp, name).abs().max().item() + 1e-30
        out.append(((p.grad.double().cpu() - rg).abs().max().item() / scale, name))
    return sorted(out, reverse=True)


def _word(m):
    return m.text_encoder.model.embeddings.word_embeddings.weight


@pytest.mark.parametrize("pad", [False, True])
def test_c0_text_trainable_parity_fp32(dev, pad):
    """fp32 parity mode, eval (no dropout): loss within 1e-5 relative and every
    gradient, the 30522-row word table included, within the project's fp32
    bound of 1e-3 max-rel. make_batch puts id 0 only at masked positions, where
    HF's padding_idx and the oracle's plain nn.Embedding agree: row 0 is zero."""
    prod, ref = _pair("fp32")
    prod.eval()
    ref.eval()
    loss, rloss = _run(prod, ref, make_batch(8, 32, pad=pad), dev)
    assert abs(loss.item() - rloss.item()) < 1e-5 * max(1.0, abs(rloss.item())), (loss.item(), rloss.item())
    worst = _grad_errs(prod, ref)
    print("worst grad rel err:", worst[:3])
    assert any(n.startswith("text_encoder.") for _, n in worst)
    assert worst[0][0] < 1e-3, worst[:5]
    assert (_word(prod).grad[0] == 0).all()
    assert (_word(ref).grad[0] == 0).all()


def test_c1_text_trainable_parity_fp32(dev):
    """C1 model shapes (6-layer text, T = 25), B = 2, ragged masks."""
    prod, ref = _pair("fp32", **VITB_C1)
    prod.eval()
    ref.eval()
    loss, rloss = _run(prod, ref, make_batch(2, 224, seed=11, pad=True), dev)
    d = abs(loss.item() - rloss.item())
    assert d < 1e-5 * max(1.0, abs(rloss.item())), (loss.item(), rloss.item())
    worst = _grad_errs(prod, ref)
    tw = max(w for w in worst if w[1].startswith("text_encoder."))
    record_parity("c1_text_trainable_fp32_vs_oracle", loss_rel=d / max(1.0, abs(rloss.item())),
                  worst_grad_maxrel=worst[0][0], worst_grad=worst[0][1], worst_text_grad_maxrel=tw[0],
                  worst_text_grad=tw[1])
    assert worst[0][0] < 1e-3, worst[:5]
    assert (_word(prod).grad[0] == 0).all()


# (loss rel, worst text-tower gradient rel-L2) of the bf16 path vs the fp64
# oracle with a trainable text tower: 2x the values measured on MI355X
# (profiles/r07/parity_text_trainable.jsonl: loss 1.61e-4, text gradients
# 1.70e-2 -- layer 5's v_lin.bias -- beside 8.5e-3 for the image tower's worst
# in the same run), as test_model_gpu.BF16_TOL
BF16_TEXT_TOL = (3.3e-4, 3.4e-2)


def test_c1_text_trainable_bf16_vs_oracle(dev):
    """bf16 production path at C1 shapes, B = 4, vs the fp64 oracle."""
    prod, ref = _pair("bf16", **VITB_C1)
    prod.eval()
    ref.eval()
    loss, rloss = _run(prod, ref, make_batch(4, 224, seed=12, pad=True), dev)
    rel = abs(loss.item() - rloss.item()) / max(1.0, abs(rloss.item()))
    rp = dict(ref.named_parameters())
    worst = {"text": (0.0, ""), "image": (0.0, "")}
    for name, p in prod.named_parameters():
        if not p.requires_grad:
            continue
        rg = rp[name].grad
        e = ((p.grad.double().cpu() - rg).norm() / (_scale_ref(rp, name).norm() + 1e-30)).item()
        side = "text" if name.startswith("text_encoder.") else "image" if name.startswith("image_encoder.") else None
        if side and e > worst[side][0]:
            worst[side] = (e, name)
    record_parity("c1_text_trainable_bf16_vs_oracle", loss_rel=rel, worst_text_grad_relL2=worst["text"][0],
                  worst_text_grad=worst["text"][1], worst_image_grad_relL2=worst["image"][0],
                  worst_image_grad=worst["image"][1])
    assert rel < BF16_TEXT_TOL[0], (loss.item(), rloss.item())
    assert worst["text"][0] < BF16_TEXT_TOL[1], worst


def test_text_tower_dropout_gradient_finite_difference(dev):
    """Dropout on, fp32, the C0 text tower alone; loss = a fixed random linear
    readout of the CLS rows. <grad, d> along a fixed direction d vs the central
    difference of the loss along d, the step counter held so that both
    evaluations draw the masks of the analytic pass. The same with dropout off,
    where the analytic gradient is pinned to the oracle: the finite-difference
    noise floor is the same in both, so the dropout-on error may be at most 3x
    the dropout-off error (a wrong mask or scale shows as orders of magnitude)."""
    from mae_clip_amd.modules import TextEncoder
    with product_config(precision="fp32", text_layers=2):
        torch.manual_seed(3)
        enc = TextEncoder(trainable=True).to(dev)
    b = make_batch(8, 32, seed=5, pad=True)
    ids, am = b["input_ids"].to(dev), b["attention_mask"].to(dev)
    gen = torch.Generator().manual_seed(9)
    R = torch.randn((8, 768), generator=gen).to(dev)
    params = list(enc.parameters())
    d = [torch.randn(p.shape, generator=gen).to(dev) * p.detach().abs().mean() for p in params]
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    eps = 1e-2

    def loss():
        return (enc(ids, am, seed=77, step_ptr=step).double() * R.double()).sum()

    errs = {}
    for mode in ("off", "on"):
        enc.train(mode == "on")
        for p in params:
            p.grad = None
        loss().backward()
        ana = sum((p.grad.double() * di.double()).sum().item() for p, di in zip(params, d))
        vals = []
        with torch.no_grad():
            for sgn in (1.0, -1.0):
                for p, di in zip(params, d):
                    p.data.add_(di, alpha=sgn * eps)
                vals.append(loss().item())
                for p, di in zip(params, d):
                    p.data.add_(di, alpha=-sgn * eps)
        fd = (vals[0] - vals[1]) / (2 * eps)
        errs[mode] = abs(fd - ana) / abs(ana)
        print(f"dropout {mode}: analytic {ana:.6e} finite difference {fd:.6e} rel err {errs[mode]:.3e}")
    record_parity("text_tower_fd_gradient", eps=eps, dropout_off_rel=errs["off"], dropout_on_rel=errs["on"])
    assert errs["on"] <= 3 * errs["off"], errs


def test_c0_text_trainable_training_fp32(dev):
    """5 AdamW steps at C0 in fp32 train mode, dropout 0 on both sides (the
    loop of helpers.train_curve): per-step loss within the fp32 train-curve
    bound 1e-4, and the text parameters move."""
    from mae_clip_amd.optim import AdamW
    prod, ref = _pair("fp32", dropout=0.0, text_dropout=0.0, text_attention_dropout=0.0)
    for m in ref.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    prod.train()
    ref.train()
    w0 = {n: p.detach().clone() for n, p in prod.text_encoder.named_parameters()}
    opt_p = AdamW([p for p in prod.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3)
    opt_r = torch.optim.AdamW([p for p in ref.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3)
    for k in range(5):
        b = make_batch(8, 32, seed=40 + k, pad=True)
        lp = prod({kk: v.to(dev) for kk, v in b.items()})
        opt_p.zero_grad()
        lp.backward()
        opt_p.step()
        lr = ref(dict(b, image=b["image"].double()))
        opt_r.zero_grad()
        lr.backward()
        opt_r.step()
        rel = abs(lp.item() - lr.item()) / max(1.0, abs(lr.item()))
        print(f"step {k}: product {lp.item():.6f} oracle {lr.item():.6f} rel {rel:.2e}")
        assert rel < 1e-4, (k, lp.item(), lr.item())
    for n, p in prod.text_encoder.named_parameters():
        if n.endswith("attention.k_lin.bias"):
            # an exactly zero gradient (see _scale_ref) on a bias initialised to zero: it stays there
            assert (p == 0).all(), n
            continue
        assert not torch.equal(p, w0[n]), n


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_captured_step_text_trainable_matches_eager(dev, precision):
    """CapturedStep with a trainable tower == eager: same losses and
    bit-identical weights after the steps, dropout at its default 0.1 so the
    step-keyed masks of the text tower's backward are exercised under replay."""
    from mae_clip_amd.CLIP import CLIPModel
    from mae_clip_amd.optim import AdamW
    from mae_clip_amd.graph import CapturedStep
    kw = {k: v for k, v in C0.items() if k != "batch_size"}
    runs = []
    for captured in (False, True):
        with product_config(precision=precision, text_trainable=True, **kw):
            torch.manual_seed(0)
            m = CLIPModel().to(dev).train()
        assert m.text_encoder.model.dropout_p == 0.1 and m.text_encoder.model.attn_dropout_p == 0.1
        opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3)
        runner = CapturedStep(m, opt, enabled=captured)
        losses = []
        for it in range(4):
            batch = {k: v.to(dev) for k, v in make_batch(8, 32, seed=it, pad=True).items()}
            losses.append(runner.step(batch).item())
        if captured:
            assert runner.captures == 1
        runs.append((losses, m))
    (le, me), (lg, mg) = runs
    assert le == lg, (le, lg)
    for (n1, p1), (n2, p2) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(p1, p2), n1


def test_resume_from_checkpoint_text_trainable(dev, tmp_path):
    """4 steps straight == 2 steps, save, fresh model + optimizer, load, 2
    steps, with a trainable text tower (train mode, dropout on)."""
    from mae_clip_amd.CLIP import CLIPModel
    from mae_clip_amd.optim import AdamW
    from mae_clip_amd.checkpoint import save_checkpoint, load_checkpoint
    kw = {k: v for k, v in C0.items() if k != "batch_size"}
    batch = {k: v.to(dev) for k, v in make_batch(8, 32, pad=True).items()}

    def fresh():
        with product_config(precision="bf16", text_trainable=True, **kw):
            torch.manual_seed(0)
            m = CLIPModel().to(dev).train()
        return m, AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3)

    def steps(m, opt, n):
        out = []
        for _ in range(n):
            opt.zero_grad(set_to_none=True)
            loss = m(batch)
            loss.backward()
            opt.step()
            out.append(loss.item())
        return out

    m, opt = fresh()
    straight = steps(m, opt, 4)
    m2, opt2 = fresh()
    first = steps(m2, opt2, 2)
    path = tmp_path / "ckpt.pt"
    save_checkpoint(path, m2, opt2)
    m3, opt3 = fresh()
    assert load_checkpoint(path, m3, opt3, map_location=dev) == 2
    assert len(opt3.state) == sum(1 for p in m3.parameters() if p.requires_grad)
    resumed = first + steps(m3, opt3, 2)
    assert resumed == straight, (resumed, straight)
    for (k, a), b in zip(m.state_dict().items(), m3.state_dict().values()):
        assert torch.equal(a, b), k

