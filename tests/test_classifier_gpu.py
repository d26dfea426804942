"""classifier.ClassifierModel on the GPU against the fp64 CPU oracle: the C0
encoder (vit_tiny_patch16_224 at size 32, depth 2) in fp32, B = 5, with
oracle.ref_model.ImageEncoder in double on the same weights + torch.nn.Linear +
F.cross_entropy. Bounds are those of test_model_gpu.py: loss |d| < 1e-3, every
trainable gradient within 1e-3 of the reference's max |grad|."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests.helpers import C0, oracle_config, product_config, same_bits

pytestmark = pytest.mark.gpu
KW = {k: v for k, v in C0.items() if k != "batch_size"}
B, S, DEPTH = 5, 32, 2


class RefClassifier(nn.Module):
    def __init__(self, num_classes):
        super().__init__()
        from oracle.ref_model import ImageEncoder
        self.image_encoder = ImageEncoder(oracle_config(vit_depth=DEPTH, **C0))
        self.head = nn.Linear(self.image_encoder.model.embed_dim, num_classes)

    def logits(self, img):
        return self.head(self.image_encoder.model(img))


def build(dev, num_classes, trainable, eps, seed=0):
    """(ClassifierModel on the device, the oracle in double) with one set of weights"""
    from mae_clip_amd.classifier import ClassifierModel
    torch.manual_seed(seed)
    with product_config(precision="fp32", **KW):
        m = ClassifierModel(num_classes=num_classes, trainable_encoder=trainable, label_smoothing=eps)
    m.image_encoder.model.blocks = m.image_encoder.model.blocks[:DEPTH]
    with torch.no_grad():     # a head away from its near-zero initialisation: logits of unit size
        m.head.weight.normal_(0, 0.5)
        m.head.bias.normal_(0, 0.5)
    ref = RefClassifier(num_classes)
    ref.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, strict=True)
    return m.to(dev), ref.double()


def images(seed=0, n=B):
    g = torch.Generator().manual_seed(seed)
    px = torch.randint(0, 256, (n, 3, S, S), generator=g).float() / 255.0
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    return (px - mean) / std


def labels(C, seed=0, n=B):
    return torch.randint(0, C, (n,), generator=torch.Generator().manual_seed(100 + seed))


def check_grads(m, ref, what):
    rp = dict(ref.named_parameters())
    worst = (0.0, None)
    for name, p in m.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, name
            continue
        assert p.grad is not None and rp[name].grad is not None, name
        rg = rp[name].grad
        err = (p.grad.double().cpu() - rg).abs().max().item() / (rg.abs().max().item() + 1e-30)
        worst = max(worst, (err, name))
        assert err < 1e-3, (what, name, err)
    print(f"[classifier] {what}: worst gradient error {worst[0]:.2e} ({worst[1]})")


@pytest.mark.parametrize("label_dtype", [torch.int64, torch.int32])
def test_fine_tune_matches_oracle(dev, label_dtype):
    C, eps = 10, 0.1                       # 10 classes on 12 columns inside
    m, ref = build(dev, C, True, eps)
    img, y = images(), labels(C)
    loss = m({"image": img.to(dev), "label": y.to(dev, label_dtype)})
    loss.backward()
    rloss = F.cross_entropy(ref.logits(img.double()), y, label_smoothing=eps)
    rloss.backward()
    assert abs(loss.item() - rloss.item()) < 1e-3, (loss.item(), rloss.item())
    assert all(p.requires_grad for p in m.parameters())
    check_grads(m, ref, "fine-tune")
    assert set(m.last_losses) == {"xent"} and m.last_losses["xent"].item() == loss.item()


class Recorder:
    """libmaeclip with the name of every call noted before it runs"""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def test_linear_probe_matches_oracle(dev, monkeypatch):
    from mae_clip_amd import _lib
    C = 7                                  # odd: 8 columns inside
    m, ref = build(dev, C, False, 0.0)
    img, y = images(1), labels(C, 1)
    loss = m({"image": img.to(dev), "label": y.to(dev)})
    rec = Recorder(_lib.load())
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "lib", lambda: rec)
        loss.backward()
        torch.cuda.synchronize()
    rloss = F.cross_entropy(ref.logits(img.double()), y)
    rloss.backward()
    assert abs(loss.item() - rloss.item()) < 1e-3, (loss.item(), rloss.item())
    assert sorted(n for n, p in m.named_parameters() if p.grad is not None) == ["head.bias", "head.weight"]
    check_grads(m, ref, "linear probe")
    # only the head's launches in the backward: the loss gradient, dW, db
    names = rec.calls
    assert names.count("maeclip_xent_bwd") == 1
    assert set(names) <= {"maeclip_xent_bwd", "maeclip_gemm", "maeclip_gemm_workspace", "maeclip_gemm_splitk",
                          "maeclip_rows_colsum",
                          "maeclip_rows_colsum_partial_rows", "maeclip_colsum_reduce", "maeclip_colsum_scratch"}, names


def test_soft_targets_match_oracle(dev):
    C, eps = 10, 0.1
    m, ref = build(dev, C, True, eps)
    img = images(2)
    g = torch.Generator().manual_seed(5)
    t = torch.softmax(torch.randn(B, C, generator=g) * 2, -1)
    # "label" is ignored when "target" is there
    loss = m({"image": img.to(dev), "target": t.to(dev), "label": torch.zeros(B, dtype=torch.int64, device=dev)})
    loss.backward()
    rloss = F.cross_entropy(ref.logits(img.double()), t.double(), label_smoothing=eps)
    rloss.backward()
    assert abs(loss.item() - rloss.item()) < 1e-3, (loss.item(), rloss.item())
    check_grads(m, ref, "soft targets")


def test_uint8_batch_equals_normalised_batch(dev):
    from mae_clip_amd.data import normalize_u8
    m, _ = build(dev, 10, False, 0.1)
    m.eval()
    g = torch.Generator().manual_seed(3)
    px = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    y = labels(10, 3).to(dev)
    with torch.no_grad():
        a = m({"image": px, "label": y}).item()
        b = m({"image": normalize_u8(px), "label": y}).item()
    assert abs(a - b) <= 1e-6 * abs(b), (a, b)


@pytest.mark.parametrize("trainable", [False, True])
def test_captured_step_matches_eager(dev, trainable):
    """Four AdamW steps on one repeated batch: the captured graph equals the eager
    steps bit for bit, and the loss goes down.

    Learning rates: Adam's first steps move every weight by about lr whatever
    the gradient's size, four times in the same direction on a repeated batch.
    The probe trains a head whose weights this file draws at scale 0.5: lr =
    config.lr = 1e-3. Fine-tuning also moves the encoder, whose weights are
    trunc-normal(0.02): 1e-3 is 5 % of their scale per step and overshoots, so
    lr = 1e-4, the size of MAE's fine-tuning rates.

    The runners leave through `finally`: a CapturedStep owns pinned host memory
    (kernels.HostScalars) whose release is a HIP call, and a failing assert
    would keep this frame, and with it the runner, alive in pytest's traceback;
    a later test that forks (multiprocessing.Manager) would then collect it in
    the child, where HIP cannot be called."""
    import gc
    from mae_clip_amd.graph import CapturedStep
    from mae_clip_amd.optim import AdamW
    C = 10
    batch = {"image": images(4).to(dev), "label": labels(C, 4).to(dev)}
    runs = []
    m = opt = runner = None
    try:
        for captured in (False, True):
            m, _ = build(dev, C, trainable, 0.1)
            m.train()
            opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4 if trainable else 1e-3,
                        weight_decay=1e-3)
            runner = CapturedStep(m, opt, enabled=captured)
            hist = []
            for _ in range(4):
                loss = runner.step(batch)
                hist.append((loss.detach().clone().cpu(), m.head.weight.detach().clone().cpu()))
            loss = None
            captures, steps = runner.captures, (m.step, int(m.step_counter.item()))
            runs.append((hist, captures, steps))
    finally:
        m = opt = runner = loss = None
        torch.cuda.synchronize()
        gc.collect()
    for (hist, captures, steps), captured in zip(runs, (False, True)):
        assert (captures == 1) == captured and steps == (4, 4)
    for k, ((le, we), (lg, wg)) in enumerate(zip(runs[0][0], runs[1][0])):
        assert same_bits(le, lg), (k, le.item(), lg.item())
        assert same_bits(we, wg), k
    losses = [l.item() for l, _ in runs[1][0]]
    print(f"[classifier] captured step, trainable={trainable}: losses {losses}")
    assert all(b < a for a, b in zip(losses, losses[1:])), losses


def test_evaluate_matches_topk_on_the_cpu(dev):
    from mae_clip_amd.classifier import evaluate
    C = 10
    m, _ = build(dev, C, False, 0.1)       # the smoothing is training's: evaluate reports plain cross-entropy
    m.eval()
    batches = [{"image": images(10 + k, n).to(dev), "label": labels(C, 10 + k, n).to(dev)} for k, n in ((0, 5), (1, 3))]
    res = evaluate(m, batches, ks=(1, 5))
    hits = {1: 0, 5: 0}
    tot, n = 0.0, 0
    for b in batches:
        lg = m.logits(b["image"]).cpu().double()
        assert lg.shape == (len(b["label"]), C)
        srt = lg.sort(1).values
        assert (srt[:, 1:] - srt[:, :-1]).min().item() > 0, "the inputs must have no ties"
        y = b["label"].cpu()
        for k in hits:
            hits[k] += (lg.topk(k, 1).indices == y.view(-1, 1)).any(1).sum().item()
        tot += F.cross_entropy(lg, y, reduction="sum").item()
        n += len(y)
    assert res["n"] == n == 8
    assert res["top1"] == hits[1] / n and res["top5"] == hits[5] / n
    assert abs(res["loss"] - tot / n) <= 1e-5 * abs(tot / n), (res["loss"], tot / n)
    assert all(p.grad is None for p in m.parameters())


def test_checkpoint_round_trip(dev, tmp_path):
    from mae_clip_amd.checkpoint import load_checkpoint, save_checkpoint
    from mae_clip_amd.optim import AdamW
    C = 10
    batch = {"image": images(6).to(dev), "label": labels(C, 6).to(dev)}

    def make(seed):
        m, _ = build(dev, C, True, 0.1, seed=seed)
        m.train()
        return m, AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3)

    def step(m, opt):
        opt.zero_grad(set_to_none=True)
        loss = m(batch)
        loss.backward()
        opt.step()
        return loss.detach().clone()

    m, opt = make(0)
    step(m, opt)
    step(m, opt)
    path = str(tmp_path / "probe.pt")
    save_checkpoint(path, m, opt)
    m2, opt2 = make(1)                      # other weights, replaced by the load
    assert load_checkpoint(path, m2, opt2) == 2 and m2.step == 2 and int(m2.step_counter.item()) == 2
    for (n1, p1), (n2, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert n1 == n2 and same_bits(p1, p2), n1
    a, b = step(m, opt), step(m2, opt2)
    assert same_bits(a, b), (a.item(), b.item())
    a, b = step(m, opt), step(m2, opt2)     # and the step after it: the optimizer state came along
    assert same_bits(a, b), (a.item(), b.item())
