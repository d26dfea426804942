"""Softmax cross-entropy and the classifier without a GPU: the ABI of the new
entry points, the argument rejections of maeclip_xent_fwd / maeclip_xent_bwd on
the real library (every check comes before any launch, so the host pointers
handed in are never dereferenced on a device; a call that got past its checks
would fail differently, "launch failed", which is why each case also looks at
the message), the config flags, ClassifierModel's state_dict, load_image_encoder
and a stubbed-launch plumbing run of probe and fine-tuning. The kernels are
compared with fp64 references in test_xent_gpu.py, the model in
test_classifier_gpu.py."""
import ctypes
import os
import re

import pytest
import torch

from mae_clip_amd import _lib as L
from tests.helpers import C0, make_batch, product_config
from tests.test_plumbing_cpu import stubbed_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUF = (ctypes.c_float * 64)()
P = ctypes.addressof(_BUF) // 16 * 16 + 16      # a 16-byte aligned host address
KW = {k: v for k, v in C0.items() if k != "batch_size"}


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_abi_and_symbols(lib):
    assert lib.maeclip_abi_version() == 14 and L.ABI_VERSION == 14
    for name, nargs in (("maeclip_xent_workspace", 1), ("maeclip_xent_fwd", 2), ("maeclip_xent_bwd", 3)):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(L._SIGS[name][1]) == nargs, name
    assert L._SIGS["maeclip_xent_workspace"][0] is ctypes.c_size_t
    names = [f[0] for f in L.XentArgs._fields_]
    assert names == ["logits", "ld", "labels", "label_dtype", "soft_targets", "targets", "ld_t", "M", "C",
                     "label_smoothing", "loss_scale", "loss", "row_loss", "lse", "lse_lo", "rank", "dlogits", "ld_d",
                     "workspace", "ws_bytes"]
    # the same fields, in the same order, as the header's struct
    src = open(os.path.join(ROOT, "include", "maeclip.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\}\s*maeclip_xent_args;", src, re.S).group(1)
    decl = [d.strip() for d in body.split(";") if d.strip()]
    header = [re.sub(r"[\s*]", "", v) for d in decl for v in d.split(",")]
    header = [re.sub(r"^(const)?(float|void|int32_t|int64_t|size_t)", "", h) for h in header]
    assert header == names
    assert lib.maeclip_xent_workspace(1) >= 4 and lib.maeclip_xent_workspace(1000) >= 4000
    assert lib.maeclip_xent_workspace(1000) % 16 == 0


def test_path_bounds_match_the_kernel_file():
    """test_xent_gpu.py straddles these: they are the constants of xent.hip"""
    from mae_clip_amd import kernels as K
    src = open(os.path.join(ROOT, "mae_clip_amd", "csrc", "xent.hip")).read()
    assert int(re.search(r"constexpr int XENT_REG_COLS = (\d+);", src).group(1)) == K.XENT_REG_COLS
    assert int(re.search(r"constexpr int XENT_WAVE_COLS = (\d+);", src).group(1)) == K.XENT_WAVE_COLS


def _args(**kw):
    """a valid small hard-target call (forward and backward fields); kw overrides"""
    d = dict(logits=P, ld=8, labels=P, label_dtype=0, soft_targets=0, targets=None, ld_t=0, M=4, C=8,
             label_smoothing=0.1, loss_scale=1.0, loss=P, row_loss=None, lse=P, lse_lo=P, rank=None, dlogits=P, ld_d=8,
             workspace=P, ws_bytes=1 << 10)
    d.update(kw)
    return L.XentArgs(**d)


BOTH, FWD, BWD = ("fwd", "bwd"), ("fwd",), ("bwd",)
CASES = {
    "null args": (None, b"null pointer", BOTH),
    "null logits": (dict(logits=None), b"null pointer", BOTH),
    "no loss": (dict(loss=None), b"null pointer", FWD),
    "no lse": (dict(lse=None), b"null pointer", BOTH),
    "no dlogits": (dict(dlogits=None), b"null pointer", BWD),
    "M 0": (dict(M=0), b"M must be in", BOTH),
    "C 0": (dict(C=0, ld=0, ld_d=0), b"C must be in", BOTH),
    "C -3": (dict(C=-3), b"C must be in", BOTH),
    "C 2^31": (dict(C=1 << 31, ld=1 << 31, ld_d=1 << 31), b"C must be in", BOTH),
    "ld < C": (dict(ld=7), b"ld must be >= C", BOTH),
    "ld_d < C": (dict(ld_d=7), b"ld_d must be >= C", BWD),
    "ld_t < C": (dict(soft_targets=1, targets=P, labels=None, ld_t=4), b"ld_t must be >= C", BOTH),
    "eps 1": (dict(label_smoothing=1.0), b"label_smoothing must be in [0, 1)", BOTH),
    "eps < 0": (dict(label_smoothing=-0.01), b"label_smoothing must be in [0, 1)", BOTH),
    "eps nan": (dict(label_smoothing=float("nan")), b"label_smoothing must be in [0, 1)", BOTH),
    "neither labels nor targets": (dict(labels=None), b"exactly one of labels / targets", BOTH),
    "soft without targets": (dict(soft_targets=1), b"exactly one of labels / targets", BOTH),
    "hard with targets too": (dict(targets=P, ld_t=8), b"exactly one of labels / targets", BOTH),
    "soft_targets 2": (dict(soft_targets=2), b"soft_targets must be 0 or 1", BOTH),
    "label_dtype 3": (dict(label_dtype=3), b"label_dtype must be", BOTH),
    "misaligned logits": (dict(logits=P + 2), b"4-byte aligned", BOTH),
    "misaligned targets": (dict(soft_targets=1, targets=P + 1, ld_t=8), b"4-byte aligned", BOTH),
    "int64 labels on 4 bytes": (dict(labels=P + 4, label_dtype=1), b"8-byte aligned", BOTH),
    "misaligned dlogits": (dict(dlogits=P + 3), b"4-byte aligned", BOTH),
    "rank without labels": (dict(soft_targets=1, targets=P, ld_t=8, labels=None, rank=P), b"rank needs labels", FWD),
    "no workspace": (dict(workspace=None), b"workspace too small or misaligned", FWD),
    "short workspace": (dict(ws_bytes=8), b"workspace too small or misaligned", FWD),
    "misaligned workspace": (dict(workspace=P + 4), b"workspace too small or misaligned", FWD),
    "in place with another stride": (dict(ld=12, ld_d=8), b"in place needs ld_d == ld", BWD),
    "misaligned grad_output": (dict(), b"grad_output must be 4-byte aligned", BWD),
}


@pytest.mark.parametrize("case,which", [(c, w) for c in CASES for w in CASES[c][2]])
def test_xent_rejects(lib, case, which):
    kw, what, _ = CASES[case]
    a = None if kw is None else _args(**kw)
    ref = ctypes.byref(a) if a is not None else None
    if which == "fwd":
        rc = lib.maeclip_xent_fwd(ref, None)
    else:
        rc = lib.maeclip_xent_bwd(ref, P + 2 if case == "misaligned grad_output" else None, None)
    msg = lib.maeclip_last_error()
    assert rc == -1, (rc, msg)
    assert what in msg and b"launch failed" not in msg, msg
    assert (b"maeclip_xent_fwd" if which == "fwd" else b"maeclip_xent_bwd") in msg, msg


def test_config_defaults():
    from mae_clip_amd import config as CFG
    assert CFG.num_classes == 1000 and CFG.label_smoothing == 0.0
    assert CFG.classifier_trainable_encoder is False and CFG.head_init_std == 0.02


def _classifier(**kw):
    from mae_clip_amd.classifier import ClassifierModel
    with product_config(precision="fp32", side_stream=False, **KW):
        torch.manual_seed(0)
        return ClassifierModel(**kw)


def _clip(**over):
    from mae_clip_amd.CLIP import CLIPModel
    with product_config(precision="fp32", side_stream=False, **{**KW, **over}):
        torch.manual_seed(1)
        return CLIPModel()


def test_state_dict_keys_and_head_init():
    m = _classifier(num_classes=10)
    keys = set(m.state_dict())
    enc = {k for k in keys if k.startswith("image_encoder.model.")}
    assert keys == enc | {"head.weight", "head.bias"} and len(enc) > 10
    assert enc == {k for k in _clip().state_dict() if k.startswith("image_encoder.")}
    assert m.head.weight.shape == (10, 192) and m.head.bias.shape == (10,)
    assert m.head.weight.abs().max().item() <= 2 * 0.02 and m.head.weight.std().item() > 0.005
    assert m.head.bias.abs().max().item() == 0.0
    with product_config(num_classes=7, label_smoothing=0.1, classifier_trainable_encoder=True, **KW):
        from mae_clip_amd.classifier import ClassifierModel
        d = ClassifierModel()
    assert d.num_classes == 7 and d.label_smoothing == 0.1 and d.trainable_encoder
    assert all(p.requires_grad for p in d.parameters())
    with pytest.raises(ValueError, match="label_smoothing"):
        _classifier(label_smoothing=1.0)


def test_linear_probe_freezes_the_encoder():
    m = _classifier(num_classes=10, trainable_encoder=False)
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == ["head.bias", "head.weight"]
    m = _classifier(num_classes=10)      # the config default is the probe
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == ["head.bias", "head.weight"]
    m = _classifier(num_classes=10, trainable_encoder=True)
    assert all(p.requires_grad for p in m.parameters())


def test_load_image_encoder(tmp_path):
    from mae_clip_amd.checkpoint import save_checkpoint
    from mae_clip_amd.classifier import load_image_encoder
    clip = _clip()
    sd = clip.state_dict()
    m = _classifier(num_classes=10)
    head = m.head.weight.detach().clone()
    skipped = load_image_encoder(m, sd)
    own = m.state_dict()
    n = 0
    for k, v in sd.items():
        if k.startswith("image_encoder."):
            assert torch.equal(own[k].view(torch.int32), v.view(torch.int32)), k
            n += 1
    assert n > 10 and torch.equal(m.head.weight, head)
    assert sorted(skipped) == sorted(k for k in sd if not k.startswith("image_encoder."))
    assert any(k.startswith("text_encoder.") for k in skipped) and any(k.startswith("mae_decoder.") for k in skipped)
    # the two file forms: a checkpoint of save_checkpoint and a bare state_dict
    for name, write in (("ckpt.pt", lambda p: save_checkpoint(p, clip)), ("best.pt", lambda p: torch.save(sd, p))):
        path = str(tmp_path / name)
        write(path)
        m2 = _classifier(num_classes=10)
        assert sorted(load_image_encoder(m2, path)) == sorted(skipped)
        for k, v in m2.image_encoder.state_dict().items():
            assert torch.equal(v, sd["image_encoder." + k]), k
    other = _clip(model_name="vit_small_patch16_224", image_embedding=384)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        load_image_encoder(_classifier(num_classes=10), other.state_dict())
    with pytest.raises(RuntimeError, match="missing"):
        load_image_encoder(_classifier(num_classes=10), {k: v for k, v in sd.items() if "fc_norm" not in k})


@pytest.mark.parametrize("trainable", [False, True])
@pytest.mark.parametrize("soft", [False, True])
def test_training_step_plumbing(monkeypatch, trainable, soft):
    """forward / backward / AdamW with every launch stubbed: the loss goes through
    maeclip_xent_fwd and maeclip_xent_bwd, the probe's backward launches nothing
    of the encoder, and the padded head (7 classes on 8 columns) hands back
    gradients of the parameters' shapes"""
    from mae_clip_amd import classifier as CM
    from mae_clip_amd.optim import AdamW
    with stubbed_kernels(monkeypatch) as stub:
        m = _classifier(num_classes=7, trainable_encoder=trainable, label_smoothing=0.1).train()
        opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3)
        for B in (5, 3):
            opt.zero_grad(set_to_none=True)
            batch = {"image": make_batch(B, 32)["image"]}
            if soft:
                batch["target"] = torch.softmax(torch.randn(B, 7), -1)
            else:
                batch["label"] = torch.arange(B) % 7
            n0 = len(stub.calls)
            loss = m(batch)
            assert loss.shape == ()
            n1 = len(stub.calls)
            loss.backward()
            bwd = stub.calls[n1:]
            assert stub.calls[n0:n1].count("maeclip_xent_fwd") == 1 and bwd.count("maeclip_xent_bwd") == 1
            assert ("maeclip_attn_bwd" in bwd) == trainable and ("maeclip_ln_bwd" in bwd) == trainable
            for n, p in m.named_parameters():
                if p.requires_grad:
                    assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32, n
                else:
                    assert p.grad is None, n
            opt.step()
        assert m.step == 2 and set(m.last_losses) == {"xent"}
        m.eval()
        n0 = len(stub.calls)
        assert m.logits(make_batch(3, 32)["image"]).shape == (3, 7)
        res = CM.evaluate(m, [{"image": make_batch(3, 32)["image"], "label": torch.tensor([0, 6, 3])}] * 2, ks=(1, 3))
        assert set(res) == {"loss", "top1", "top3", "n"} and res["n"] == 6
        tail = stub.calls[n0:]
        assert tail.count("maeclip_xent_fwd") == 2 and not [c for c in tail if c.endswith("_bwd")]
        with pytest.raises(TypeError, match="int64 or int32"):
            m({"image": make_batch(2, 32)["image"], "label": torch.zeros(2)})
        with pytest.raises(ValueError, match="target"):
            m({"image": make_batch(2, 32)["image"], "target": torch.zeros(2, 9)})


def test_kernels_wrapper_argument_checks(monkeypatch):
    from mae_clip_amd import kernels as K
    with stubbed_kernels(monkeypatch):
        x = torch.zeros(4, 12)
        y = torch.zeros(4, dtype=torch.int64)
        with pytest.raises(ValueError, match="labels or targets"):
            K.xent_fwd(x)
        with pytest.raises(ValueError, match="C=13"):
            K.xent_fwd(x, y, C=13)
        with pytest.raises(ValueError, match="label_smoothing"):
            K.xent_fwd(x, y, label_smoothing=1.0)
        with pytest.raises(ValueError, match="labels must be"):
            K.xent_fwd(x, y.float())
        with pytest.raises(ValueError, match="targets must be"):
            K.xent_fwd(x, targets=torch.zeros(4, 8))
        with pytest.raises(ValueError, match="want_rank"):
            K.xent_fwd(x, targets=torch.zeros(4, 12), want_rank=True)
        out = K.xent_fwd(x, y, C=10, want_rank=True, row_loss=True)
        assert out.loss.shape == () and out.lse.shape == out.lse_lo.shape == out.row_loss.shape == (4,)
        assert out.rank.shape == (4,) and out.rank.dtype == torch.int32
        assert K.xent_fwd(x, y).rank is None and K.xent_fwd(x, y).row_loss is None
        d = K.xent_bwd(x, out.lse, y, C=10, lse_lo=out.lse_lo)
        assert d.shape == (4, 12) and d.dtype == torch.float32
        assert K.xent_bwd(x, out.lse, y, C=10, out=x) is x
        with pytest.raises(ValueError, match="dense"):
            K.xent_bwd(x, out.lse, y, C=10, out=torch.zeros(4, 16)[:, :12])
        with pytest.raises(ValueError, match="grad_output"):
            K.xent_bwd(x, out.lse, y, grad_output=torch.zeros(2))
