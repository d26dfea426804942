"""optim.layer_decay_param_groups (MAE's param_groups_lrd) on the tiny ViT the
classifier tests build: vit_tiny_patch16_224 at size 32, cut to depth 2, with a
10-class head. No GPU: only names, shapes and requires_grad are looked at."""
import pytest
import torch

from tests.helpers import C0, product_config

KW = {k: v for k, v in C0.items() if k != "batch_size"}
DEPTH, LR, WD, LD = 2, 1e-3, 0.05, 0.75


def _model(trainable):
    from mae_clip_amd.classifier import ClassifierModel
    with product_config(precision="fp32", side_stream=False, **KW):
        torch.manual_seed(0)
        m = ClassifierModel(num_classes=10, trainable_encoder=trainable, label_smoothing=0.1)
    m.image_encoder.model.blocks = m.image_encoder.model.blocks[:DEPTH]
    return m


def _groups(m, **kw):
    from mae_clip_amd.optim import layer_decay_param_groups
    return layer_decay_param_groups(m, kw.get("lr", LR), kw.get("weight_decay", WD), kw.get("layer_decay", LD))


def _group_of(groups, p):
    hit = [g for g in groups if any(q is p for q in g["params"])]
    assert len(hit) == 1
    return hit[0]


def test_every_trainable_parameter_is_in_exactly_one_group():
    m = _model(True)
    groups = _groups(m)
    ids = [id(p) for g in groups for p in g["params"]]
    assert len(ids) == len(set(ids))
    assert set(ids) == {id(p) for p in m.parameters() if p.requires_grad}
    assert all(g["params"] for g in groups)
    names = [g["name"] for g in groups]
    assert len(set(names)) == len(names) and len(groups) <= 2 * (DEPTH + 2)
    assert names == sorted(names, key=lambda n: (int(n.split("_")[1]), n.endswith("no_decay")))


def test_layer_ids_and_scales():
    m = _model(True)
    groups = _groups(m)
    named = dict(m.named_parameters())
    pre = "image_encoder.model."
    want = {pre + "cls_token": 0, pre + "pos_embed": 0, pre + "patch_embed.proj.weight": 0,
            pre + "patch_embed.proj.bias": 0, pre + "blocks.0.attn.qkv.weight": 1, pre + "blocks.0.norm1.bias": 1,
            pre + f"blocks.{DEPTH - 1}.mlp.fc2.weight": DEPTH, pre + f"blocks.{DEPTH - 1}.mlp.fc2.bias": DEPTH,
            pre + "fc_norm.weight": DEPTH + 1, pre + "fc_norm.bias": DEPTH + 1, "head.weight": DEPTH + 1,
            "head.bias": DEPTH + 1}
    for name, k in want.items():
        g = _group_of(groups, named[name])
        scale = LD ** (DEPTH + 1 - k)
        assert g["name"].startswith(f"layer_{k}_"), (name, g["name"])
        assert g["lr_scale"] == pytest.approx(scale, rel=1e-12) and g["lr"] == pytest.approx(LR * scale, rel=1e-12), name
    assert _group_of(groups, named["head.weight"])["lr"] == LR


def test_no_decay_split():
    m = _model(True)
    groups = _groups(m)
    for name, p in m.named_parameters():
        g = _group_of(groups, p)
        no_decay = p.ndim == 1 or name.endswith("cls_token") or name.endswith("pos_embed")
        assert g["weight_decay"] == (0.0 if no_decay else WD), name
        assert g["name"].endswith("_no_decay") == no_decay, name
    named = dict(m.named_parameters())
    assert named["image_encoder.model.pos_embed"].ndim == 3       # not caught by the 1-D rule: by name
    assert _group_of(groups, named["image_encoder.model.pos_embed"])["weight_decay"] == 0.0


def test_frozen_encoder_yields_head_groups_only():
    m = _model(False)
    groups = _groups(m)
    assert sorted(g["name"] for g in groups) == [f"layer_{DEPTH + 1}_decay", f"layer_{DEPTH + 1}_no_decay"]
    assert [p is m.head.weight for g in groups for p in g["params"] if g["weight_decay"]] == [True]
    assert [p is m.head.bias for g in groups for p in g["params"] if not g["weight_decay"]] == [True]
    assert all(g["lr_scale"] == 1.0 and g["lr"] == LR for g in groups)     # the depth still counts the frozen blocks


def test_groups_feed_the_optimizer():
    from mae_clip_amd.optim import AdamW
    m = _model(True)
    opt = AdamW(_groups(m), lr=LR, weight_decay=WD, device_lr=True)
    assert len(opt.param_groups) == 2 * (DEPTH + 2) <= 32
    assert all({"lr_scale", "name", "lr", "weight_decay"} <= set(g) for g in opt.param_groups)
    assert [g["lr"] for g in opt.param_groups] == [LR * g["lr_scale"] for g in opt.param_groups]
    # ViT-B: 12 blocks -> 14 layer ids, two groups each: one push_lr launch
    assert 2 * (12 + 2) == 28


def test_layer_decay_one_and_bad_values():
    m = _model(True)
    assert all(g["lr"] == LR and g["lr_scale"] == 1.0 for g in _groups(m, layer_decay=1.0))
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="layer_decay"):
            _groups(m, layer_decay=bad)
