"""Plain-torch restatement of classifier.ClassifierModel's forward with drop-path
(timm VisionTransformer(global_pool="avg") with DropPath(scale_by_keep=True) on
both residual branches + head + cross-entropy), in float64 on the CPU, behind
tests/test_droppath_gpu.py. Nothing of the product is used but the state_dict
(timm's names) and the per-sample branch scales, which the caller takes from
kernels.droppath_scales_host: scales[i][j][b] multiplies branch j (0 attention,
1 MLP) of block i for sample b (1 / (1 - p) or 0; all ones without drop-path)."""
import torch
import torch.nn.functional as F


def params_of(state_dict):
    """float64 leaf copies of a ClassifierModel state_dict, by name"""
    return {k: v.detach().cpu().double().clone().requires_grad_() for k, v in state_dict.items()}


def classifier_loss(P, img, labels, scales, depth, heads, patch, label_smoothing=0.0, eps=1e-6):
    """P: params_of(model.state_dict()); img float64 [B, 3, S, S]; scales float64
    [depth, 2, B]. Returns (loss, logits)."""
    pre = "image_encoder.model."
    B = img.shape[0]
    w = P[pre + "patch_embed.proj.weight"]
    D = w.shape[0]
    # patch embedding: Conv2d(kernel = stride = patch) as unfold + linear, row-major patches
    cols = F.unfold(img, kernel_size=patch, stride=patch).transpose(1, 2)            # [B, L, 3 p p]
    x = F.linear(cols, w.reshape(D, -1), P[pre + "patch_embed.proj.bias"])
    x = torch.cat([P[pre + "cls_token"].expand(B, -1, -1), x], 1) + P[pre + "pos_embed"]
    n = x.shape[1]
    hd = D // heads
    for i in range(depth):
        b = f"{pre}blocks.{i}."
        h = F.layer_norm(x, (D,), P[b + "norm1.weight"], P[b + "norm1.bias"], eps)
        qkv = F.linear(h, P[b + "attn.qkv.weight"], P[b + "attn.qkv.bias"]).reshape(B, n, 3, heads, hd)
        q, k, v = qkv.permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, n, D)
        o = F.linear(o, P[b + "attn.proj.weight"], P[b + "attn.proj.bias"])
        x = x + scales[i, 0].view(B, 1, 1) * o
        h = F.layer_norm(x, (D,), P[b + "norm2.weight"], P[b + "norm2.bias"], eps)
        h = F.gelu(F.linear(h, P[b + "mlp.fc1.weight"], P[b + "mlp.fc1.bias"]))
        h = F.linear(h, P[b + "mlp.fc2.weight"], P[b + "mlp.fc2.bias"])
        x = x + scales[i, 1].view(B, 1, 1) * h
    feat = F.layer_norm(x[:, 1:].mean(1), (D,), P[pre + "fc_norm.weight"], P[pre + "fc_norm.bias"], eps)
    logits = F.linear(feat, P["head.weight"], P["head.bias"])
    return F.cross_entropy(logits, labels, label_smoothing=label_smoothing), logits
