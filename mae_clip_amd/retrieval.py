"""Embedding search of the reference's inference.py on libmaeclip kernels
(SURVEY.md §8f row 4).

inference.py:13-27 (get_image_embeddings) runs the image tower + projection
over the validation loader; inference.py:29-47 (find_matches) embeds one
tokenised query, L2-normalises both sides (F.normalize), forms
text_n @ image_n.T and keeps every 5th of the top n*5 matches. The same calls
are made here, with the normalisation, the fp32 similarity GEMM and the top-k
selection on the device (maeclip_l2_normalize / maeclip_gemm /
maeclip_topk_rows). Tokenisation (DistilBertTokenizer.from_pretrained) and the
matplotlib display stay with the caller: there is no tokenizer download here.
"""
from __future__ import annotations

import torch

from . import kernels as K
from .kernels import _dev, _call, _stream


def l2_normalize(x: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """F.normalize(x, p=2, dim=-1) for fp32 [M, P] (inference.py:40-41)."""
    _dev(x)
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("l2_normalize: fp32 [M, P] with unit column stride expected")
    y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    _call("maeclip_l2_normalize", x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], x.stride(0), y.stride(0), eps,
          _stream())
    return y


def topk_rows(s: torch.Tensor, k: int):
    """torch.topk(s, k, dim=-1) for fp32 [Q, N]: values descending, ties -> lower index."""
    _dev(s)
    if s.dtype != torch.float32 or s.dim() != 2 or s.stride(1) != 1:
        raise ValueError("topk_rows: fp32 [Q, N] with unit column stride expected")
    Q, N = s.shape
    vals = torch.empty((Q, k), device=s.device, dtype=torch.float32)
    idx = torch.empty((Q, k), device=s.device, dtype=torch.int64)
    _call("maeclip_topk_rows", s.data_ptr(), Q, N, s.stride(0), int(k), vals.data_ptr(), idx.data_ptr(), _stream())
    return vals, idx


def similarity(text_embeddings: torch.Tensor, image_embeddings: torch.Tensor) -> torch.Tensor:
    """normalize(text) @ normalize(image).T (inference.py:40-42), fp32 [Q, N]."""
    tn = l2_normalize(text_embeddings.float().contiguous())
    im = l2_normalize(image_embeddings.float().contiguous())
    Q, P = tn.shape
    N = im.shape[0]
    # the GEMM writes 4-column groups: a gallery of any size is padded with zero
    # rows to a multiple of 4 and the padded similarity columns are cut off
    # (a view with row stride Npad: topk_rows honours it)
    Npad = (N + 3) // 4 * 4
    if Npad != N:
        im = torch.cat([im, im.new_zeros((Npad - N, P))])
    out = torch.empty((Q, Npad), device=tn.device, dtype=torch.float32)
    K.gemm(tn, im, out, Q, Npad, P, tn.stride(0), im.stride(0), Npad, K.KC, K.KC)
    return out[:, :N]


@torch.no_grad()
def get_image_embeddings(model, image_batches):
    """inference.py:13-27 minus the loader: image tower + projection over an
    iterable of device image batches ([B, 3, S, S] fp32) in eval mode."""
    model.eval()
    out = [model.image_projection(model.image_encoder(b)) for b in image_batches]
    return torch.cat(out)


@torch.no_grad()
def get_text_embeddings(model, token_batches):
    """The text side of get_image_embeddings: text tower + text projection over
    an iterable of device (input_ids, attention_mask) pairs (or dicts with
    those keys) in eval mode."""
    model.eval()
    out = []
    for b in token_batches:
        ids, mask = (b["input_ids"], b["attention_mask"]) if isinstance(b, dict) else b
        out.append(model.text_projection(model.text_encoder(input_ids=ids, attention_mask=mask)))
    return torch.cat(out)


def _emb(q, g):
    for name, x in (("query_emb", q), ("gallery_emb", g)):
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2:
            raise ValueError(f"similarity_topk: {name} must be an fp32 [rows, P] tensor")
    if q.shape[1] != g.shape[1]:
        raise ValueError("similarity_topk: query and gallery widths differ")
    _dev(q, g)
    return tuple(x if x.stride(1) == 1 else x.contiguous() for x in (q, g))


def _labels(name, x, n, device):
    x = torch.as_tensor(x)
    if x.dim() != 1 or x.shape[0] != n or x.dtype.is_floating_point:
        raise ValueError(f"similarity_topk: {name} must be {n} integer labels")
    return x.to(device=device, dtype=torch.int64).contiguous()


def similarity_topk(query_emb, gallery_emb, k, *, normalize=True, query_labels=None, gallery_labels=None, splits=0):
    """torch.topk(query @ gallery.T, k) per query row without the [Q, N] matrix
    (maeclip_sim_topk): (vals fp32 [Q, k] descending, idx int64 [Q, k], ties to
    the lower index). normalize=True passes both sides through l2_normalize
    first (inference.py:40-41). With query_labels [Q] and gallery_labels [N]
    also first_hit int32 [Q]: the first rank whose gallery label equals the
    query's, k when none does. 1 <= k <= min(N, 64), P % 16 == 0, P <= 512;
    splits: 0 = automatic (see maeclip_sim_topk)."""
    q, g = _emb(query_emb, gallery_emb)
    if (query_labels is None) != (gallery_labels is None):
        raise ValueError("similarity_topk: query_labels and gallery_labels go together")
    if normalize:
        q, g = l2_normalize(q), l2_normalize(g)
    (Q, P), N, k, splits = q.shape, g.shape[0], int(k), int(splits)
    lib = K.L.lib()
    nbytes = lib.maeclip_sim_topk_workspace(Q, N, P, k, splits)
    if nbytes < 0:
        K.L.check(int(nbytes), "maeclip_sim_topk_workspace")
    ws = torch.empty(nbytes, device=q.device, dtype=torch.uint8) if nbytes else None
    vals = torch.empty((Q, k), device=q.device, dtype=torch.float32)
    idx = torch.empty((Q, k), device=q.device, dtype=torch.int64)
    ql = gl = fh = None
    if query_labels is not None:
        ql, gl = _labels("query_labels", query_labels, Q, q.device), _labels("gallery_labels", gallery_labels, N, q.device)
        fh = torch.empty((Q,), device=q.device, dtype=torch.int32)
    ptr = lambda t: t.data_ptr() if t is not None else None
    _call("maeclip_sim_topk", q.data_ptr(), g.data_ptr(), Q, N, P, q.stride(0), g.stride(0), k, splits,
          vals.data_ptr(), idx.data_ptr(), ptr(ql), ptr(gl), ptr(fh), ptr(ws), nbytes, _stream())
    return (vals, idx) if fh is None else (vals, idx, fh)


def recall_at_k(query_emb, gallery_emb, query_labels, gallery_labels, ks=(1, 5, 10)):
    """{K: recall@K}: the share of queries with a gallery row of their own label
    among the K most similar. One fused call at k = max(ks) (N if smaller)."""
    ks = tuple(int(c) for c in ks)
    k = min(max(ks), gallery_emb.shape[0])
    _, _, fh = similarity_topk(query_emb, gallery_emb, k, query_labels=query_labels, gallery_labels=gallery_labels)
    return {c: (fh < min(c, k)).float().mean().item() for c in ks}


def zero_shot_accuracy(image_emb, class_text_emb, targets, ks=(1, 5), class_labels=None):
    """Zero-shot top-K accuracy: an image counts at K when a prompt of its target
    class is among its K most similar prompt embeddings. class_labels[c] is the
    class of prompt c (default arange: one prompt per class)."""
    if class_labels is None:
        class_labels = torch.arange(class_text_emb.shape[0], device=class_text_emb.device)
    return recall_at_k(image_emb, class_text_emb, targets, class_labels, ks)


@torch.no_grad()
def evaluate_retrieval(model, image_batches, token_batches, text_image_index, ks=(1, 5, 10)):
    """Image->text and text->image recall@K of a model over a validation set:
    {"i2t": {K: r}, "t2i": {K: r}}. text_image_index[c] is the image caption c
    belongs to (COCO: five captions per image). i2t counts an image at K when
    one of its captions is among its K nearest; t2i a caption when its image is."""
    img = get_image_embeddings(model, image_batches).float()
    txt = get_text_embeddings(model, token_batches).float()
    t2i = torch.as_tensor(text_image_index).to(device=img.device, dtype=torch.int64)
    if t2i.shape != (txt.shape[0],):
        raise ValueError("evaluate_retrieval: one image index per caption expected")
    ids = torch.arange(img.shape[0], device=img.device)
    return {"i2t": recall_at_k(img, txt, ids, t2i, ks), "t2i": recall_at_k(txt, img, t2i, ids, ks)}


@torch.no_grad()
def find_matches(model, image_embeddings, input_ids, attention_mask, n=9):
    """inference.py:29-45: indices of the n matches of one tokenised query
    (torch.topk(..., n * 5) then every 5th, as the reference does)."""
    model.eval()
    text_features = model.text_encoder(input_ids=input_ids, attention_mask=attention_mask)
    text_embeddings = model.text_projection(text_features)
    sim = similarity(text_embeddings, image_embeddings)
    _, indices = topk_rows(sim[:1], n * 5)
    return indices[0, ::5]
