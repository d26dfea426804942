"""Retrieval evaluation on the device (retrieval_eval.hip through
mae_clip_amd.retrieval): the fused similarity + top-k against exact integer
references with ties at the cut, its independence of the split count, fp64
bounds on random normalised data, strided inputs, label first-hit / recall /
zero-shot accuracy, the absence of the [Q, N] matrix, and the model flow."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GRID = [(1, 1, 1), (1, 7, 3), (3, 16, 16), (2, 17, 17), (17, 300, 64), (33, 1001, 45), (65, 129, 10)]
FORCED = (1, 2, 7, 1000)


def _splits(Q, N, P, k, forced):
    from mae_clip_amd import _lib as L
    return L.lib().maeclip_sim_topk_splits(Q, N, P, k, forced)


def _cpu_order(scores, k):
    """[Q][k] lists of the CPU order (score descending, index ascending)."""
    return [sorted(range(scores.shape[1]), key=lambda j: (-scores[q, j].item(), j))[:k + 1]
            for q in range(scores.shape[0])]


def _int_case(Q, N, k, P):
    """Integer embeddings in [-4, 4] (every score an exact integer below 2^24 in
    any summation order), from the first seed that gives some query row equal
    scores at positions k - 1 and k of the CPU order (k < N), so that the tie
    break decides the cut; with k == N there is no cut, and the seed must give
    equal neighbours inside the list instead (N > 1)."""
    for seed in range(20000):
        gen = torch.Generator().manual_seed(1000 * P + seed)
        q = torch.randint(-4, 5, (Q, P), generator=gen).float()
        g = torch.randint(-4, 5, (N, P), generator=gen).float()
        sc = (q.double() @ g.double().T)
        srt = sc.sort(dim=1, descending=True).values
        if N == 1:
            tie = True
        elif k < N:
            tie = bool((srt[:, k - 1] == srt[:, k]).any())
        else:
            tie = bool((srt[:, 1:] == srt[:, :-1]).any())
        if tie:
            return q, g, sc
    raise AssertionError("no seed with a tie at the cut")


@pytest.mark.parametrize("P", [16, 64, 256, 512])
@pytest.mark.parametrize("QNk", GRID, ids=lambda t: "x".join(map(str, t)))
def test_exact_with_ties(dev, QNk, P):
    from mae_clip_amd.retrieval import similarity_topk
    Q, N, k = QNk
    q, g, sc = _int_case(Q, N, k, P)
    assert sc.abs().max().item() < 2 ** 24
    order = _cpu_order(sc, k)
    if 1 < N:
        if k < N:   # the condition the data was chosen for: a tie straddles rank k
            assert any(sc[r, o[k - 1]] == sc[r, o[k]] for r, o in enumerate(order))
        else:
            assert any(sc[r, o[t]] == sc[r, o[t + 1]] for r, o in enumerate(order) for t in range(N - 1))
    want_idx = torch.tensor([o[:k] for o in order])
    want_val = torch.gather(sc, 1, want_idx).float()
    qd, gd = q.to(dev), g.to(dev)
    tiles = (N + 15) // 16
    for forced in FORCED:
        assert _splits(Q, N, P, k, forced) == min(forced, tiles)
        vals, idx = similarity_topk(qd, gd, k, normalize=False, splits=forced)
        assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and vals.shape == idx.shape == (Q, k)
        assert torch.equal(idx.cpu(), want_idx), (forced, idx.cpu(), want_idx)
        assert torch.equal(vals.cpu().view(torch.int32), want_val.view(torch.int32)), forced


def _normalised(Q, N, P, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn((Q, P), generator=gen)
    g = torch.randn((N, P), generator=gen)
    g[min(5, N - 1)] = g[3 % N]   # exact duplicate candidates -> tied scores
    g[N // 2] = 0.0               # zero row: the normalisation's eps clamp
    return q.to(dev), g.to(dev)


def test_split_independence_and_determinism(dev):
    from mae_clip_amd.retrieval import similarity_topk
    Q, N, P, k = 70, 3000, 128, 33
    q, g = _normalised(Q, N, P, dev, 7)
    base_v, base_i = similarity_topk(q, g, k, splits=1)
    for forced in (1, 2, 3, 8, 0):
        v, i = similarity_topk(q, g, k, splits=forced)
        assert torch.equal(i, base_i), forced
        assert torch.equal(v.view(torch.int32), base_v.view(torch.int32)), forced
    # one query row takes the automatic many-slice plan
    assert _splits(1, N, P, k, 0) > 1
    a = similarity_topk(q[:1], g, k)
    b = similarity_topk(q[:1], g, k)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[1], base_i[:1]) and torch.equal(a[0].view(torch.int32), base_v[:1].view(torch.int32))


@pytest.mark.parametrize("QNk", [(1, 6000, 45), (3, 1000, 7), (40, 2100, 10)], ids=lambda t: "x".join(map(str, t)))
def test_random_normalised_against_fp64(dev, QNk):
    from mae_clip_amd.retrieval import similarity_topk
    Q, N, k = QNk
    q, g = _normalised(Q, N, 256, dev, 91)
    vals, idx = similarity_topk(q, g, k)
    ref = (torch.nn.functional.normalize(q.double(), dim=-1) @ torch.nn.functional.normalize(g.double(), dim=-1).T).cpu()
    vals, idx = vals.cpu().double(), idx.cpu()
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    err = (vals - torch.gather(ref, 1, idx)).abs().max().item()
    print(f"max |vals - ref| = {err:.3e}")
    assert err < 1e-5
    for r in range(Q):
        assert len(set(idx[r].tolist())) == k
        for t in range(k - 1):
            assert vals[r, t] > vals[r, t + 1] or (vals[r, t] == vals[r, t + 1] and idx[r, t] < idx[r, t + 1])
        rest = torch.ones(N, dtype=torch.bool)
        rest[idx[r]] = False
        if rest.any():
            over = (ref[r][rest].max() - vals[r, k - 1]).item()
            assert over <= 2e-5, (r, over)


def test_strided_inputs(dev):
    from mae_clip_amd.retrieval import similarity_topk
    Q, N, P, k = 19, 500, 64, 12
    gen = torch.Generator().manual_seed(5)
    wq = torch.randn((Q, P + 9), generator=gen).to(dev)
    wg = torch.randn((N, P + 7), generator=gen).to(dev)
    q, g = wq[:, 3:3 + P], wg[:, 5:5 + P]   # row strides above P, rows at odd float offsets
    assert q.stride(0) > P and g.stride(0) > P
    for forced in (1, 3):
        v, i = similarity_topk(q, g, k, normalize=False, splits=forced)
        cv, ci = similarity_topk(q.contiguous(), g.contiguous(), k, normalize=False, splits=forced)
        assert torch.equal(i, ci) and torch.equal(v.view(torch.int32), cv.view(torch.int32))


def _first_hit(idx, ql, gl, k):
    hit = gl[idx] == ql[:, None]
    pos = torch.arange(k, device=idx.device).expand_as(hit)
    return torch.where(hit, pos, torch.full_like(pos, k)).min(dim=1).values


@pytest.mark.parametrize("direction", ["t2i", "i2t"])
def test_labels_first_hit_and_recall(dev, direction):
    from mae_clip_amd.retrieval import similarity_topk, recall_at_k
    n_img, per, P, k = 60, 5, 64, 10
    gen = torch.Generator().manual_seed(11)
    img = torch.randn((n_img, P), generator=gen)
    cap_img = torch.arange(n_img).repeat_interleave(per)
    cap = img[cap_img] + 4.0 * torch.randn((n_img * per, P), generator=gen)   # captions near their image
    img, cap, cap_img = img.to(dev), cap.to(dev), cap_img.to(dev)
    img_id = torch.arange(n_img, device=dev)
    if direction == "t2i":
        q, g, ql, gl = cap, img, cap_img.clone(), img_id
    else:
        q, g, ql, gl = img, cap, img_id.clone(), cap_img
    ql[1] = 10 ** 12   # a label the gallery does not have
    for forced in (0, 3):
        vals, idx, fh = similarity_topk(q, g, k, query_labels=ql, gallery_labels=gl, splits=forced)
        assert fh.dtype == torch.int32 and fh.shape == (q.shape[0],)
        want = _first_hit(idx, ql, gl, k)
        assert torch.equal(fh.long(), want)
        assert fh[1].item() == k
        v2, i2 = similarity_topk(q, g, k, splits=forced)
        assert torch.equal(i2, idx) and torch.equal(v2, vals)
    assert 0 < (want < k).sum().item() < q.shape[0]   # some rows hit, some do not
    rec = recall_at_k(q, g, ql, gl, ks=(1, 5, 10))
    for K_ in (1, 5, 10):
        assert rec[K_] == (want < K_).float().mean().item()
    assert rec[1] <= rec[5] <= rec[10]


def test_zero_shot_accuracy_exact(dev):
    """Integer data whose order survives the wrapper's normalisation exactly:
    one-hot prompts (norm 1) and images with 2 at the target class, every 4th
    also 3 at another class; a row's scaling by its own norm keeps zeros zero
    and the order of the rest, so top-1 = 3/4 and top-5 = 1 as on the CPU."""
    from mae_clip_amd.retrieval import zero_shot_accuracy
    n_cls, n_img, P = 37, 200, 64
    gen = torch.Generator().manual_seed(3)
    tgt = torch.randint(0, n_cls, (n_img,), generator=gen)
    cls = torch.zeros(n_cls, P)
    cls[torch.arange(n_cls), torch.arange(n_cls)] = 1.0
    img = torch.zeros(n_img, P)
    img[torch.arange(n_img), tgt] = 2.0
    img[torch.arange(0, n_img, 4), ((tgt + 1) % n_cls)[::4]] = 3.0
    order = torch.tensor([o[:5] for o in _cpu_order(img.double() @ cls.double().T, 5)])
    want1 = (order[:, 0] == tgt).float().mean().item()
    want5 = (order == tgt[:, None]).any(dim=1).float().mean().item()
    assert want1 == 0.75 and want5 == 1.0
    got = zero_shot_accuracy(img.to(dev), cls.to(dev), tgt.to(dev), ks=(1, 5))
    assert got == {1: want1, 5: want5}
    # several prompts per class share a label
    got2 = zero_shot_accuracy(img.to(dev), torch.cat([cls, cls]).to(dev), tgt.to(dev), ks=(1, 5),
                              class_labels=torch.arange(n_cls).repeat(2).to(dev))
    assert got2[1] == want1 and got2[5] == 1.0


def test_no_similarity_matrix(dev):
    from mae_clip_amd.retrieval import similarity_topk
    Q, N, P, k = 2048, 8192, 256, 10
    gen = torch.Generator().manual_seed(1)
    q = torch.randn((Q, P), generator=gen).to(dev)
    g = torch.randn((N, P), generator=gen).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    vals, idx = similarity_topk(q, g, k)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print(f"peak growth {growth} bytes, matrix {Q * N * 4} bytes")
    assert growth < Q * N * 4 // 2
    ref = torch.nn.functional.normalize(q[:4].double(), dim=-1) @ torch.nn.functional.normalize(g.double(), dim=-1).T
    assert (vals[:4].double() - ref.topk(k, dim=1).values).abs().max().item() < 1e-5


def test_evaluate_retrieval_flow(dev):
    from mae_clip_amd.retrieval import (evaluate_retrieval, get_image_embeddings, get_text_embeddings,
                                        similarity_topk)
    from tests.helpers import build_pair, make_batch
    prod, _ = build_pair("fp32")
    ib = [make_batch(4, 32, seed=20 + s)["image"].to(dev) for s in range(3)]
    tb = []
    for s in range(3):
        b = make_batch(5, 32, seed=30 + s, pad=True)
        tb.append((b["input_ids"].to(dev), b["attention_mask"].to(dev)))
    t2i = torch.tensor([c % 12 for c in range(15)])
    ks = (1, 5, 10)
    out = evaluate_retrieval(prod, ib, tb, t2i, ks=ks)
    assert set(out) == {"i2t", "t2i"} and all(set(out[d]) == set(ks) for d in out)
    img = get_image_embeddings(prod, ib)
    txt = get_text_embeddings(prod, tb)
    assert img.shape[0] == 12 and txt.shape[0] == 15
    with torch.no_grad():
        direct = torch.cat([prod.text_projection(prod.text_encoder(input_ids=i, attention_mask=m)) for i, m in tb])
    assert torch.equal(txt, direct)
    t2i_d, ids = t2i.to(dev), torch.arange(12, device=dev)
    for name, q, g, ql, gl in (("i2t", img, txt, ids, t2i_d), ("t2i", txt, img, t2i_d, ids)):
        _, idx = similarity_topk(q.float(), g.float(), 10)
        fh = _first_hit(idx, ql, gl, 10)
        for K_ in ks:
            assert out[name][K_] == (fh < K_).float().mean().item(), (name, K_)
