"""Kernels behind the trainable text tower vs fp64 torch: the attention
backward with DistilBERT's key-padding mask and attention dropout, the
LayerNorm-fused dropout masks the backward redraws, and the embedding
backward. Runs on the GPU box only."""
import pytest
import torch

from mae_clip_amd import kernels as K
from tests import attn_cases as A

pytestmark = pytest.mark.gpu

# the bounds of test_kernels_gpu.test_attention_fwd_bwd (forward, backward), per dtype
ATT_TOL = {torch.float32: (2e-5, 1e-4), torch.bfloat16: (2e-2, 3e-2)}


def _rand(shape, dtype, dev, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def _attn_ref(qkv, B, n, H, hd, scale, key_mask=None, keep=None, p=0.0):
    """fp64 attention, masked_fill then softmax (oracle/ref_model.py:326-328);
    keep [B, H, n, n]: explicit dropout keep mask on the probabilities."""
    q, k, v = qkv.double().view(B, n, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * scale
    if key_mask is not None:
        s = s.masked_fill(key_mask.view(B, 1, 1, n) == 0, float("-inf"))
    pr = s.softmax(-1)
    if keep is not None:
        pr = pr * keep.double() / (1.0 - p)
    return (pr @ v).transpose(1, 2).reshape(B * n, H * hd)


def _key_mask(lens, n, dev):
    km = torch.zeros((len(lens), n), device=dev)
    for b, L in enumerate(lens):
        km[b, :L] = 1
    return km


def _bwd_guarded(qkv, o, dout, lse, B, n, H, hd, **kw):
    """attn_bwd into the head of a larger buffer: the rows past B*n must stay untouched."""
    D3 = 3 * H * hd
    big = torch.full((B * n + 8, D3), 7.0, device=qkv.device, dtype=qkv.dtype)
    dqkv, part = K.attn_bwd(qkv, o, dout, lse, B, n, H, hd, hd ** -0.5, dqkv_out=big[:B * n], **kw)
    assert (big[B * n:] == 7.0).all()
    return dqkv, part


def _check_grads(dqkv, part, g, B, n, H, hd, tolb, dv_sum_is_dout=None):
    gs = g.abs().max().item()
    HH = H * hd
    for j, name in enumerate(("dq", "dk", "dv")):
        err = (dqkv.double() - g)[:, j * HH:(j + 1) * HH].abs().max().item() / gs
        print(f"{name} max err / max|g| = {err:.3e} (bound {tolb})")
        assert err < tolb, name
    cs = part.sum(0)
    gsum = g.view(B * n, 3, HH).sum(0)
    err = (cs.double() - gsum.view(-1)).abs().max().item() / (gs * n)
    print(f"bias partial err = {err:.3e}")
    assert err < tolb
    # the k-bias gradient is identically zero, with a mask and with dropout
    assert gsum[1].abs().max().item() < 1e-9 * gs * n
    assert (cs.view(3, -1)[1] == 0).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,lens", [((2, 16, 2), (1, 16)), ((2, 25, 2), (7, 25)), ((1, 33, 1), (20,)),
                                        ((2, 200, 2), (200, 131))])
def test_attention_bwd_key_mask(dev, dtype, shape, lens):
    """(a) the masked backward of the two-phase kernel: one tile, make_batch's
    T, one past a 32-row pad boundary, the reference's max_length (npad 224);
    ragged lengths from 1 (CLS only) to n."""
    (B, n, H), hd = shape, 64
    scale = hd ** -0.5
    km = _key_mask(lens, n, dev)
    qkv = _rand((B * n, 3 * H * hd), dtype, dev, seed=51)
    dout = _rand((B * n, H * hd), dtype, dev, seed=52)
    o, lse = K.attn_fwd(qkv, B, n, H, hd, scale, key_mask=km)
    x64 = qkv.double().detach().requires_grad_(True)
    ref = _attn_ref(x64, B, n, H, hd, scale, key_mask=km)
    tolf, tolb = ATT_TOL[dtype]
    assert (o.double() - ref).abs().max().item() < tolf
    (ref * dout.double()).sum().backward()
    g = x64.grad
    assert A.path(dtype, n, H, hd, True, B=B, key_mask=True) == A.BWD_MASKED
    dqkv, part = _bwd_guarded(qkv, o, dout, lse, B, n, H, hd, key_mask=km)
    _check_grads(dqkv, part, g, B, n, H, hd, tolb)
    # masked keys: dk / dv rows exactly zero, as in the reference
    dead = (km.view(-1) == 0)
    HH = H * hd
    assert (g[dead][:, HH:] == 0).all()
    assert (dqkv[dead][:, HH:] == 0).all()
    # valid rows still sum to 1: the v-bias partial is the column sum of dO
    assert (part.sum(0).view(3, -1)[2].double() - dout.double().sum(0)).abs().max().item() < 1e-4 * max(1.0, n ** 0.5)
    dq2, part2 = K.attn_bwd(qkv, o, dout, lse, B, n, H, hd, scale, key_mask=km)
    assert torch.equal(dq2, dqkv) and torch.equal(part2, part)


def _recover_keep(B, n, H, hd, p, seed, step, dev):
    """The forward's keep mask [B, H, n, n] from the forward itself: q = k = 0
    gives uniform probabilities 1/n, V an identity block on rows 64j..64j+63,
    so O[q, d] = keep(q, 64j + d) / (n (1 - p)); the mask depends only on
    (seed, step, b*H + h, q, k)."""
    keep = torch.zeros((B, H, n, n), device=dev)
    for j in range((n + hd - 1) // hd):
        w = min(hd, n - hd * j)
        qkv = torch.zeros((B, n, 3, H, hd), device=dev)
        qkv[:, hd * j:hd * j + w, 2, :, :w] = torch.eye(w, device=dev).view(1, w, 1, w)
        o, _ = K.attn_fwd(qkv.view(B * n, 3 * H * hd), B, n, H, hd, hd ** -0.5, dropout_p=p, seed=seed,
                          want_lse=False, step_ptr=step)
        blk = o.view(B, n, H, hd)[..., :w].permute(0, 2, 1, 3)     # [B, H, q, k - 64j]
        nz = blk[blk != 0]
        assert torch.allclose(nz, torch.full_like(nz, 1 / (n * (1 - p))), rtol=1e-5)
        keep[:, :, :, hd * j:hd * j + w] = (blk != 0).float()
    frac = 1 - keep.mean().item()
    assert abs(frac - p) < 6 * (p * (1 - p) / keep.numel()) ** 0.5, frac
    return keep


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape,lens", [((2, 25, 2), (25, 9)), ((1, 200, 2), (150,))])
def test_attention_bwd_dropout(dev, dtype, masked, p, shape, lens):
    """(b) the backward redraws the forward's dropout mask (same seed and step
    value): dq / dk / dv and the bias partials vs fp64 torch with the mask
    recovered from the forward; bitwise equal on a second run."""
    (B, n, H), hd = shape, 64
    scale = hd ** -0.5
    seed = 977
    step = torch.tensor([3], dtype=torch.int64, device=dev)
    keep = _recover_keep(B, n, H, hd, p, seed, step, dev)
    km = _key_mask(lens, n, dev) if masked else None
    qkv = _rand((B * n, 3 * H * hd), dtype, dev, seed=53)
    dout = _rand((B * n, H * hd), dtype, dev, seed=54)
    o, lse = K.attn_fwd(qkv, B, n, H, hd, scale, key_mask=km, dropout_p=p, seed=seed, step_ptr=step)
    x64 = qkv.double().detach().requires_grad_(True)
    ref = _attn_ref(x64, B, n, H, hd, scale, key_mask=km, keep=keep, p=p)
    tolf, tolb = ATT_TOL[dtype]
    ferr = (o.double() - ref).abs().max().item()
    print(f"forward err {ferr:.3e}")
    assert ferr < tolf / (1 - p)   # the kept probabilities, and with them O and its rounding, scale by 1/(1-p)
    (ref * dout.double()).sum().backward()
    kw = dict(key_mask=km, dropout_p=p, seed=seed, step_ptr=step)
    assert A.path(dtype, n, H, hd, True, B=B, key_mask=masked, dropout_p=p) == A.BWD_MASKED
    dqkv, part = _bwd_guarded(qkv, o, dout, lse, B, n, H, hd, **kw)
    _check_grads(dqkv, part, x64.grad, B, n, H, hd, tolb)
    dq2, part2 = K.attn_bwd(qkv, o, dout, lse, B, n, H, hd, scale, **kw)
    assert torch.equal(dq2, dqkv) and torch.equal(part2, part)
    # another step value draws another mask
    other = torch.tensor([4], dtype=torch.int64, device=dev)
    dq3, _ = K.attn_bwd(qkv, o, dout, lse, B, n, H, hd, scale, **dict(kw, step_ptr=other))
    assert not torch.equal(dq3, dqkv)


def test_attention_bwd_mask_limits(dev):
    """Past n = 256 (and at head_dim 32) the masked / dropout backward is
    rejected with a message; the fp32 rows path still takes the mask."""
    from mae_clip_amd._lib import MaeClipNativeError
    for dtype, B, n, H, hd, kw in ((torch.bfloat16, 1, 288, 1, 64, {}), (torch.bfloat16, 1, 40, 1, 32, {}),
                                   (torch.float32, 1, 40, 1, 64, dict(dropout_p=1.0))):
        qkv = _rand((B * n, 3 * H * hd), dtype, dev, seed=55)
        km = _key_mask((n - 3,), n, dev)
        o, lse = K.attn_fwd(qkv, B, n, H, hd, hd ** -0.5, key_mask=km)
        with pytest.raises(MaeClipNativeError, match="maeclip_attn_bwd"):
            K.attn_bwd(qkv, o, o, lse, B, n, H, hd, hd ** -0.5, key_mask=km, **kw)
    B, n, H, hd = 1, 600, 1, 64
    qkv = _rand((B * n, 3 * H * hd), torch.float32, dev, seed=56)
    km = _key_mask((500,), n, dev)
    o, lse = K.attn_fwd(qkv, B, n, H, hd, hd ** -0.5, key_mask=km)
    dqkv, _ = K.attn_bwd(qkv, o, o, lse, B, n, H, hd, hd ** -0.5, key_mask=km)
    assert (dqkv[500:, H * hd:] == 0).all() and torch.isfinite(dqkv).all()


@pytest.mark.parametrize("p,zero_res", [(0.5, False), (0.1, True)])
def test_ln_dropout_masks_are_maeclip_dropout(dev, p, zero_res):
    """(c) what TextStackFn's backward relies on: the LayerNorm's fused output
    and input dropouts draw the mask of maeclip_dropout for the same seed and
    step. Bitwise: p = 0.5 scales by exactly 2, so dropout(x) + res rounds once
    however the kernel fuses the add; at DistilBERT's p = 0.1 the residual is
    zero for the same reason."""
    M, D, s = 77, 768, 4242
    step = torch.tensor([5], dtype=torch.int64, device=dev)
    x = _rand((M, D), torch.float32, dev, seed=61)
    res = torch.zeros((M, D), device=dev) if zero_res else _rand((M, D), torch.float32, dev, seed=62)
    g = _rand((D,), torch.float32, dev, seed=63)
    b = _rand((D,), torch.float32, dev, seed=64)
    plain = K.ln_fwd(x, g, b, 1e-12, out_dtype=torch.float32)[0]
    yo, _, _, yob, _ = K.ln_fwd(x, g, b, 1e-12, out_dtype=torch.float32, out_dropout=p, seed_out=s, y2=True,
                                step_ptr=step)
    want = K.dropout(plain, p, s, step_ptr=step)
    assert torch.equal(yo, want)
    assert torch.equal(yob, want.to(torch.bfloat16))
    assert 0 < (want == 0).float().mean().item() < 1
    yi, mi, ri, _, xs = K.ln_fwd(x, g, b, 1e-12, out_dtype=torch.float32, res=res, in_dropout=p, seed_in=s, xsum=True,
                                 step_ptr=step)
    xd = K.dropout(x, p, s, step_ptr=step) + res
    assert torch.equal(xs, xd)
    y2, m2, r2, _, _ = K.ln_fwd(xd, g, b, 1e-12, out_dtype=torch.float32)
    assert torch.equal(yi, y2) and torch.equal(mi, m2) and torch.equal(ri, r2)


def test_ln_in_dropout_mask_at_p01_with_residual(dev):
    """The mask identity at the p the tower runs with (0.1) and a real residual:
    x * 1/(1-p) + res may round once or twice depending on how the kernel fuses
    the add, so the values are not compared bitwise; the positions where the
    LayerNorm's input sum differs from the residual are exactly the kept
    positions of maeclip_dropout (|x| and |res| are kept away from zero, so a
    kept term cannot vanish in the sum), and the values agree within the three
    half-ulp roundings that separate fma(x, sc, res) from round(round(x sc) + res)."""
    M, D, s, p = 77, 768, 4242, 0.1
    step = torch.tensor([5], dtype=torch.int64, device=dev)
    x = _rand((M, D), torch.float32, dev, seed=65)
    x = torch.where(x.abs() < 0.05, torch.full_like(x, 0.5), x)
    res = _rand((M, D), torch.float32, dev, seed=66)
    res = torch.where(res.abs() < 0.05, torch.full_like(res, -0.5), res)
    g, b = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    xs = K.ln_fwd(x, g, b, 1e-12, out_dtype=torch.float32, res=res, in_dropout=p, seed_in=s, xsum=True,
                  step_ptr=step)[4]
    xd = K.dropout(x, p, s, step_ptr=step)
    assert torch.equal(xs != res, xd != 0)
    assert 0.05 < (xd == 0).float().mean().item() < 0.15
    want = xd + res
    assert ((xs - want).abs() <= 3 * 2.0 ** -24 * want.abs().clamp_min(xd.abs())).all()


def _embed_case(case, B, T, V, gen):
    if case == "repeats":
        ids = torch.randint(1, min(V, 12), (B, T), generator=gen)      # every id repeats many times
    elif case == "with_pad":
        ids = torch.randint(0, min(V, 40), (B, T), generator=gen)
        ids[:, T // 2:] = 0                                            # id 0 fills the tails
        ids[0, 0] = 0
    else:   # "one_row": one id fills a whole sample
        ids = torch.randint(1, V, (B, T), generator=gen)
        ids[B - 1, :] = min(V - 1, 17)
    return ids


@pytest.mark.parametrize("case", ["repeats", "with_pad", "one_row"])
@pytest.mark.parametrize("shape", [(2, 25, 64, 50), (8, 200, 768, 30522)])
def test_embed_bwd(dev, shape, case):
    """(d) dense word / position gradients vs torch.nn.functional.embedding's
    autograd in fp64 on the CPU with padding_idx = 0 (HF). The longest sum is
    B*T = 1600 terms: relative 1e-5 of the largest gradient entry."""
    B, T, D, V = shape
    P = 512
    gen = torch.Generator().manual_seed(71)
    ids = _embed_case(case, B, T, V, gen)
    dx = torch.randn((B * T, D), generator=gen)
    word = torch.zeros((V, D), dtype=torch.float64, requires_grad=True)
    pos = torch.zeros((P, D), dtype=torch.float64, requires_grad=True)
    out = torch.nn.functional.embedding(ids, word, padding_idx=0) + pos[:T].unsqueeze(0)
    (out.view(B * T, D) * dx.double()).sum().backward()
    wd, pd = torch.empty((V, D), device=dev), torch.empty((P, D), device=dev)
    wd.fill_(float("nan"))
    pd.fill_(float("nan"))
    ids_d, dx_d = ids.to(dev), dx.to(dev)
    dword, dpos = K.embed_bwd(dx_d, ids_d, wd, pd, padding_idx=0, dword=wd, dpos=pd)
    gw, gp = dword.cpu().double(), dpos.cpu().double()
    werr = (gw - word.grad).abs().max().item() / word.grad.abs().max().item()
    perr = (gp - pos.grad).abs().max().item() / pos.grad.abs().max().item()
    print(f"embed_bwd word rel {werr:.3e} pos rel {perr:.3e}")
    assert werr < 1e-5 and perr < 1e-5
    assert (gw[0] == 0).all()
    untouched = torch.ones(V, dtype=torch.bool)
    untouched[ids.view(-1)] = False
    assert (gw[untouched] == 0).all() and (gp[T:] == 0).all()
    w2, p2 = K.embed_bwd(dx_d, ids_d, wd, pd, padding_idx=0)
    assert torch.equal(w2, dword) and torch.equal(p2, dpos)
    # padding_idx = -1: torch's default, row 0 takes its gradient
    if case == "with_pad":
        w3, _ = K.embed_bwd(dx_d, ids_d, wd, pd, padding_idx=-1)
        ref0 = dx.double().view(B, T, D)[ids == 0].sum(0)
        assert (w3[0].cpu().double() - ref0).abs().max().item() < 1e-5 * ref0.abs().max().item()
        assert torch.equal(w3[1:], dword[1:])
