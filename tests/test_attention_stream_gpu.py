"""The streamed bf16 attention kernels (attention.hip, option ATTN_STREAM):
sequences past the LDS-resident limit (n = 576 at hd 64; 1216 forward / 1152
backward at hd 32) run by default, and the same kernels forced at the smallest
shapes where a ring of 64-row blocks can go wrong. Reference: fp64 softmax
attention and fp64 autograd on the CPU, computed once per shape. Bounds are
those of test_kernels_gpu.py::test_attention_fwd_bwd; none is widened for the
long shapes."""
import functools
import math

import pytest
import torch

from mae_clip_amd import kernels as K
from tests import attn_cases as A
from tests.helpers import build_pair, make_batch, product_config, record_parity, same_bits

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# (B, n, H, hd). LONG: past the resident limit with no option set (1153 at hd
# 32: resident forward, streamed backward). SMALL: less than one 16-row tile,
# one tile, exactly one block, one block + 1 key (tail of 1 tile), two blocks +
# 2 keys with two row blocks of 128, the decoder's 197, four whole blocks, and
# B * H = 6 workgroup groups (not a multiple of the 8 XCDs).
LONG = [(1, 577, 2, 64), (1, 1025, 1, 64), (1, 1217, 1, 32), (1, 1153, 1, 32)]
SMALL = [(3, 5, 2, 32), (1, 16, 1, 64), (1, 64, 2, 64), (1, 65, 1, 32), (2, 130, 2, 64), (1, 197, 2, 32),
         (2, 256, 2, 64), (2, 145, 3, 64)]


def _rand(shape, dtype, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _attn_ref(qkv, B, n, H, hd, scale):
    q, k, v = qkv.double().view(B, n, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * scale
    lse2 = torch.logsumexp(s, -1) / math.log(2.0)   # [B, H, n], log2 domain
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B * n, H * hd), lse2


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs (CPU bf16) and the fp64 reference of one shape; never modified"""
    B, n, H, hd = shape
    scale = hd ** -0.5
    qkv = _rand((B * n, 3 * H * hd), BF, seed=11)
    dout = _rand((B * n, H * hd), BF, seed=12)
    x64 = qkv.double().requires_grad_(True)
    ref, lse2 = _attn_ref(x64, B, n, H, hd, scale)
    (ref * dout.double()).sum().backward()
    return dict(qkv=qkv, dout=dout, ref=ref.detach(), lse2=lse2.detach(), g=x64.grad, scale=scale)


def _fwd(dev, shape, **kw):
    B, n, H, hd = shape
    c = _case(shape)
    return K.attn_fwd(c["qkv"].to(dev), B, n, H, hd, c["scale"], **kw)


def _bwd(dev, shape, o, lse, **kw):
    B, n, H, hd = shape
    c = _case(shape)
    return K.attn_bwd(c["qkv"].to(dev), o, c["dout"].to(dev), lse, B, n, H, hd, c["scale"], **kw)


def _check_fwd(shape, o):
    err = (o.double().cpu() - _case(shape)["ref"]).abs().max().item()
    print(f"[stream] {shape} fwd max|o - ref| {err:.3e}")
    assert err < 2e-2, err


def _check_bwd(shape, dqkv, part):
    B, n, H, hd = shape
    c = _case(shape)
    g = c["g"]
    gs = g.abs().max().item()
    err = (dqkv.double().cpu() - g).abs().max().item() / gs
    cs = part.double().cpu().sum(0)
    gsum = g.view(B * n, 3, H * hd).sum(0)
    cerr = (cs - gsum.view(-1)).abs().max().item() / (gs * n)
    verr = (cs.view(3, -1)[2] - c["dout"].double().sum(0)).abs().max().item()
    print(f"[stream] {shape} bwd rel {err:.3e} colsum rel {cerr:.3e} v-slice abs {verr:.3e}")
    assert err < 3e-2, err
    assert cerr < 3e-2, cerr
    assert (part.cpu().view(B, 3, -1)[:, 1] == 0).all()
    assert verr < 1e-4 * max(1.0, n ** 0.5), verr


def _lse_dev(shape, lse):
    return (lse.double().cpu() - _case(shape)["lse2"]).abs().max().item()


@functools.lru_cache(maxsize=None)
def _resident_lse_worst():
    """worst deviation of the RESIDENT forward's lse from fp64 over the shapes
    both paths take, measured in this run (the long shapes' yardstick)"""
    dev = torch.device("cuda:0")
    prev = K.set_option("ATTN_STREAM", 0)
    try:
        return max(_lse_dev(s, _fwd(dev, s)[1]) for s in SMALL)
    finally:
        K.set_option("ATTN_STREAM", prev)


@pytest.mark.parametrize("shape", LONG)
def test_long_sequences_run_by_default(dev, shape):
    """no option set: forward, backward and bias partials against fp64. Before
    the streamed kernels these calls were rejected ("needs ... B of LDS")."""
    assert K.get_option("ATTN_STREAM") == -1
    B, n, H, hd = shape
    # (1, 1153, 1, 32): the resident forward (16 waves) still holds it, the backward streams
    assert A.path(BF, n, H, hd, False, B=B) == (A.FWD16 if shape == (1, 1153, 1, 32) else A.STREAM)
    assert A.path(BF, n, H, hd, True, B=B) == A.STREAM
    o, lse = _fwd(dev, shape)
    _check_fwd(shape, o)
    dqkv, part = _bwd(dev, shape, o, lse)
    _check_bwd(shape, dqkv, part)
    d, worst = _lse_dev(shape, lse), _resident_lse_worst()
    record_parity("attn_stream_lse_long", shape=str(shape), lse_dev=d, resident_worst=worst)
    assert d <= 2 * worst, (d, worst)


@pytest.mark.parametrize("shape", SMALL)
def test_forced_at_small_shapes(dev, shape, opts):
    B, n, H, hd = shape
    opts(ATTN_STREAM=0)
    assert A.path(BF, n, H, hd, False, B=B) == A.FWD   # every SMALL shape: the 8-wave resident forward
    _, lse_r = _fwd(dev, shape)
    opts(ATTN_STREAM=1)
    assert A.path(BF, n, H, hd, False, B=B) == A.path(BF, n, H, hd, True, B=B) == A.STREAM
    o, lse = _fwd(dev, shape)
    _check_fwd(shape, o)
    dqkv, part = _bwd(dev, shape, o, lse)
    _check_bwd(shape, dqkv, part)
    # the summation order across blocks is all that may differ from the resident kernel
    ds, dr = _lse_dev(shape, lse), _lse_dev(shape, lse_r)
    record_parity("attn_stream_lse", shape=str(shape), streamed=ds, resident=dr)
    assert ds <= 2 * dr, (ds, dr)


def test_streamed_and_resident_interchange(dev, opts):
    """o / lse are one convention: each forward feeds the other path's backward"""
    shape = (1, 197, 2, 64)
    for f, b in ((1, 0), (0, 1)):
        opts(ATTN_STREAM=f)
        assert A.path(BF, 197, 2, 64, False) == (A.STREAM if f else A.FWD)
        o, lse = _fwd(dev, shape)
        _check_fwd(shape, o)
        opts(ATTN_STREAM=b)
        assert A.path(BF, 197, 2, 64, True) == (A.STREAM if b else A.BWD_DIAG)
        _check_bwd(shape, *_bwd(dev, shape, o, lse))


def test_deterministic(dev):
    shape = (2, 577, 2, 64)
    assert A.path(BF, 577, 2, 64, False, B=2) == A.path(BF, 577, 2, 64, True, B=2) == A.STREAM
    runs = []
    for _ in range(2):
        o, lse = _fwd(dev, shape)
        dqkv, part = _bwd(dev, shape, o, lse)
        runs.append((o, lse, dqkv, part))
    for a, b in zip(*runs):
        assert same_bits(a, b)


@pytest.mark.parametrize("shape", [(2, 197, 2, 64), (1, 577, 2, 32)])
def test_no_change_below_the_limit(dev, shape, opts):
    """an unset option routes every shape that ran before exactly as ATTN_STREAM = 0"""
    runs = []
    B, n, H, hd = shape
    # hd 64, n = 197: 8-wave forward, diagonal backward; hd 32, n = 577: the 16-wave forward and backward
    want = (A.FWD, A.BWD_DIAG) if hd == 64 else (A.FWD16, A.BWD_16)
    for v in (None, 0):
        opts(ATTN_STREAM=v)
        assert (A.path(BF, n, H, hd, False, B=B), A.path(BF, n, H, hd, True, B=B)) == want
        o, lse = _fwd(dev, shape)
        dqkv, part = _bwd(dev, shape, o, lse)
        runs.append((o, lse, dqkv, part))
    for a, b in zip(*runs):
        assert same_bits(a, b)


def _scale_off(r, b, T):
    """byte offset of (row r, 32-block b) in the fp8-blocks scale tensor (common.h mc_fp8b_off)"""
    return (((r >> 6) * T + (b >> 2)) << 8) | ((b & 3) << 6) | ((r & 15) << 2) | ((r >> 4) & 3)


def _scales_to_rc(e_dev, rows, cols):
    e = e_dev.cpu()
    r = torch.arange(rows).view(-1, 1)
    b = torch.arange(cols // 32).view(1, -1)
    return e[_scale_off(r, b, cols // 128)]


@pytest.mark.parametrize("fmt", [K.FP8_E4M3, K.FP8_E5M2])
def test_fp8_blocks_copy(dev, fmt):
    """the q8 copy of o / dqkv (the standalone pass after the streamed kernels)
    is maeclip_quant_blocks_fp8 of the stored bf16 output, bit for bit"""
    shape = (1, 577, 2, 64)
    B, n, H, hd = shape
    D = H * hd
    q8 = K.new_fp8_blocks(B * n, D, fmt, dev)
    assert A.path(BF, n, H, hd, False, q8=True) == A.path(BF, n, H, hd, True, q8=True) == A.STREAM
    o, lse = _fwd(dev, shape, q8=q8)
    r = K.quant_blocks_fp8(o, fmt)
    assert torch.equal(q8.q, r.q)
    assert torch.equal(_scales_to_rc(q8.e, B * n, D), _scales_to_rc(r.e, B * n, D))
    d8 = K.new_fp8_blocks(B * n, 3 * D, fmt, dev)
    dqkv, _ = _bwd(dev, shape, o, lse, q8=d8)
    r = K.quant_blocks_fp8(dqkv, fmt)
    assert torch.equal(d8.q, r.q)
    assert torch.equal(_scales_to_rc(d8.e, B * n, 3 * D), _scales_to_rc(r.e, B * n, 3 * D))


def test_vitl14_336_unmasked_model(dev):
    """ViT-L/14 @336 with mask_ratio 0 (n = 577 at hd 64, the CLIP path and the
    inference flow), encoder cut to 2 blocks, B = 2: bf16 loss vs the fp64
    oracle (2e-2, as test_vitl14_336_shapes_bf16_vs_oracle), finite gradients,
    every trainable gradient within 5e-2 relative L2 of the fp32 parity model on
    the same weights (test_vitb_bf16_grads_match_fp32's bar; fp32 takes the
    rows path at this n), and get_image_embeddings vs the oracle's image tower."""
    from mae_clip_amd.CLIP import CLIPModel
    from mae_clip_amd.retrieval import get_image_embeddings
    kw = dict(model_name="vit_large_patch14_336", size=336, image_embedding=1024, text_layers=2, mask_ratio=0.0)
    prod, ref = build_pair("bf16", vit_depth=2, **kw)
    with product_config(precision="fp32", **kw):
        p32 = CLIPModel()
        p32.image_encoder.model.blocks = p32.image_encoder.model.blocks[:2]
    p32.load_state_dict(prod.state_dict())
    p32 = p32.to(dev).eval()
    prod.eval()
    ref.eval()
    batch = make_batch(2, 336)
    bd = {k: v.to(dev) for k, v in batch.items()}
    # the encoder's attention, 16 heads of 64 at n = 577: streamed in bf16, the rows kernels in fp32
    for dt, want in ((BF, A.STREAM), (torch.float32, A.ROWS)):
        assert A.path(dt, 577, 16, 64, False, B=2) == A.path(dt, 577, 16, 64, True, B=2) == want
    loss = prod(bd)
    loss.backward()
    p32(bd).backward()
    with torch.no_grad():
        rloss = ref(dict(batch, image=batch["image"].double())).item()
    assert abs(loss.item() - rloss) < 2e-2 * max(1.0, abs(rloss)), (loss.item(), rloss)
    g32 = dict(p32.named_parameters())
    bad = []
    for name, p in prod.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all().item(), name
        g, rg = p.grad.double(), g32[name].grad.double()
        rel = ((g - rg).norm() / (rg.norm() + 1e-30)).item()
        if not rel < 5e-2:
            bad.append((rel, name))
    assert not bad, sorted(bad, reverse=True)[:5]
    b1, b2 = make_batch(2, 336, seed=3), make_batch(2, 336, seed=4)
    emb = get_image_embeddings(prod, [b1["image"].to(dev), b2["image"].to(dev)])
    assert tuple(emb.shape) == (4, 256) and torch.isfinite(emb).all().item()
    with torch.no_grad():
        remb = torch.cat([ref.image_projection(ref.image_encoder.model(b["image"].double())) for b in (b1, b2)])
    err = (emb.double().cpu() - remb).abs().max().item()
    assert err < 2e-2 * max(1.0, remb.abs().max().item()), err


def test_captured_block_replays_bitwise(dev):
    """one transformer block at n = 577, hd 64, forward + backward, captured
    with torch.cuda.graph on the default queues and no option set: two replays
    equal the eager result bit for bit (the streamed path allocates and
    synchronises nothing)"""
    from mae_clip_amd import modules as Mo
    torch.manual_seed(0)
    blocks = torch.nn.ModuleList([Mo.Block(128, 2)]).to(dev)
    blocks[0].init_weights()
    cache = Mo.WeightCache()
    for p in blocks[0].gemm_weights():
        cache.register(p, p.shape)
    cache.refresh(BF)
    x0 = torch.randn(1, 577, 128, device=dev)
    gy = torch.randn(1, 577, 128, device=dev)
    assert A.path(BF, 577, 2, 64, False) == A.path(BF, 577, 2, 64, True) == A.STREAM   # 2 heads of 64

    def step():
        for p in blocks.parameters():
            p.grad = None
        x = x0.clone().requires_grad_()
        y = Mo.run_stack(blocks, x, 2, BF, cache)
        y.backward(gy)
        return [y.detach(), x.grad] + [p.grad for p in blocks.parameters()]

    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    replay = torch.cuda.current_stream().cuda_stream
    # as graph.CapturedStep captures: the capture stream shares the replay
    # stream's GEMM scratch, and the autograd thread may launch into it
    with torch.cuda.graph(graph, capture_error_mode="relaxed"):
        cap = torch.cuda.current_stream().cuda_stream
        K.alias_stream(cap, replay)
        try:
            out = step()
        finally:
            K.alias_stream(cap, None)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert same_bits(a, b)
