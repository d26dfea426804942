"""fp8 path (C4, BASELINE.json configs[4]): quantisation kernels bit-exact
against torch's OCP float8 conversion, the block-scaled fp8 GEMM against an
fp64 product of the dequantised operands, and the ViT-L/14@336 model in fp8
against the CPU oracle and the bf16 path (documented tolerances)."""
import pytest
import torch

from mae_clip_amd import kernels as K
from tests.helpers import build_pair, make_batch

pytestmark = pytest.mark.gpu

F8 = {K.FP8_E4M3: (torch.float8_e4m3fn, 448.0), K.FP8_E5M2: (torch.float8_e5m2, 57344.0)}


def _rows_input(rows, cols, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * torch.logspace(-6, 3, rows).view(-1, 1)
    x[3] = 0.0                                   # amax 0 -> scale 1
    x[5, 7] = 1e4                                # outlier row
    return x.to(dtype).to(dev)


def _ref_rows(x, fmt):
    tdt, fmax = F8[fmt]
    xf = x.float().cpu()
    amax = xf.abs().amax(1)
    s = torch.where(amax > 0, amax / fmax, torch.ones_like(amax))
    q = (xf * (1.0 / s).view(-1, 1)).to(tdt)     # the kernel multiplies by 1/s, RNE
    return q, s


@pytest.mark.parametrize("fmt", [K.FP8_E4M3, K.FP8_E5M2])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("cols", [512, 1024, 4096, 5120])
def test_quant_rows_bit_exact(dev, fmt, dtype, cols):
    x = _rows_input(37, cols, dtype, dev, seed=cols)
    out = K.quant_rows_fp8(x, fmt)
    q_ref, s_ref = _ref_rows(x, fmt)
    assert torch.equal(out.s.cpu(), s_ref)
    assert torch.equal(out.q.cpu(), q_ref.view(torch.uint8))


@pytest.mark.parametrize("D", [512, 768, 1024])
@pytest.mark.parametrize("fmt", [K.FP8_E4M3, K.FP8_E5M2])
def test_layernorm_fused_fp8_copy_bit_exact(dev, D, fmt):
    """The LayerNorm forward / backward fill the fp8 operand of the next GEMM
    themselves (the quantisation pass fused): identical bytes and scales to
    quant_rows_fp8 of the bf16 output they store (y; the dx copy)."""
    M = 300
    g = torch.Generator().manual_seed(D + fmt)
    x = (torch.randn(M, D, generator=g) * 3 + 1).to(dev)
    x[4] = 0.0                                         # constant row: y = beta
    gam = (torch.rand(D, generator=g) + 0.5).to(dev)
    bet = (torch.randn(D, generator=g) * 0.1).to(dev)
    q = K.new_fp8_rows(M, D, fmt, x.device)
    y, mean, rstd, _, _ = K.ln_fwd(x, gam, bet, 1e-6, out_dtype=torch.bfloat16, q8=q)
    r = K.quant_rows_fp8(y, fmt)
    assert torch.equal(q.s, r.s) and torch.equal(q.q, r.q)
    dy = (torch.randn(M, D, generator=g) * 1e-3).to(torch.bfloat16).to(dev)
    dres = (torch.randn(M, D, generator=g) * 1e-3).to(dev)
    qb = K.new_fp8_rows(M, D, fmt, x.device)
    dx, dxb, _, _, _ = K.ln_bwd(dy, x, mean, rstd, gam, dres=dres, want_bf16=True, q8=qb)
    rb = K.quant_rows_fp8(dxb, fmt)
    assert torch.equal(qb.s, rb.s) and torch.equal(qb.q, rb.q)


@pytest.mark.parametrize("fmt", [K.FP8_E4M3, K.FP8_E5M2])
def test_rows_colsum_fused_fp8_rows(dev, fmt):
    """The fp8 stack's top gradient: rows_colsum writes the bf16 copy and its fp8
    rows in one pass, bit-identical to quant_rows_fp8 of the bf16 copy."""
    g = torch.Generator().manual_seed(5 + fmt)
    x = (torch.randn(300, 1024, generator=g) * torch.logspace(-4, 2, 300).view(-1, 1)).to(dev)
    x[9] = 0.0
    xb = torch.empty_like(x, dtype=torch.bfloat16)
    q = K.new_fp8_rows(300, 1024, fmt, dev)
    part = K.rows_colsum(x, out_bf16=xb, q8=q)
    r = K.quant_rows_fp8(xb, fmt)
    assert torch.equal(q.q, r.q) and torch.equal(q.s, r.s)
    assert torch.equal(xb, x.to(torch.bfloat16))
    assert (part.sum(0) - x.sum(0)).abs().max().item() < 1e-3 * x.abs().max().item()


def test_quant_cols_bit_exact(dev):
    g = torch.Generator().manual_seed(7)
    w = (torch.randn(200, 136, generator=g) * torch.logspace(-3, 1, 136)).to(dev)
    out = K.quant_cols_fp8(w)
    q_ref, s_ref = _ref_rows(w.t().contiguous(), K.FP8_E4M3)
    assert out.q.shape == (136, 200)
    assert torch.equal(out.s.cpu(), s_ref)
    assert torch.equal(out.q.cpu(), q_ref.view(torch.uint8))


def _deq(op):
    tdt = F8[op.fmt][0]
    return op.q.cpu().view(tdt).double() * op.s.cpu().double().view(-1, 1)


def _fp8_plan(dev, M, N, Kd, blocks=False):
    """K.gemm_plan of an fp8 launch of this shape (a workspace offered) under the current options with the
    device's CU count"""
    from mae_clip_amd import _lib as L
    a = L.GemmArgs(A=16, B=16, C=16, M=M, N=N, K=Kd, lda=Kd, ldb=Kd, ldc=N, batch=1, dtype=K.FP8_E4M3,
                   out_dtype=L.F32, a_layout=0, b_layout=0, alpha=1.0, splitk=1, workspace=None if blocks else 16)
    return K.gemm_plan(a, torch.cuda.get_device_properties(dev).multi_processor_count,
                       fp8="blocks" if blocks else "rows")


@pytest.mark.parametrize("bm", ["auto", "192", "sk", "sk192"])
@pytest.mark.parametrize("afmt", [K.FP8_E4M3, K.FP8_E5M2])
@pytest.mark.parametrize("mnk", [(512, 384, 256), (1000, 768, 1024), (2308, 512, 2048), (9280, 1024, 512)])
def test_gemm_fp8_vs_dequantised_fp64(dev, afmt, mnk, bm, opts):
    """C = (s_A q_A)(s_B q_B)^T: the operands are exact in fp64, so the only
    error is the fp32 accumulation (and the bf16 / fp32 output rounding).
    bm = "192": the 192-row tile variant forced (N = 1024 at M = 9280 picks it
    by itself, like the C4 encoder's N = 1024 shapes)."""
    if bm in ("192", "sk192"):
        opts(GEMM_BM=192)
    if bm.startswith("sk"):   # stream-K forced wherever the tiles leave a partial last round
        opts(GEMM_SK=1)
    M, N, Kd = mnk
    p = _fp8_plan(dev, M, N, Kd)
    if bm in ("192", "sk192"):
        assert p["bm"] == 192, p
    assert p["S"] in ((0, 2) if bm.startswith("sk") else (0,)) and (p["S"] == 0 or p["bm"] == 192), p
    g = torch.Generator().manual_seed(M + N)
    x = (torch.randn(M, Kd, generator=g) * 3).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, Kd, generator=g) * 0.05).to(dev)
    A = K.quant_rows_fp8(x, afmt)
    B = K.quant_rows_fp8(w, K.FP8_E4M3)
    ref = _deq(A) @ _deq(B).t()
    bias = torch.randn(N, generator=g).to(dev)
    y = K.linear_fp8(A, B, out_dtype=torch.float32)
    sc = ref.abs().max().item()
    tol = 5e-6 * Kd ** 0.5          # fp32 accumulation of exact products (+ the scale multiply)
    assert (y.double().cpu() - ref).abs().max().item() / sc < tol
    # epilogues of the stack: GELU' (bf16 out + aux), residual (fp32), mul-aux
    d = torch.empty((M, N), device=dev, dtype=torch.bfloat16)
    y4 = K.linear_fp8(A, B, bias=bias, epilogue=K.EPI_GELU_D, aux_out=d)
    r64 = (ref + bias.double().cpu()).requires_grad_(True)
    gl = torch.nn.functional.gelu(r64)
    gd = torch.autograd.grad(gl.sum(), r64)[0]
    assert (y4.double().cpu() - gl.detach()).abs().max().item() < 1e-2 * max(1.0, gl.abs().max().item())
    assert (d.double().cpu() - gd).abs().max().item() < 2e-2
    res = torch.randn(M, N, generator=g).to(dev)
    y2 = K.linear_fp8(A, B, bias=bias, out_dtype=torch.float32, epilogue=K.EPI_RESID, resid=res)
    assert (y2.double().cpu() - (ref + bias.double().cpu() + res.double().cpu())).abs().max().item() < tol * sc + 1e-5
    aux = torch.rand(M, N, generator=g).to(torch.bfloat16).to(dev)
    y5 = K.linear_fp8(A, B, epilogue=K.EPI_MUL_AUX, aux=aux)
    ref5 = ref * aux.double().cpu()
    assert (y5.double().cpu() - ref5).abs().max().item() < 1e-2 * ref5.abs().max().item()


# ------------------------------------------------------------- fp8 blocks
def _scale_off(r, b, T):
    """byte offset of (row r, 32-block b) in the GEMM-layout scale tensor
    (include/maeclip.h "fp8 blocks"), numpy restatement of common.h mc_fp8b_off"""
    return (((r >> 6) * T + (b >> 2)) << 8) | ((b & 3) << 6) | ((r & 15) << 2) | ((r >> 4) & 3)


def _ref_blocks(x, fmt):
    """torch restatement of maeclip_quant_blocks_fp8: e from the bits of the
    block amax (the smallest 2^(e-127) with amax / 2^(e-127) <= FMT_MAX), q =
    rne(x 2^(127-e)) by torch's OCP float8 cast; returns (q bytes [rows, cols],
    e [rows, cols / 32])"""
    tdt, _ = F8[fmt]
    xf = x.float().cpu()
    rows, cols = xf.shape
    amax = xf.abs().view(rows, cols // 32, 32).amax(-1)
    u = amax.view(torch.int32).long()
    e = (u >> 23) - (15 if fmt == K.FP8_E5M2 else 8) + ((u & 0x7FFFFF) > 0x600000).long()
    e = e.clamp(min=0)
    inv = ((254 - e) << 23).to(torch.int32).view(torch.float32)
    q = (xf.view(rows, cols // 32, 32) * inv.unsqueeze(-1)).view(rows, cols).to(tdt)
    return q.view(torch.uint8), e.to(torch.uint8)


def _scales_to_rc(e_dev, rows, cols):
    """the kernel's scale tensor -> [rows, cols / 32] (row, block) order"""
    e = e_dev.cpu()
    T = cols // 128
    r = torch.arange(rows).view(-1, 1)
    b = torch.arange(cols // 32).view(1, -1)
    return e[_scale_off(r, b, T)]


def _deq_blocks(op):
    rows, cols = op.q.shape
    tdt = F8[op.fmt][0]
    e = _scales_to_rc(op.e, rows, cols).double()
    return (op.q.cpu().view(tdt).double().view(rows, cols // 32, 32) * torch.pow(2.0, e - 127).unsqueeze(-1)).view(
        rows, cols)


@pytest.mark.parametrize("fmt", [K.FP8_E4M3, K.FP8_E5M2])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", [(37, 512), (200, 1024), (64, 4096), (300, 640)])
def test_quant_blocks_bit_exact(dev, fmt, dtype, shape):
    """fp8 blocks vs the torch restatement: identical fp8 bytes and e8m0
    exponents (at their GEMM-layout offsets); zero blocks, outliers, a 2^-20
    .. 2^10 magnitude range; |x - 2^(e-127) q| within the format's rounding."""
    rows, cols = shape
    x = _rows_input(rows, cols, dtype, dev, seed=rows + cols)
    x[7, 32:64] = 0.0
    out = K.quant_blocks_fp8(x, fmt)
    q_ref, e_ref = _ref_blocks(x, fmt)
    assert torch.equal(out.q.cpu(), q_ref)
    assert torch.equal(_scales_to_rc(out.e, rows, cols), e_ref)
    if fmt == K.FP8_E4M3:
        xr, xd = x.double().cpu(), _deq_blocks(out)
        sc = torch.pow(2.0, _scales_to_rc(out.e, rows, cols).double() - 127).repeat_interleave(32, 1)
        assert ((xd - xr).abs() <= 2.0 ** -4 * xr.abs() + sc * 2.0 ** -10 + 1e-30).all()


@pytest.mark.parametrize("afmt", [K.FP8_E4M3, K.FP8_E5M2])
@pytest.mark.parametrize("mnk", [(512, 384, 256), (1000, 768, 1024), (2308, 512, 2048), (9280, 1024, 512),
                                 (18560, 1024, 4096)])
def test_gemm_fp8_blocks_vs_dequantised_fp64(dev, afmt, mnk):
    """fp8-blocks A (the MFMA applies the e8m0 block scales) x per-channel B:
    vs the fp64 product of the dequantised operands (exact in fp64: only the
    fp32 accumulation differs), with the epilogues the fp8 stack runs on it
    (plain bf16, fp32 residual); A rows with blocks 2^30 apart in magnitude so
    a wrong scale byte cannot hide. (18560, 1024, 4096): the C4 encoder's fc2."""
    M, N, Kd = mnk
    p = _fp8_plan(dev, M, N, Kd, blocks=True)
    assert (p["bm"], p["S"]) == (192, 0), p
    g = torch.Generator().manual_seed(M + N + 1)
    x = torch.randn(M, Kd, generator=g) * 3
    x[:, : Kd // 2] *= 2.0 ** -15
    x[::7, 96:128] *= 2.0 ** 15
    x = x.to(torch.bfloat16).to(dev)
    w = (torch.randn(N, Kd, generator=g) * 0.05).to(dev)
    A = K.quant_blocks_fp8(x, afmt)
    B = K.quant_rows_fp8(w, K.FP8_E4M3)
    ref = _deq_blocks(A) @ _deq(B).t()
    y = K.linear_fp8(A, B, out_dtype=torch.float32)
    sc = ref.abs().max().item()
    tol = 5e-6 * Kd ** 0.5
    assert (y.double().cpu() - ref).abs().max().item() / sc < tol
    bias = torch.randn(N, generator=g).to(dev)
    res = torch.randn(M, N, generator=g).to(dev)
    y2 = K.linear_fp8(A, B, bias=bias, out_dtype=torch.float32, epilogue=K.EPI_RESID, resid=res)
    assert (y2.double().cpu() - (ref + bias.double().cpu() + res.double().cpu())).abs().max().item() < tol * sc + 1e-5
    yb = K.linear_fp8(A, B)
    assert (yb.double().cpu() - ref).abs().max().item() < 1e-2 * sc


@pytest.mark.parametrize("path", ["bf16", "bf16_192", "fp8rows", "fp8blocks"])
@pytest.mark.parametrize("fmt", [K.FP8_E4M3, K.FP8_E5M2])
def test_gemm_epilogue_fp8_blocks_output(dev, path, fmt, opts):
    """A GEMM epilogue that writes its bf16 output's fp8 blocks itself
    (maeclip_gemm_args q8: the fc1 GELU' and fc2-dgrad mul-aux launches of the
    fp8 stack) gives the same bytes and exponents as maeclip_quant_blocks_fp8 of
    the stored bf16 output: GELU' (+ aux_out), mul-aux with column sums
    (256-row tile), plain; ragged M (a partial last tile)."""
    M, N, Kd = 1000, 1024, 512
    g = torch.Generator().manual_seed(17 + fmt)
    x = (torch.randn(M, Kd, generator=g)).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, Kd, generator=g) * 0.05).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    aux = torch.rand(M, N, generator=g).to(torch.bfloat16).to(dev)
    if path == "bf16_192":
        opts(GEMM_BM=192)
        from mae_clip_amd import _lib as L
        a = L.GemmArgs(A=16, B=16, C=16, M=M, N=N, K=Kd, lda=Kd, ldb=Kd, ldc=N, batch=1, dtype=L.BF16,
                       out_dtype=L.BF16, a_layout=0, b_layout=0, alpha=1.0, splitk=1)
        p = K.gemm_plan(a, torch.cuda.get_device_properties(dev).multi_processor_count)
        assert (p["route"], p["bm"], p["S"]) == (4, 192, 0), p
    elif path == "fp8blocks":
        assert _fp8_plan(dev, M, N, Kd, blocks=True)["bm"] == 192
    if path.startswith("bf16"):
        wb = w.to(torch.bfloat16)

        def run(q8, epilogue=K.EPI_NONE, bias=None, aux=None, aux_out=None, colsum=None):
            y = torch.empty((M, N), device=dev, dtype=torch.bfloat16)
            K.gemm(x, wb, y, M, N, Kd, Kd, Kd, N, epilogue=epilogue, bias=bias, aux=aux, aux_out=aux_out,
                   ldaux=N if (aux is not None or aux_out is not None) else 0, colsum=colsum, q8=q8)
            return y
    else:
        A = K.quant_rows_fp8(x, K.FP8_E4M3) if path == "fp8rows" else K.quant_blocks_fp8(x, K.FP8_E4M3)
        B = K.quant_rows_fp8(w, K.FP8_E4M3)
        run = lambda **kw: K.linear_fp8(A, B, **kw)
    cases = [dict(bias=bias, epilogue=K.EPI_GELU_D, aux_out=torch.empty((M, N), device=dev, dtype=torch.bfloat16)),
             dict(epilogue=K.EPI_MUL_AUX, aux=aux), dict(bias=bias)]
    if path != "fp8blocks":   # column sums: 256-row tiles (per-row / bf16 A only)
        cases.append(dict(epilogue=K.EPI_MUL_AUX, aux=aux,
                          colsum=torch.empty((K.gemm_colsum_rows(M), N), device=dev, dtype=torch.float32)))
    for kw in cases:
        q8 = K.new_fp8_blocks(M, N, fmt, dev)
        y = run(q8=q8, **kw)
        r = K.quant_blocks_fp8(y, fmt)
        assert torch.equal(q8.q, r.q), kw.get("epilogue")
        assert torch.equal(_scales_to_rc(q8.e, M, N), _scales_to_rc(r.e, M, N)), kw.get("epilogue")


@pytest.mark.parametrize("shape", [(2, 145, 4, 64), (2, 50, 2, 64), (3, 197, 4, 32), (1, 577, 4, 32), (2, 197, 2, 64)])
@pytest.mark.parametrize("fmt", [K.FP8_E4M3, K.FP8_E5M2])
def test_attention_fp8_blocks_output(dev, shape, fmt):
    """The attention forward / backward write the fp8 blocks of o / dqkv (the
    proj forward's and the qkv dgrad's fp8 operands) from their own stores:
    the same bytes and exponents as maeclip_quant_blocks_fp8 of the bf16
    output. (145, hd 64): the C4 encoder; (197, hd 32): the diagonal backward,
    which takes the standalone pass; (577, hd 32): the 16-wave kernels."""
    B, n, H, hd = shape
    g = torch.Generator().manual_seed(n + H)
    qkv = (torch.randn(B * n, 3 * H * hd, generator=g)).to(torch.bfloat16).to(dev)
    D = H * hd
    q8 = K.new_fp8_blocks(B * n, D, fmt, dev)
    o, lse = K.attn_fwd(qkv, B, n, H, hd, hd ** -0.5, q8=q8)
    r = K.quant_blocks_fp8(o, fmt)
    assert torch.equal(q8.q, r.q)
    assert torch.equal(_scales_to_rc(q8.e, B * n, D), _scales_to_rc(r.e, B * n, D))
    dout = (torch.randn(B * n, D, generator=g) * 1e-2).to(torch.bfloat16).to(dev)
    d8 = K.new_fp8_blocks(B * n, 3 * D, fmt, dev)
    dqkv, _ = K.attn_bwd(qkv, o, dout, lse, B, n, H, hd, hd ** -0.5, q8=d8)
    r = K.quant_blocks_fp8(dqkv, fmt)
    assert torch.equal(d8.q, r.q)
    assert torch.equal(_scales_to_rc(d8.e, B * n, 3 * D), _scales_to_rc(r.e, B * n, 3 * D))


def test_fp8_quantisation_error_is_bounded(dev):
    """e4m3 rows: |x - s q| <= 2^-4 |x| + s 2^-10 per element (3 mantissa bits,
    RNE; subnormal step 2^-9 s) -- the operand error the fp8 GEMM adds."""
    x = (torch.randn(64, 1024) * 2).to(torch.bfloat16).to(dev)
    A = K.quant_rows_fp8(x, K.FP8_E4M3)
    xd = _deq(A)
    xr = x.double().cpu()
    bound = 2.0 ** -4 * xr.abs() + A.s.cpu().double().view(-1, 1) * 2.0 ** -10
    assert ((xd - xr).abs() <= bound + 1e-12).all()


@pytest.mark.parametrize("gfmt", ["e4m3", "e5m2"])
def test_vitl14_336_fp8_vs_oracle_and_bf16(dev, gfmt):
    """C4 shapes (ViT-L/14 @336, encoder cut to 4 blocks, B = 4; decoder 2 x 512,
    n = 577): fp8 stack GEMMs (e4m3 forward; the gradient operand in e4m3, the
    default, or e5m2; per-token scales from the LayerNorms, fp8 blocks from the
    GEMM epilogues and the attention, per-channel weight scales) and the bf16
    path vs the fp64 CPU oracle (forward AND backward) on the same weights.
    Tolerances FP8_TOL_BY_FMT (about 2x the values measured on MI355X): loss
    relative; every trainable gradient's relative L2 error vs the ORACLE's (bf16:
    BF16_C4_TOL); fp8 vs bf16."""
    from tests.helpers import record_parity
    kw = dict(model_name="vit_large_patch14_336", size=336, image_embedding=1024, text_layers=2, mask_ratio=0.75,
              decoder_embed_dim=512, decoder_depth=2, decoder_num_heads=16, vit_depth=4)
    batch = make_batch(4, 336)
    out = {}
    from tests.helpers import product_config
    for prec in ("fp8", "bf16"):
        with product_config(fp8_grad_format=gfmt):
            prod, ref = build_pair(prec, **kw)
        prod.eval()
        with product_config(fp8_grad_format=gfmt):
            loss = prod({k: v.to(dev) for k, v in batch.items()})
            loss.backward()
        torch.cuda.synchronize()
        out[prec] = (loss.item(), {n: p.grad.detach().double().cpu() for n, p in prod.named_parameters()
                                   if p.requires_grad})
    ref.eval()
    rl = ref(dict(batch, image=batch["image"].double()))
    rl.backward()
    rloss = rl.item()
    rg = {n: p.grad.detach() for n, p in ref.named_parameters() if p.grad is not None}
    l8, g8 = out["fp8"]
    lb, gb = out["bf16"]

    def worst_rel(g, base):
        w, wn = 0.0, None
        for n, b in base.items():
            assert torch.isfinite(g[n]).all(), n
            den = b.norm().item()
            if den > 0:
                e = (g[n] - b).norm().item() / den
                if e > w:
                    w, wn = e, n
        return w, wn

    w8o, n8o = worst_rel(g8, rg)
    wbo, nbo = worst_rel(gb, rg)
    w8b, _ = worst_rel(g8, gb)
    r8 = abs(l8 - rloss) / max(1.0, abs(rloss))
    rb = abs(lb - rloss) / max(1.0, abs(rloss))
    record_parity(f"vitl14_336_fp8_vs_oracle_grad_{gfmt}", loss_rel=r8, worst_grad_relL2=w8o, worst_grad=n8o,
                  worst_grad_relL2_vs_bf16=w8b)
    record_parity("vitl14_336_bf16_vs_oracle_grads", loss_rel=rb, worst_grad_relL2=wbo, worst_grad=nbo)
    tol = FP8_TOL_BY_FMT[gfmt]
    assert r8 < tol[0], (l8, lb, rloss)
    assert w8o < tol[1], (w8o, n8o)
    assert wbo < BF16_C4_TOL, (wbo, nbo)
    assert w8b < tol[2], w8b


# (loss rel, worst grad rel-L2 vs the oracle, vs bf16) per gradient format, about 2x
# the measurements (r06, fp8 blocks + per-row operands: e4m3 0.0115 / 0.082 / 0.082,
# e5m2 0.0115 / 0.110 / 0.111; profiles/r06/parity_r6d.jsonl)
FP8_TOL_BY_FMT = {"e4m3": (2.5e-2, 0.16, 0.16), "e5m2": (2.5e-2, 0.2, 0.2)}
BF16_C4_TOL = 1.25e-2           # measured r03: 0.0061


def test_batched_weight_quantisation_matches_single(dev):
    """maeclip_quant_weights_fp8 (all stack weights in two launches) ==
    the per-weight quant_rows_fp8 / quant_cols_fp8, bit for bit, over weights of
    different shapes (row counts not multiples of 64 / 256; K = 5120 is past the
    batched call's 4096 columns and takes the per-weight launches)."""
    g = torch.Generator().manual_seed(3)
    shapes = [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096), (200, 136), (72, 512), (96, 5120)]
    ws = [(torch.randn(s, generator=g) * torch.logspace(-2, 1, s[1])).to(dev) for s in shapes]
    plan = K.Fp8WeightPlan(ws, dev)
    assert plan.n == len(shapes) - 1 and len(plan.single) == 1
    plan.run()
    for w, (wq, wt) in zip(ws, plan.ops):
        r = K.quant_rows_fp8(w, K.FP8_E4M3)
        c = K.quant_cols_fp8(w)
        assert torch.equal(wq.q, r.q) and torch.equal(wq.s, r.s)
        assert torch.equal(wt.q, c.q) and torch.equal(wt.s, c.s)


