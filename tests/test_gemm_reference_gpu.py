"""Reference tests of the GEMM family (gemm_small.hip, gemm.hip "v1", gemm2.hip
"v2", gemm4.hip "v4" and the grouped weight gradient) on small shapes that sit
on every boundary: tile edges, the shortest legal K, a K ending inside a
K-tile, M = 1, both sides of each dispatcher limit, every epilogue, alpha /
beta / bias, batch strides, the caller's split-K and the kernels' own.

Cases and their CPU half are in tests/gemm_cases.py (operands in NaN-padded
allocations, outputs in sentinel-filled ones, the header's formula in fp64
and in fp32 torch). After each launch every output is finite, every byte
outside the addressed region is bitwise intact, and helpers.check holds: the
kernel's max error against fp64 <= 4 x E32, E32 the error of the same
statement in fp32 torch (a bf16 output adds the bf16 half-ulp at the
reference). Each group asserts the kernel it means to exercise by restating
the dispatcher (gemm_cases.predict) and, where a plan decides,
maeclip_gemm_workspace. Each check prints "[ratio] name kernel-error E32
ratio" (pytest -s); the maxima are tabulated in DESIGN.md section 4.

Out of reach of the argument checks: a row-contiguous operand with fewer than
8 rows (the condition that keeps it from v2) needs a row extent that is a
multiple of 8, and an extent of 0 returns before any launch, so no accepted
call leaves v2 for that reason; M = 1 and N = 8 run K-contiguous."""
import ctypes
import math

import pytest
import torch

from mae_clip_amd import _lib as L
from mae_clip_amd import kernels as K
from tests import gemm_cases as G
from tests.helpers import check, same_bits

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


def _launch(a):
    L.check(L.lib().maeclip_gemm(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), "maeclip_gemm")


def _intact(name, buf):
    vals, rest, orig = buf.read()
    assert same_bits(rest, orig), f"{name}: bytes outside the addressed region changed"
    assert torch.isfinite(vals.float()).all(), f"{name}: not every addressed value was written"
    return vals


def run_case(c, dev, opts):
    assert G.predict(c) == c.path, (c.id, G.predict(c))
    for k, v in c.opts:
        opts(**{k: v})
    d = G.build(c)
    bufs = d["bufs"]
    if c.plan_ws:
        # the plan's own scratch: gemm_small's K-slice partials, or the v4 split's arrival counters (zero before
        # the first launch, left zero by every launch) and partial tiles
        nb = G.plan_workspace(c)
        assert nb > 0, (c.id, "no split plan")
        n = nb // 4
        bufs["ws"] = G.Buf(F32, torch.arange(n), n, G.SENTINEL, torch.zeros(n), band=256)
    for b in bufs.values():
        b.to(dev)
    a = G.gemm_args(c, lambda name: bufs[name].ptr)
    _launch(a)
    torch.cuda.synchronize()
    r64, r32 = d["ref64"], d["ref32"]
    Cv = _intact(c.id + " C", bufs["C"])
    res = [("C", check(c.id + " C", Cv, r64["C"], r32["C"]))]
    if "aux_out" in bufs:
        av = _intact(c.id + " aux_out", bufs["aux_out"])
        res.append(("aux_out", check(c.id + " aux_out", av, r64["aux_out"], r32["aux_out"])))
    if c.colsum:
        rows = K.gemm_colsum_rows(c.M)
        assert rows == -(-c.M // 64)
        _intact(c.id + " colsum", bufs["colsum"])
        part = bufs["colsum"].dev[bufs["colsum"].lead:][:c.batch * rows * c.N].view(c.batch, rows, c.N)
        cs = torch.stack([K.colsum_reduce(part[z]) for z in range(c.batch)])
        res.append(("colsum", check(c.id + " colsum", cs, r64["colsum"], r32["colsum"])))
    if "ws" in bufs:
        wv, rest, orig = bufs["ws"].read()
        assert same_bits(rest, orig), f"{c.id}: workspace bytes beyond the plan changed"
        if c.S > 1:                          # every slab of the caller's split is written, an empty slice as zeros
            assert torch.isfinite(wv).all(), f"{c.id}: a split-K slab was not written"
        if c.path == "v4" and c.plan_ws:     # the arrival counters (first 16 KiB) are back to zero
            assert int(wv[:4096].view(torch.int32).abs().sum()) == 0
    for name in ("A", "B", "bias", "aux", "resid"):
        if name in bufs:
            assert same_bits(bufs[name].dev, bufs[name].orig), f"{c.id}: input {name} written"
    if c.S > 1 or c.plan_ws:
        # a repeat launch is bitwise equal (fixed summation order)
        bufs["C"].to(dev)
        a = G.gemm_args(c, lambda name: bufs[name].ptr)
        _launch(a)
        torch.cuda.synchronize()
        assert same_bits(bufs["C"].read()[0], Cv), f"{c.id}: repeat launch differs"
    return res


def _params(cases):
    return [pytest.param(c, id=c.id) for c in cases]


@pytest.mark.parametrize("c", _params(G.shape_cases()))
def test_gemm_shapes(dev, opts, c):
    """every path at its base and one size at a time: tile edges, the shortest K, K ending inside a K-tile,
    M = 1, both sides of 128 (v1 / v2), of 256 (v2 / v4) and of the gemm_small limit, every v4 tile height"""
    run_case(c, dev, opts)


@pytest.mark.parametrize("c", _params(G.scalar_cases()))
def test_gemm_alpha_beta_bias(dev, opts, c):
    run_case(c, dev, opts)


@pytest.mark.parametrize("c", _params(G.epilogue_cases()))
def test_gemm_epilogues(dev, opts, c):
    """epilogues 1 to 5, ldaux != ldc and ldr != ldc, aux_out and resid present and absent"""
    run_case(c, dev, opts)


@pytest.mark.parametrize("c", _params(G.small_split_cases()))
def test_gemm_small_k_split(dev, opts, c):
    """gemm_small's own K slices and small_reduce_kernel, every epilogue"""
    run_case(c, dev, opts)


@pytest.mark.parametrize("c", _params(G.colsum_cases()))
def test_gemm_colsum(dev, opts, c):
    """column-sum partials: maeclip_gemm_colsum_rows(M) rows, M on both sides of the 64-row groups, batch 3;
    rows beyond the documented count keep their sentinel"""
    run_case(c, dev, opts)


@pytest.mark.parametrize("c", _params(G.batch_cases()))
def test_gemm_batched(dev, opts, c):
    """batch = 3: own strides larger than dense, a shared B (strideB = 0), a shared A, and the epilogue
    operands advancing by z * strideC"""
    run_case(c, dev, opts)


@pytest.mark.parametrize("c", _params(G.splitk_cases()))
def test_gemm_explicit_splitk(dev, opts, c):
    """the caller's split-K on v1 fp32, v1 bf16, v2 and v4: an empty last slice, alpha, bias, beta, bf16
    output, batch 2; repeat launch bitwise equal; workspace beyond batch * S * M * N floats untouched"""
    run_case(c, dev, opts)


@pytest.mark.parametrize("c", _params(G.v4_split_cases()))
def test_gemm_v4_forced_split(dev, opts, c):
    """the in-launch split of 192-row tiles at the smallest shape that fits it; run_case sets the plan options
    and asserts that maeclip_gemm_workspace > 0 under them (a split plan was chosen)"""
    T = -(-c.M // 192) * -(-c.N // 256)
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    assert T <= 256 and 2 * T <= 2 * ncu and c.K // 64 >= 4          # the fit rule of test_gemm_stream_k
    run_case(c, dev, opts)


# ------------------------------------------------------------ GELU accuracy
GELU_ABS = 4.2e-7        # common.h: |gelu err| <= 4.2e-7 over [-12, 12]
GELU_D_ABS = 6e-7        # gelu': twice the measured worst absolute error, one significant digit
GELU_TAIL_REL = 6.3e-2   # gelu on [-12, -4]: twice the measured worst relative error


@pytest.mark.parametrize("path", ["small", "v1f"])
def test_gelu_sweep(dev, path):
    """GELU separated from the product: B is the identity, so the pre-activation is the operand itself, exactly;
    65536 points cover [-12, 12] at a spacing of 3.7e-4. Epilogue 1 stores the pre-activation (bitwise the
    operand) and C = gelu(pre) within the header's stated bound; epilogue 4 stores gelu'(pre); the negative tail
    is checked relatively (no cancellation there)."""
    M, N = 1024, 64
    x = torch.linspace(-12.0, 12.0, M * N, dtype=F64).to(F32).view(M, N)
    xd, eye = x.to(dev), torch.eye(N, device=dev)
    x64 = x.double()
    g64 = G.gelu64(x64)
    d64 = G.gelu_grad(x64)
    part = torch.empty((K.gemm_colsum_rows(M), N), device=dev) if path == "v1f" else None   # column sums: v1
    c = G.Case(path, M, N, N, colsum=part is not None)
    assert G.predict(c) == path
    for epi in (1, 4):
        C = torch.full((M, N), math.nan, device=dev)
        aux = torch.full((M, N), math.nan, device=dev)
        K.gemm(xd, eye, C, M, N, N, N, N, N, epilogue=epi, aux_out=aux, ldaux=N, colsum=part)
        err = (C.double().cpu() - g64).abs()
        tail = x64 <= -4.0
        rel = (err[tail] / g64[tail].abs()).max().item()
        print(f"[gelu] {path} epi{epi} abs {err.max().item():.3e} tail-rel {rel:.3e}")
        assert err.max().item() <= GELU_ABS
        assert rel <= GELU_TAIL_REL
        if epi == 1:
            assert same_bits(aux, x)
        else:
            derr = (aux.double().cpu() - d64).abs().max().item()
            print(f"[gelu] {path} epi4 gelu' abs {derr:.3e}")
            assert derr <= GELU_D_ABS


# ------------------------------------------------------- weight gradients
def _padded(rows, cols, seed, dtype, dev, scale=1.0):
    """[rows, cols] view of a NaN-padded [rows + 2, cols + 8] tensor"""
    big = torch.full((rows + 2, cols + 8), math.nan, dtype=dtype)
    big[1:-1, :cols] = G._randn((rows, cols), seed, dtype, scale)
    return big.to(dev)[1:-1, :cols], big[1:-1, :cols]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("tokens", [64, 200, 1032, 2056])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
def test_linear_wgrad_beta(dev, dtype, tokens, strided):
    """linear_wgrad(beta = 1) into a pre-filled out: dense (the wrapper's split path where
    maeclip_gemm_splitk > 1: 2056 tokens) and a strided out (S = 1)"""
    N, Kd = 40, 24
    dy, dy_c = _padded(tokens, N, 1, dtype, dev)
    x, x_c = _padded(tokens, Kd, 2, dtype, dev, 0.25)
    S = int(L.lib().maeclip_gemm_splitk(N, Kd, tokens))
    assert (S > 1) == (tokens == 2056)
    wide = torch.full((N + 2, Kd + 4), G.SENTINEL)
    w0 = G._randn((N, Kd), 3, F32)
    if strided:
        wide[1:-1, :Kd] = w0
        wd = wide.to(dev)
        out = wd[1:-1, :Kd]
    else:
        out = w0.to(dev)
    K.linear_wgrad(dy, x, out=out, beta=1.0)
    ref64 = dy_c.double().t() @ x_c.double() + w0.double()
    ref32 = dy_c.float().t() @ x_c.float() + w0
    check(f"linear_wgrad T{tokens} S{S}", out, ref64, ref32)
    if strided:
        got = wd.cpu()
        got[1:-1, :Kd] = G.SENTINEL
        assert same_bits(got, torch.full_like(got, G.SENTINEL))


def _grouped(dev, M, shapes, dtype, beta):
    """problems (N, K) sharing M tokens: every dy / x is a view of its own NaN-padded tensor (ldy = N + 8,
    ldx = K + 8), every dW sits in its own sentinel-guarded allocation"""
    items, refs = [], []
    for i, (n, k) in enumerate(shapes):
        dy, dy_c = _padded(M, n, 2 * i + 5, dtype, dev)
        x, x_c = _padded(M, k, 2 * i + 6, dtype, dev, 0.25)
        w0 = G._randn((n, k), 300 + i, F32)
        buf = G.Buf(F32, torch.arange(n * k), n * k, G.SENTINEL, w0 if beta else torch.full((n * k,), math.nan),
                    band=2 * k).to(dev)
        out = buf.dev[buf.lead:buf.lead + n * k].view(n, k)
        items.append((dy, x, out))
        refs.append((buf, dy_c, x_c, w0))
    K.wgrad_grouped(items, beta=beta)
    torch.cuda.synchronize()
    worst = 0.0
    for i, (buf, dy_c, x_c, w0) in enumerate(refs):
        n, k = shapes[i]
        vals = _intact(f"wgrad_grouped p{i}", buf).view(n, k)
        r64 = dy_c.double().t() @ x_c.double() + (beta * w0.double() if beta else 0.0)
        r32 = dy_c.float().t() @ x_c.float() + (beta * w0 if beta else 0.0)
        worst = max(worst, check(f"wgrad_grouped M{M} p{i}/{len(shapes)} beta{beta}", vals, r64, r32)[2])
    return worst


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("nprob", [1, 2, 48, 49])
@pytest.mark.parametrize("M", [64, 192])
def test_wgrad_grouped_reference(dev, M, nprob, beta):
    """the persistent grouped launch: 48 problems per launch (49 = a second launch of one), problems of
    256 x 256 and one of 264 x 256"""
    shapes = [(256, 256)] * nprob
    shapes[-1] = (264, 256)
    _grouped(dev, M, shapes, BF16, beta)


@pytest.mark.parametrize("case", ["fp32", "ragged_tokens"])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_wgrad_grouped_fallback(dev, case, beta):
    """problems outside the grouped kernel run one maeclip_gemm each: fp32, and M % 64 != 0"""
    if case == "fp32":
        _grouped(dev, 64, [(256, 256), (264, 256)], F32, beta)
    else:
        _grouped(dev, 72, [(256, 256), (264, 256)], BF16, beta)
