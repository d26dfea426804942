"""Case table and CPU half of the GEMM reference tests
(test_gemm_reference_gpu.py runs the cases on the GPU, test_gemm_cases_cpu.py
checks the table itself without one).

A case is one maeclip_gemm launch. build(case) makes, on the CPU and from
seeded randn already rounded to the dtype the kernel receives,
  - every operand in its layout's storage with ld = contiguous extent + the
    minimum legal excess (8 bf16 / 4 fp32 elements), inside a larger
    allocation whose pad columns and the bands before and after are NaN;
  - every output (C, aux_out, the column-sum partials, the workspace) in an
    allocation filled with a non-NaN sentinel outside the addressed region; C
    is seeded when beta != 0 and NaN when beta == 0 (a kernel that reads it
    when it must not shows);
  - the fp64 torch statement of the header's formula, alpha A B (+bias), the
    epilogue, (+beta C), and the same statement in fp32 torch (E32).
predict(case) restates the dispatcher (gemm.hip maeclip_gemm, gemm_small_ok,
gemm_v4_ok): the path a case is meant to exercise."""
import dataclasses
import math

import torch
import torch.nn.functional as F

from tests.helpers import f32

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
KC, RC = 0, 1
LAYOUTS = [(KC, KC), (KC, RC), (RC, KC), (RC, RC)]
SENTINEL = -1234.5


@dataclasses.dataclass
class Case:
    path: str                 # small / v1f / v1b / v2 / v4: the kernel the case is meant for
    M: int
    N: int
    K: int
    la: int = KC
    lb: int = KC
    dt: torch.dtype = F32     # operands (and aux)
    out: torch.dtype = F32
    alpha: float = 1.0
    beta: float = 0.0
    bias: bool = False
    epi: int = 0
    aux_out: bool = True      # epilogues 1 / 4
    resid: bool = False       # epilogues 3 / 5 (2 always has it)
    colsum: bool = False
    batch: int = 1
    strides: str = "own"      # own: distinct, larger than dense; a0 / b0: strideA / strideB = 0
    S: int = 1                # caller's split-K
    plan_ws: bool = False     # offer the maeclip_gemm_workspace bytes (gemm_small K split, v4 split plan)
    ld_eq: bool = False       # ldaux = ldr = ldc (batched epilogues)
    opts: tuple = ()          # plan options, ((name, value), ...)
    bscale: float = 0.25
    seed: int = 0
    tag: str = ""

    @property
    def id(self):
        o = "".join(f"-{k}{v}" for k, v in self.opts)
        lay = "KR"[self.la] + "KR"[self.lb]
        return (f"{self.path}-{self.M}x{self.N}x{self.K}-{lay}-{'bf' if self.out == BF16 else 'f32'}"
                f"{o}{'-' + self.tag if self.tag else ''}")

    @property
    def epc(self):
        return 8 if self.dt == BF16 else 4


def legal(c):
    """the nearest legal sizes: a row-contiguous operand needs its row extent to be a multiple of 8 (bf16) / 4
    (fp32); N is always a multiple of 4"""
    e = c.epc
    near = lambda v, q: max(q, int(round(v / q)) * q)
    M = near(c.M, e) if c.la == RC else c.M
    N = near(c.N, e) if c.lb == RC else near(c.N, 4)
    return dataclasses.replace(c, M=M, N=N)


def geometry(c):
    """leading dimensions and batch strides (elements)"""
    e = c.epc
    lda = (c.K if c.la == KC else c.M) + e
    ldb = (c.K if c.lb == KC else c.N) + e
    if c.S > 1:
        ldc = c.N                                        # split-K: dense output
    else:
        ldc = c.N + (8 if (c.out == BF16 and c.path == "v4") else 4)
    ldaux = ldc if c.ld_eq else c.N + 8
    ldr = ldc if c.ld_eq else c.N + 12
    rows_a = c.M if c.la == KC else c.K
    rows_b = c.N if c.lb == KC else c.K
    sA = 0 if (c.strides == "a0" or c.batch == 1) else rows_a * lda + 16
    sB = 0 if (c.strides == "b0" or c.batch == 1) else rows_b * ldb + 24
    sC = 0 if c.batch == 1 else (c.M * max(ldc, ldaux, ldr) + 7) // 8 * 8 + 8
    return dict(lda=lda, ldb=ldb, ldc=ldc, ldaux=ldaux, ldr=ldr, sA=sA, sB=sB, sC=sC, rows_a=rows_a, rows_b=rows_b)


def predict(c):
    """the dispatcher restated: gemm_small_ok, gemm_v4_ok, the v2 line, else v1 (operands of the harness are
    16-byte aligned, which v4 also asks of C, aux, resid, bias and the split-K workspace). This is the test's
    own reading of gemm.hip compared with the case's own label: it keeps the table honest about which kernel
    a case is written for. The library's own answer, maeclip_gemm_impl (maeclip::gemm_route, the function
    maeclip_gemm routes by), is checked against the same labels in test_gemm_cases_cpu.py, so a dispatcher
    change that moves a case shows there; this restatement stays independent of it."""
    g = geometry(c)
    if c.dt == F32:
        small = c.out == F32 and c.S <= 1 and not c.colsum and c.M * c.N <= 256 * 1024 and c.K <= 8192
        return "small" if small else "v1f"
    k64 = c.K % 64 == 0 and c.K > 0 and g["lda"] % 8 == 0 and g["ldb"] % 8 == 0
    v4 = k64 and c.M >= 256 and c.N >= 256 and c.N % 8 == 0
    if v4 and c.S <= 1:
        v4 = g["ldc"] % (8 if c.out == BF16 else 4) == 0
        if c.epi in (1, 3, 4, 5) and (c.epi in (3, 5) or c.aux_out):
            v4 = v4 and g["ldaux"] % 8 == 0
        if c.epi == 2 or c.resid:
            v4 = v4 and g["ldr"] % 4 == 0
    if v4:
        return "v4"
    if k64 and (c.la == KC or c.M >= 8) and (c.lb == KC or c.N >= 8):
        return "v2"
    return "v1b"


def gemm_args(c, ptr=lambda name: 4096):
    """the ABI struct of a case; ptr(name) -> address of A, B, C, bias, aux, aux_out, resid, colsum, ws (the
    default, one aligned dummy address, serves the host-side queries)"""
    from mae_clip_amd import _lib as L
    g = geometry(c)
    has = lambda name, on: ptr(name) if on else None
    return L.GemmArgs(A=ptr("A"), B=ptr("B"), C=ptr("C"), M=c.M, N=c.N, K=c.K, lda=g["lda"], ldb=g["ldb"], ldc=g["ldc"],
                      batch=c.batch, strideA=g["sA"], strideB=g["sB"], strideC=g["sC"],
                      dtype=L.BF16 if c.dt == BF16 else L.F32, out_dtype=L.BF16 if c.out == BF16 else L.F32,
                      a_layout=c.la, b_layout=c.lb, epilogue=c.epi, alpha=c.alpha, beta=c.beta,
                      bias=has("bias", c.bias), aux=has("aux", c.epi in (3, 5)),
                      aux_out=has("aux_out", c.epi in (1, 4) and c.aux_out), ldaux=g["ldaux"],
                      resid=has("resid", c.epi == 2 or c.resid), ldr=g["ldr"], colsum_partial=has("colsum", c.colsum),
                      splitk=c.S, workspace=has("ws", c.S > 1 or c.plan_ws))


def plan_workspace(c):
    """maeclip_gemm_workspace of the case under the current options, a workspace being offered"""
    import ctypes
    from mae_clip_amd import _lib as L
    a = gemm_args(dataclasses.replace(c, plan_ws=True))
    return int(L.lib().maeclip_gemm_workspace(ctypes.byref(a)))


# ------------------------------------------------------------------ buffers
class Buf:
    """a flat allocation: `guard` everywhere, `inside` at base + idx"""

    def __init__(self, dtype, idx, span, guard, inside=None, band=0):
        self.idx = idx
        self.lead = (band + 7) // 8 * 8 + 64
        total = self.lead + span + self.lead
        self.flat = torch.full((total,), guard, dtype=dtype)
        if inside is not None:
            self.flat[self.lead + idx.reshape(-1)] = inside.reshape(-1).to(dtype)
        self.orig = self.flat.clone()
        self.dev = None

    def to(self, dev):
        self.dev = self.flat.to(dev)
        return self

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.lead * self.dev.element_size()

    def read(self):
        """(the addressed values, everything else, everything else as it was)"""
        got = self.dev.cpu()
        keep = torch.ones(got.numel(), dtype=torch.bool)
        keep[self.lead + self.idx.reshape(-1)] = False
        return got[self.lead + self.idx.reshape(-1)].reshape(self.idx.shape), got[keep], self.orig[keep]


def _idx(batch, stride, rows, cols, ld, transposed=False):
    """[batch, rows, cols] element offsets of a row-major [rows][ld] image (transposed: stored [cols][ld])"""
    z = torch.arange(batch).view(-1, 1, 1) * stride
    r = torch.arange(rows).view(1, -1, 1)
    c = torch.arange(cols).view(1, 1, -1)
    return z + (c * ld + r if transposed else r * ld + c)


def _randn(shape, seed, dtype, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _cdf(x):
    """Phi(x) = erfc(-x / sqrt 2) / 2: no cancellation in the negative tail"""
    return 0.5 * torch.special.erfc(x * (-1.0 / math.sqrt(2.0)))


def gelu64(x):
    """erf-GELU x Phi(x) with a tail that keeps its relative accuracy (F.gelu's 1 + erf cancels there)"""
    return x * _cdf(x)


def gelu_grad(x):
    """erf-GELU derivative, in x's precision: Phi(x) + x phi(x)"""
    return _cdf(x) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


def statement(c, dt, A, B, bias, aux, resid, C0):
    """the header's formula in precision dt: dict of C, aux_out (epilogues 1, 4), colsum"""
    al, be = f32(c.alpha), f32(c.beta)
    v = al * torch.matmul(A.to(dt), B.to(dt))
    if bias is not None:
        v = v + bias.to(dt)
    r = {}
    if c.epi == 1:
        r["aux_out"] = v
        v = F.gelu(v)
    elif c.epi == 2:
        v = v + resid.to(dt)
    elif c.epi == 3:
        v = v * gelu_grad(aux.to(dt))
        if resid is not None:
            v = v + resid.to(dt)
    elif c.epi == 4:
        r["aux_out"] = gelu_grad(v)
        v = F.gelu(v)
    elif c.epi == 5:
        v = v * aux.to(dt)
        if resid is not None:
            v = v + resid.to(dt)
    if c.beta != 0.0:
        v = v + be * C0.to(dt)
    r["C"] = v
    r["colsum"] = v.sum(1)        # [batch, N]
    return r


def build(c):
    """CPU half of a case: buffers, fp64 reference and fp32 run"""
    g = geometry(c)
    M, N, K, nb = c.M, c.N, c.K, c.batch
    sd = 1000 * c.seed + 17
    na = 1 if (c.strides == "a0") else nb
    nbb = 1 if (c.strides == "b0") else nb
    A = _randn((na, M, K), sd + 1, c.dt)                       # logical A[z][m][k]
    B = _randn((nbb, K, N), sd + 2, c.dt, c.bscale)            # logical B[z][k][n]
    nan = math.nan
    bufs = {}
    bufs["A"] = Buf(c.dt, _idx(na, g["sA"], M, K, g["lda"], c.la == RC), (na - 1) * g["sA"] + g["rows_a"] * g["lda"],
                    nan, A, band=64 * g["lda"] + 128)
    bufs["B"] = Buf(c.dt, _idx(nbb, g["sB"], K, N, g["ldb"], c.lb == KC), (nbb - 1) * g["sB"] + g["rows_b"] * g["ldb"],
                    nan, B, band=64 * g["ldb"] + 128)
    bias = _randn((N,), sd + 3, F32) if c.bias else None
    if bias is not None:
        bufs["bias"] = Buf(F32, torch.arange(N), N, nan, bias, band=64)
    C0 = _randn((nb, M, N), sd + 4, c.out) if c.beta != 0.0 else None
    span_c = (nb - 1) * g["sC"] + M * g["ldc"]
    bufs["C"] = Buf(c.out, _idx(nb, g["sC"], M, N, g["ldc"]), span_c, SENTINEL,
                    C0 if C0 is not None else torch.full((nb, M, N), nan), band=2 * g["ldc"])
    aux = resid = None
    if c.epi in (3, 5):
        aux = _randn((nb, M, N), sd + 5, c.dt)
        bufs["aux"] = Buf(c.dt, _idx(nb, g["sC"], M, N, g["ldaux"]), (nb - 1) * g["sC"] + M * g["ldaux"], nan, aux,
                          band=2 * g["ldaux"])
    if c.epi in (1, 4) and c.aux_out:
        bufs["aux_out"] = Buf(c.dt, _idx(nb, g["sC"], M, N, g["ldaux"]), (nb - 1) * g["sC"] + M * g["ldaux"],
                              SENTINEL, torch.full((nb, M, N), nan), band=2 * g["ldaux"])
    if c.epi == 2 or c.resid:
        resid = _randn((nb, M, N), sd + 6, F32)
        bufs["resid"] = Buf(F32, _idx(nb, g["sC"], M, N, g["ldr"]), (nb - 1) * g["sC"] + M * g["ldr"], nan, resid,
                            band=2 * g["ldr"])
    if c.colsum:
        rows = (M + 63) // 64
        bufs["colsum"] = Buf(F32, torch.arange(nb * rows * N), nb * rows * N, SENTINEL,
                             torch.full((nb * rows * N,), nan), band=4 * N)
    if c.S > 1:
        n = nb * c.S * M * N
        bufs["ws"] = Buf(F32, torch.arange(n), n, SENTINEL, torch.full((n,), nan), band=4 * N)
    ref64 = statement(c, F64, A, B, bias, aux, resid, C0)
    ref32 = statement(c, F32, A, B, bias, aux, resid, C0)
    return dict(case=c, geo=g, bufs=bufs, ref64=ref64, ref32=ref32)


# --------------------------------------------------------------------- table
def _vary(path, base, dt, out, Ms=(), Ns=(), Ks=(), layouts=LAYOUTS, **kw):
    """one factor at a time around base = (M, N, K), every layout pair"""
    M0, N0, K0 = base
    shapes = [base] + [(m, N0, K0) for m in Ms] + [(M0, n, K0) for n in Ns] + [(M0, N0, k) for k in Ks]
    out_cases = []
    for i, (m, n, k) in enumerate(shapes):
        for la, lb in layouts:
            out_cases.append(legal(Case(path, m, n, k, la, lb, dt, out, seed=i, **kw)))
    return out_cases


def _dedup(cases):
    seen, res = set(), []
    for c in cases:
        if c.id not in seen:
            seen.add(c.id)
            res.append(c)
    return res


def small_split_cases():
    """gemm_small's own K split (small_reduce_kernel) with every epilogue: the shortest K (multiple of 4) at
    which maeclip_gemm_workspace of the 96 x 64 base is > 0, found by query; 8192 if nothing smaller splits"""
    k = next((k for k in range(8, 8192, 4) if plan_workspace(Case("small", 96, 64, k)) > 0), 8192)
    cs = []
    for i, (epi, kw) in enumerate(((0, {}), (1, {}), (2, {}), (3, dict(resid=True)), (4, {}), (5, {}),
                                   (0, dict(alpha=0.5, beta=-0.5)))):
        la, lb = LAYOUTS[i % 4]
        cs.append(legal(Case("small", 96, 64, k, la, lb, epi=epi, bias=True, plan_ws=True, seed=40 + i,
                             tag=f"ksplit-epi{epi}" + ("-ab" if kw.get("alpha") else ""), **kw)))
    return cs


def shape_cases():
    cs = []
    cs += _vary("small", (96, 64, 64), F32, F32, Ms=(1, 31, 32, 33, 100), Ns=(4, 28, 32, 36), Ks=(4, 28, 32, 36, 68))
    cs += [legal(Case("small", 512, 512, 64, la, lb, tag="limit")) for la, lb in LAYOUTS]
    cs += [legal(Case("v1f", 512, 516, 64, la, lb, tag="limit")) for la, lb in LAYOUTS]
    # v1 fp32: reached by a bf16 output, and (fp32 output) by the column sums
    cs += _vary("v1f", (136, 132, 36), F32, BF16, Ms=(1, 127, 128, 129), Ns=(4, 124, 128, 132), Ks=(4, 32, 36, 100))
    cs += _vary("v1f", (136, 132, 36), F32, F32, Ks=(100,), colsum=True, tag="colsum")
    cs += _vary("v1b", (136, 136, 72), BF16, F32, Ms=(1, 120, 128, 136), Ns=(8, 120, 128, 136), Ks=(8, 56, 72, 136))
    cs += _vary("v1b", (136, 136, 72), BF16, BF16, Ks=(136,))
    cs += _vary("v2", (136, 136, 128), BF16, F32, Ms=(1, 8, 120, 128, 136, 248), Ns=(8, 120, 128, 136, 248),
                Ks=(64, 128, 320))
    cs += _vary("v2", (136, 136, 128), BF16, BF16, Ks=(320,))
    cs += [legal(Case("v2", m, n, 128, la, lb, BF16, F32, tag="v4limit")) for m, n in ((136, 256), (256, 136))
           for la, lb in LAYOUTS]
    # the K limit of gemm_small: 8192 on it, 8196 on v1 fp32 (a K that also ends inside a K-tile)
    cs += [legal(Case("small", 8, 8, 8192, la, lb, tag="klimit")) for la, lb in LAYOUTS]
    cs += [legal(Case("v1f", 8, 8, 8196, la, lb, tag="klimit")) for la, lb in LAYOUTS]
    # v4: every tile height, one factor at a time, both outputs. Auto and 256-row tiles: every layout pair.
    # 192- and 128-row tiles exist for K-contiguous A only: both B layouts there (the base also with
    # row-contiguous A, which falls back to 256 rows)
    shapes = [(264, 264, k) for k in (64, 128, 320)] + [(m, 264, 128) for m in (256, 384, 392, 520)] + \
             [(264, n, 128) for n in (256, 520)]
    for bm in (0, 256, 192, 128):
        o = (("GEMM_BM", bm),) if bm else ()
        for i, (m, n, k) in enumerate(shapes):
            base = (m, n, k) == (264, 264, 128)
            for la, lb in (LAYOUTS if (bm in (0, 256) or base) else LAYOUTS[:2]):
                for out in (F32, BF16):
                    cs.append(legal(Case("v4", m, n, k, la, lb, BF16, out, opts=o, seed=i)))
    return _dedup(cs)


REP = {   # one representative shape per path, ragged in M and N
    "small": dict(M=100, N=36, K=64, dt=F32, out=F32),
    "v1f": dict(M=136, N=132, K=36, dt=F32, out=BF16),
    "v1b": dict(M=136, N=136, K=72, dt=BF16, out=F32),
    "v2": dict(M=136, N=136, K=128, dt=BF16, out=F32),
    "v4": dict(M=264, N=264, K=128, dt=BF16, out=F32),
}


def _rep(path, i=0, **kw):
    d = dict(REP[path])
    d.update(kw)
    la, lb = d.pop("lay", LAYOUTS[i % 4])
    return legal(Case(path, la=la, lb=lb, seed=50 + i, **d))


def _outs(path):
    # gemm_small is fp32 -> fp32 by definition; v1 fp32 with an fp32 output is reached through the column sums
    return {"small": [dict(out=F32)], "v1f": [dict(out=BF16), dict(out=F32, colsum=True)]}.get(
        path, [dict(out=F32), dict(out=BF16)])


def scalar_cases():
    """alpha / beta / bias, one at a time and all together"""
    cs = []
    for path in REP:
        i = 0
        for o in _outs(path):
            for kw in (dict(alpha=0.5), dict(alpha=-1.25), dict(beta=1.0), dict(beta=-0.5), dict(bias=True),
                       dict(alpha=-1.25, beta=-0.5, bias=True)):
                t = "".join(f"{k[0]}{v}" for k, v in kw.items())
                cs.append(_rep(path, i, tag=t, **o, **kw))
                i += 1
    return cs


def epilogue_cases():
    """epilogues 1 to 5 with ldaux != ldc and ldr != ldc, aux_out / resid present and absent"""
    cs = []
    for path in REP:
        i = 0
        for o in _outs(path):
            variants = [(1, dict(aux_out=True)), (1, dict(aux_out=False)), (3, dict(resid=False)),
                        (3, dict(resid=True)), (4, dict(aux_out=True)), (4, dict(aux_out=False)),
                        (5, dict(resid=False)), (5, dict(resid=True))]
            if o["out"] == F32:
                variants.insert(2, (2, {}))
            for epi, kw in variants:
                t = f"epi{epi}" + ("" if kw.get("aux_out", True) else "-noaux") + ("-resid" if kw.get("resid") else "")
                cs.append(_rep(path, i, epi=epi, bias=(i % 2 == 0), tag=t, **o, **kw))
                i += 1
    return cs


def colsum_cases():
    """column-sum partials: M on both sides of 64 and 128 (v4: of 256 and 320), and batch = 3"""
    cs = []
    for path, Ms in (("v1f", (60, 64, 68, 124, 128, 132)), ("v1b", (56, 64, 72, 120, 128, 136)),
                     ("v2", (56, 64, 72, 120, 128, 136)), ("v4", (256, 264, 320, 328))):
        for i, m in enumerate(Ms):
            cs.append(_rep(path, i, M=m, colsum=True, bias=True, out=(F32, BF16)[i % 2], tag="colsum"))
        cs.append(_rep(path, 1, colsum=True, batch=3, tag="colsum-b3"))
    return cs


def batch_cases():
    cs = []
    for path in REP:
        col = dict(colsum=True) if path == "v1f" else {}
        for i, st in enumerate(("own", "b0", "a0")):
            cs.append(_rep(path, i, batch=3, strides=st, tag=f"b3-{st}", **col))
        out = BF16 if path in ("v1f", "v4") else F32     # v4: ldaux = ldc must be a multiple of 8
        for i, (epi, kw) in enumerate(((1, {}), (3, dict(resid=True)), (5, dict(resid=True)))):
            cs.append(_rep(path, i + 1, batch=3, epi=epi, ld_eq=True, out=out, bias=True, tag=f"b3-epi{epi}", **kw))
    return cs


def splitk_cases():
    """the caller's split-K: S in {2, 3, 5}, an empty last slice, alpha, bias, beta, bf16 output, batch 2"""
    cs = []
    shapes = {"v1f": (136, 132, 100), "v1b": (136, 136, 136), "v2": (136, 136, 128), "v4": (264, 264, 128)}
    for path, (m, n, k) in shapes.items():
        dt = F32 if path == "v1f" else BF16
        i = 0
        for S in (2, 3, 5):      # S = 3 at K = 128 (64-deep) and S = 5 at K = 100 (32-deep) leave the last slice empty
            cs.append(legal(Case(path, m, n, k, *LAYOUTS[i % 4], dt, F32, S=S, alpha=0.5, seed=70 + i, tag=f"S{S}")))
            i += 1
        for kw in (dict(bias=True), dict(beta=-0.5), dict(out=BF16), dict(batch=2),
                   dict(alpha=-1.25, bias=True, beta=1.0, out=BF16, batch=2)):
            t = "-".join(f"{a}{'' if v is True else v}" for a, v in kw.items()).replace("torch.", "")
            d = dict(out=F32)
            d.update(kw)
            cs.append(legal(Case(path, m, n, k, *LAYOUTS[i % 4], dt, S=3, seed=70 + i, tag="S3-" + t, **d)))
            i += 1
    return cs


def v4_split_cases():
    """the forced in-launch split (GEMM_SPLIT = 2 on 192-row tiles) at K = 256, the smallest K that fits it
    (>= 2 K-tiles per slice); K-contiguous A only"""
    o = (("GEMM_SPLIT", 2), ("GEMM_BM", 192))
    return [legal(Case("v4", 264, 264, 256, KC, lb, BF16, out, opts=o, plan_ws=True, seed=90 + lb, tag="split2"))
            for lb in (KC, RC) for out in (F32, BF16)]


# ---------------------------------------------------------- v4 launch plans
# Labelled by hand from the rules in mae_clip_amd/csrc/gemm4_plan.h (gemm4_plan, wgrad_plan), at 256 and at 64 CUs.
# Cost model of a plain launch, in 256-row K-tiles: rounds of the grid x (K-tiles x c + 2.5), c = 1 (256 rows),
# 0.89 (192), 0.72 (128); a split of S = 2 on 192-row tiles costs rounds x L0 x 0.89 + 2.5 + 2.
PLAN_OPTS = ("GEMM_BM", "GEMM_SK", "GEMM_SPLIT", "GEMM_SPLIT_D", "GEMM_SPLIT_MINK", "GEMM_BM128", "GEMM_GRID", "WG_SK")
LDS = {256: 163840, 192: 149504, 128: 131072}     # 2 operand stages (+ 2 KiB of fp8 scale images at 192) + 32 KiB


def sk_ws(ncu):
    """16 KiB of arrival counters + two fp32 256 x 256 partial tiles per CU"""
    return 16384 + 2 * ncu * 262144


@dataclasses.dataclass
class PlanCase:
    tag: str
    M: int
    N: int
    K: int
    want: dict                # ncu -> (bm, S, L0, (grid x, y, z), persistent)
    family: str = "bf16"      # bf16 / fp8rows / fp8blocks
    la: int = KC
    colsum: bool = False
    batch: int = 1
    S: int = 1                # caller's split-K
    ws: bool = False          # a workspace is offered
    opts: tuple = ()

    @property
    def id(self):
        return self.tag


def plan_args(c):
    from mae_clip_amd import _lib as L
    f8 = c.family != "bf16"
    return L.GemmArgs(A=4096, B=4096, C=4096, M=c.M, N=c.N, K=c.K, lda=c.K if c.la == KC else c.M, ldb=c.K, ldc=c.N,
                      batch=c.batch, strideA=c.M * c.K, strideB=c.N * c.K, strideC=c.M * c.N,
                      dtype=2 if f8 else L.BF16, out_dtype=L.F32, a_layout=c.la, b_layout=KC, epilogue=0, alpha=1.0,
                      beta=0.0, colsum_partial=4096 if c.colsum else None, splitk=c.S,
                      workspace=4096 if (c.ws or c.S > 1) else None)


def plan_cases():
    P = PlanCase
    split = (("GEMM_SPLIT", 2), ("GEMM_BM", 192))
    cs = [
        # encoder N = 768: 256 rows 50 x 3 = 150 tiles, 192 rows 67 x 3 = 201. 256 CUs: one round each, 12 + 2.5 =
        # 14.5 against 12 x 0.89 + 2.5 = 13.18 -> 192. 64 CUs: 3 rounds x 14.5 = 43.5 against 4 x 13.18 = 52.7 -> 256
        P("enc768", 12800, 768, 768, {256: (192, 0, 0, (201, 1, 1), True), 64: (256, 0, 0, (64, 1, 1), True)}),
        # 64 x 4 = 256 tiles of 256 rows: one full round (4 + 2.5 = 6.5); 192 rows: 86 x 4 = 344 tiles = 2 rounds
        # (2 x 6.06). 64 CUs: 4 rounds x 6.5 = 26 against 6 x 6.06 = 36.4
        P("full_round", 16384, 1024, 256, {256: (256, 0, 0, (256, 1, 1), True), 64: (256, 0, 0, (64, 1, 1), True)}),
        # row-contiguous A / column sums: 256 rows only
        P("rc_a", 12800, 768, 768, {256: (256, 0, 0, (150, 1, 1), True), 64: (256, 0, 0, (64, 1, 1), True)}, la=RC),
        P("colsum", 12800, 768, 768, {256: (256, 0, 0, (150, 1, 1), True), 64: (256, 0, 0, (64, 1, 1), True)},
          colsum=True),
        # caller split-K / batched: 256 rows, one block per (tile, slice, batch); 2 x 2 and 50 x 3 tiles
        P("caller_splitk", 264, 264, 128, {256: (256, 0, 0, (4, 3, 1), False), 64: (256, 0, 0, (4, 3, 1), False)}, S=3),
        P("batched", 264, 264, 128, {256: (256, 0, 0, (4, 1, 3), False), 64: (256, 0, 0, (4, 1, 3), False)}, batch=3),
        P("batched_big", 12800, 768, 768, {256: (256, 0, 0, (150, 1, 2), False), 64: (256, 0, 0, (150, 1, 2), False)},
          batch=2),
        P("splitk_batched", 264, 264, 128, {256: (256, 0, 0, (4, 4, 2), False), 64: (256, 0, 0, (4, 4, 2), False)},
          S=4, batch=2, opts=(("GEMM_BM", 192),)),
        # forced tile heights: 100 x 3 = 300, 201, 150 tiles
        P("bm128", 12800, 768, 768, {256: (128, 0, 0, (256, 1, 1), True), 64: (128, 0, 0, (64, 1, 1), True)},
          opts=(("GEMM_BM", 128),)),
        P("bm192", 12800, 768, 768, {256: (192, 0, 0, (201, 1, 1), True), 64: (192, 0, 0, (64, 1, 1), True)},
          opts=(("GEMM_BM", 192),)),
        P("bm256", 12800, 768, 768, {256: (256, 0, 0, (150, 1, 1), True), 64: (256, 0, 0, (64, 1, 1), True)},
          opts=(("GEMM_BM", 256),)),
        # a forced height the launch cannot take (row-contiguous A) falls back to 256
        P("bm192_rc_a", 12800, 768, 768, {256: (256, 0, 0, (150, 1, 1), True), 64: (256, 0, 0, (64, 1, 1), True)},
          la=RC, opts=(("GEMM_BM", 192),)),
        # forced split of 2 on 192-row tiles, 2 x 2 tiles, K = 256: NT = 4 = 2 S fits; the whole grid launches.
        # lead 4: L0 = ceil((4 + 4) / 2) = 4, capped at NT - 1 = 3; lead 0: L0 = 2
        P("split2_k256", 264, 264, 256, {256: (192, 2, 3, (256, 1, 1), True), 64: (192, 2, 3, (64, 1, 1), True)},
          ws=True, opts=split),
        P("split2_k256_lead0", 264, 264, 256, {256: (192, 2, 2, (256, 1, 1), True), 64: (192, 2, 2, (64, 1, 1), True)},
          ws=True, opts=split + (("GEMM_SPLIT_D", 0),)),
        # K = 1024, NT = 16: lead 4 -> ceil(20 / 2) = 10, lead 9 -> ceil(25 / 2) = 13
        P("split2_k1024", 264, 264, 1024, {256: (192, 2, 10, (256, 1, 1), True), 64: (192, 2, 10, (64, 1, 1), True)},
          ws=True, opts=split),
        P("split2_k1024_lead9", 264, 264, 1024, {256: (192, 2, 13, (256, 1, 1), True), 64: (192, 2, 13, (64, 1, 1), True)},
          ws=True, opts=split + (("GEMM_SPLIT_D", 9),)),
        # K = 192: NT = 3 < 2 S does not fit -> the best data-parallel plan (192 rows forced, 4 tiles)
        P("split2_k192", 264, 264, 192, {256: (192, 0, 0, (4, 1, 1), True), 64: (192, 0, 0, (4, 1, 1), True)},
          ws=True, opts=split),
        # no workspace offered: no split
        P("split2_no_ws", 264, 264, 256, {256: (192, 0, 0, (4, 1, 1), True), 64: (192, 0, 0, (4, 1, 1), True)},
          opts=split),
        # the cost model's split (GEMM_SK = 1): 6400 x 768 x 3072, NT = 48; 256 rows 75 tiles (50.5), 192 rows 102
        # tiles (48 x 0.89 + 2.5 = 45.2); split of the 102: 204 units = one round of 256, L0 = ceil(52 / 2) = 26:
        # 26 x 0.89 + 4.5 = 27.6 -> taken. 64 CUs: 204 units > 2 x 64 -> none; 2 rounds x 45.2 against 2 x 50.5 -> 192
        P("sk_ws", 6400, 768, 3072, {256: (192, 2, 26, (256, 1, 1), True), 64: (192, 0, 0, (64, 1, 1), True)},
          ws=True, opts=(("GEMM_SK", 1),)),
        P("sk_no_ws", 6400, 768, 3072, {256: (192, 0, 0, (102, 1, 1), True), 64: (192, 0, 0, (64, 1, 1), True)},
          opts=(("GEMM_SK", 1),)),
        # without GEMM_SK a workspace changes nothing
        P("ws_default", 6400, 768, 3072, {256: (192, 0, 0, (102, 1, 1), True), 64: (192, 0, 0, (64, 1, 1), True)},
          ws=True),
        # fp8 rows, K-tile 128: 9280 x 1024 x 512 is NT = 4; 256 rows 37 x 4 = 148 tiles (6.5), 192 rows 49 x 4 = 196
        # (4 x 0.89 + 2.5 = 6.06) -> 192; 64 CUs: 3 x 6.5 against 4 x 6.06 -> 256
        P("fp8_rows", 9280, 1024, 512, {256: (192, 0, 0, (196, 1, 1), True), 64: (256, 0, 0, (64, 1, 1), True)},
          family="fp8rows"),
        # the forced split needs 4 K-tiles of 128: not at K = 256 (bf16 fits there), at K = 512 with L0 = 3
        P("fp8_rows_split_k256", 264, 264, 256, {256: (192, 0, 0, (4, 1, 1), True), 64: (192, 0, 0, (4, 1, 1), True)},
          family="fp8rows", ws=True, opts=split),
        P("fp8_rows_split_k512", 264, 264, 512, {256: (192, 2, 3, (256, 1, 1), True), 64: (192, 2, 3, (64, 1, 1), True)},
          family="fp8rows", ws=True, opts=split),
        # a forced 128 rules 192 out, and 128-row tiles are bf16 only: fp8 is left with 256 rows (148 tiles)
        P("fp8_rows_bm128", 9280, 1024, 512, {256: (256, 0, 0, (148, 1, 1), True), 64: (256, 0, 0, (64, 1, 1), True)},
          family="fp8rows", opts=(("GEMM_BM", 128),)),
        P("fp8_rows_batched", 264, 264, 512, {256: (256, 0, 0, (4, 1, 2), False), 64: (256, 0, 0, (4, 1, 2), False)},
          family="fp8rows", batch=2),
        # fp8 blocks: always 192 rows, never a split
        P("fp8_blocks", 9280, 1024, 512, {256: (192, 0, 0, (196, 1, 1), True), 64: (192, 0, 0, (64, 1, 1), True)},
          family="fp8blocks"),
        P("fp8_blocks_forced", 264, 264, 512, {256: (192, 0, 0, (4, 1, 1), True), 64: (192, 0, 0, (4, 1, 1), True)},
          family="fp8blocks", ws=True, opts=(("GEMM_SPLIT", 2), ("GEMM_BM", 256), ("GEMM_SK", 1))),
    ]
    return cs


@dataclasses.dataclass
class WgradCase:
    tag: str
    shapes: list              # (N, K) of every problem
    M: int
    want: dict                # ncu -> dict of the plan fields that are checked
    opts: tuple = ()

    @property
    def id(self):
        return self.tag


ENC_LAYER = [(2304, 768), (768, 768), (3072, 768), (768, 3072)]     # 27 + 9 + 36 + 36 = 108 tiles of 256 x 256
DEC_LAYER = [(1536, 512), (512, 512), (2048, 512), (512, 2048)]     # 12 + 4 + 16 + 16 = 48 tiles


def wgrad_problems(shapes):
    from mae_clip_amd import _lib as L
    probs = (L.WgradProblem * len(shapes))()
    for q, (N, K) in zip(probs, shapes):
        q.dy, q.x, q.dw, q.N, q.K, q.ldy, q.ldx = 4096, 4096, 4096, N, K, N, K
    return probs


def wgrad_plan_cases():
    W = WgradCase
    sk = lambda ncu: 2 * ncu * 262144          # two fp32 256 x 256 slots per block
    dec_nk = 8 * sum(n * k for n, k in DEC_LAYER)
    return [
        # encoder: 12 x 108 = 1296 tiles, NT = 12800 / 64 = 200. 256 CUs: remainder 1296 % 256 = 16 tiles,
        # skw = ceil(16 x 200 / 256) = 13 >= 8, Tdp = 1280. 64 CUs: 1296 % 64 = 16, skw = ceil(3200 / 64) = 50
        W("encoder48", ENC_LAYER * 12, 12800,
          {256: dict(mode="streamk", T=1296, S=1, skw=13, Tdp=1280, NT=200, grid=256, reduce=2, reduce_grid=(16, 16),
                     workspace_bytes=sk(256)),
           64: dict(mode="streamk", T=1296, S=1, skw=50, Tdp=1280, NT=200, grid=64, reduce=2, reduce_grid=(16, 16),
                    workspace_bytes=sk(64))}),
        # decoder: 8 x 48 = 384 tiles, NT = 50432 / 64 = 788. 256 CUs: remainder 128 tiles, skw = ceil(128 x 788 /
        # 256) = 394, Tdp = 256. 64 CUs: 384 = 6 rounds, no remainder; slices: S = 2, 3, 4 all keep 6 rounds per
        # tile-K (12 / 2, 18 / 3, 24 / 4), none beats 6 by 15 % -> whole tiles
        W("decoder32", DEC_LAYER * 8, 50432,
          {256: dict(mode="streamk", T=384, S=1, skw=394, Tdp=256, NT=788, grid=256, reduce=2, reduce_grid=(128, 16),
                     workspace_bytes=sk(256)),
           64: dict(mode="whole", T=384, S=1, skw=0, Tdp=0, NT=0, grid=64, reduce=0, workspace_bytes=0)}),
        # WG_SK = 0, decoder. 256 CUs: S = 1 costs ceil(384 / 256) = 2 rounds; S = 2: ceil(768 / 256) / 2 = 1.5 <
        # 0.85 x 2; S = 3: 5 / 3 and S = 4: 6 / 4 do not beat 1.5 -> S = 2: two fp32 slabs of every dW; the reduce
        # covers the largest dW (2048 x 512 / 4 / 256 = 1024 blocks) x 32 problems
        W("decoder32_uniform", DEC_LAYER * 8, 50432,
          {256: dict(mode="split", T=384, S=2, skw=0, grid=256, reduce=1, reduce_grid=(1024, 32),
                     workspace_bytes=2 * dec_nk * 4),
           64: dict(mode="whole", T=384, S=1, skw=0, grid=64, reduce=0, workspace_bytes=0)}, opts=(("WG_SK", 0),)),
        # WG_SK = 0, encoder: 6 rounds; S = 2: 11 / 2, S = 3: 16 / 3, S = 4: 21 / 4 are all above 0.85 x 6 = 5.1.
        # 64 CUs: 21 rounds; 41 / 2, 61 / 3, 81 / 4 are all above 17.85
        W("encoder48_uniform", ENC_LAYER * 12, 12800,
          {256: dict(mode="whole", T=1296, S=1, skw=0, grid=256, reduce=0, workspace_bytes=0),
           64: dict(mode="whole", T=1296, S=1, skw=0, grid=64, reduce=0, workspace_bytes=0)}, opts=(("WG_SK", 0),)),
        # 16 x 16 = 256 tiles: a multiple of both grids, no remainder; slices never cut the rounds per tile-K
        W("full_rounds", [(4096, 4096)], 4096,
          {256: dict(mode="whole", T=256, S=1, skw=0, Tdp=0, grid=256, reduce=0, workspace_bytes=0),
           64: dict(mode="whole", T=256, S=1, skw=0, Tdp=0, grid=64, reduce=0, workspace_bytes=0)}),
        # 4 tiles, NT = 64: skw = ceil(4 x 64 / 256) = 1 < 8 -> no stream-K; S = 4 (16 K-tiles each) cuts the one
        # round to 1 / 4. 64 CUs: skw = ceil(256 / 64) = 4 < 8, the same
        W("few_tiles", [(512, 256), (256, 512)], 4096,
          {256: dict(mode="split", T=4, S=4, skw=0, grid=16, reduce=1, reduce_grid=(128, 2),
                     workspace_bytes=4 * 2 * 512 * 256 * 4),
           64: dict(mode="split", T=4, S=4, skw=0, grid=16, reduce=1, reduce_grid=(128, 2),
                    workspace_bytes=4 * 2 * 512 * 256 * 4)}),
        # 52 problems: the plan is the first chunk's, the encoder's 48
        W("longer_than_a_chunk", ENC_LAYER * 13, 12800,
          {256: dict(mode="streamk", T=1296, S=1, skw=13, Tdp=1280, grid=256, reduce_grid=(16, 16)),
           64: dict(mode="streamk", T=1296, S=1, skw=50, Tdp=1280, grid=64, reduce_grid=(16, 16))}),
    ]
