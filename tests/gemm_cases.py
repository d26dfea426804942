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
