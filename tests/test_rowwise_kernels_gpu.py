"""Kernel-level reference tests of the row-wise and multi-tensor kernels that run
in every step: LayerNorm forward / backward (every NC = ceil(D / 256)
instantiation, both sides of the 256 boundaries, bf16 inputs, the fused pool
backward, the row loop past the grid cap, strides), the fused AdamW step and
the fp32 -> bf16 weight cast (entry search across chunk boundaries, vector and
element paths, misaligned entries), the batched column reductions, the pooled
mean and the token gathers.

Every reference is plain torch in fp64 on the CPU from the same seeded inputs
(already rounded to the dtype the kernel is handed). Tolerances are not
constants: the same operation is also run with ordinary fp32 torch ops on the
CPU, its per-tensor max error against fp64 is E32, and the kernel passes when
its own max error is <= 4 * E32 (a different but equally valid fp32 summation
order, the hardware rsqrt / pow). A bf16 output may add the half-ulp of the
bf16 grid at the reference value; where an output is specified as a copy of a
stored value, or as a single fp32 operation, the comparison is bitwise.
Each check prints "[ratio] name kernel-error E32 ratio" (pytest -s); the
measured maxima are tabulated in DESIGN.md section 4."""
import math

import pytest
import torch
import torch.nn.functional as F

from mae_clip_amd import kernels as K
from tests.helpers import FACTOR, _bf16_half_ulp, check, f32, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
LN_D = [4, 60, 256, 260, 512, 768, 1024, 1028, 1280, 1536, 1792, 2048]
LN_D_ALL_TYPES = (260, 768, 1024)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, dtype=F32, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=_gen(seed)) * scale + shift).to(dtype)


def _types(D):
    if D in LN_D_ALL_TYPES:
        return [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)]
    return [(F32, F32), (BF16, BF16)]


_LN_CASES = [pytest.param(D, a, b, id=f"D{D}-{str(a)[6:]}-{str(b)[6:]}") for D in LN_D for a, b in _types(D)]


# ------------------------------------------------------------ LayerNorm forward
def _ln_inputs(kind, M, D, xdt, seed):
    if kind == "randn":      # the existing test's distribution
        x = _randn((M, D), seed, xdt, 3.0, 1.0)
        res = _randn((M, D), seed + 1)
    else:                    # hard: mean 100, std 0.5 (x - mean cancels 8 bits)
        x = _randn((M, D), seed, xdt, 0.4, 100.0)
        res = _randn((M, D), seed + 1, F32, 0.3)
    return x, res, _randn((D,), seed + 2), _randn((D,), seed + 3)


def _ln_fwd_refs(x, res, g, b, eps):
    """fp64 reference and the fp32 torch run of y, mean, rstd, xsum (eps: the fp32 value)"""
    D = x.shape[1]
    out = []
    for dt in (torch.float64, F32):
        xs = x.to(dt) if res is None else x.to(dt) + res.to(dt)
        y = F.layer_norm(xs, (D,), g.to(dt), b.to(dt), eps)
        mean = xs.mean(-1)
        rstd = (xs.var(-1, unbiased=False) + eps).rsqrt()
        out.append(dict(y=y, mean=mean, rstd=rstd, xsum=xs))
    return out


def _check_ln_fwd(tag, dev, x, res, g, b, eps, ydt, xd=None, resd=None):
    xd = x.to(dev) if xd is None else xd
    resd = (res.to(dev) if res is not None else None) if resd is None else resd
    y, mean, rstd, y2, xs = K.ln_fwd(xd, g.to(dev), b.to(dev), eps, out_dtype=ydt, res=resd, y2=True, xsum=True)
    r64, r32 = _ln_fwd_refs(x, res, g, b, f32(eps))
    assert y.dtype == ydt and y2.dtype == BF16 and xs.dtype == F32
    check(f"ln_fwd.y {tag}", y, r64["y"], r32["y"])
    check(f"ln_fwd.mean {tag}", mean, r64["mean"], r32["mean"])
    check(f"ln_fwd.rstd {tag}", rstd, r64["rstd"], r32["rstd"])
    check(f"ln_fwd.xsum {tag}", xs, r64["xsum"], r32["xsum"])
    # y2 is a copy of the stored y
    assert same_bits(y2, y.to(BF16)), f"ln_fwd.y2 {tag}"


@pytest.mark.parametrize("D,xdt,ydt", _LN_CASES)
def test_ln_fwd(dev, D, xdt, ydt):
    M = 7   # a ragged last workgroup (4 rows each)
    for kind in ("randn", "hard"):
        x, res, g, b = _ln_inputs(kind, M, D, xdt, 100 + D)
        for eps in (1e-6, 1e-12):
            _check_ln_fwd(f"D{D} {kind} eps{eps:g}", dev, x, res, g, b, eps, ydt)


@pytest.mark.parametrize("D", [260, 1028])
@pytest.mark.parametrize("xdt", [F32, BF16])
def test_ln_fwd_constant_rows_exact(dev, D, xdt):
    """rows of all 2.0 and of zeros: the fp32 sum and mean are exact, every
    deviation is 0, so y == beta bitwise, mean == the constant and rstd ==
    eps^-1/2. A padded lane (D is no multiple of 256) that leaks into the
    variance adds (0 - 2)^2 and fails this."""
    eps = 1e-6
    x = torch.zeros((5, D))
    x[0::2] = 2.0
    g, b = _randn((D,), 7), _randn((D,), 8)
    want_mean = x[:, 0].clone()
    want_rstd = f32(eps) ** -0.5
    # torch's own fp32 layer_norm meets the same conditions on these rows
    assert same_bits(F.layer_norm(x, (D,), g, b, eps), b.expand(5, D))
    assert torch.equal(x.mean(-1), want_mean)
    assert ((x.var(-1, unbiased=False) + eps).rsqrt().double() - want_rstd).abs().max().item() <= 2.0 ** -23 * want_rstd
    y, mean, rstd, _, _ = K.ln_fwd(x.to(xdt).to(dev), g.to(dev), b.to(dev), eps, out_dtype=F32)
    assert same_bits(y, b.expand(5, D))
    assert torch.equal(mean.cpu(), want_mean)
    assert (rstd.cpu().double() - want_rstd).abs().max().item() <= 2.0 ** -23 * want_rstd, rstd


@pytest.mark.parametrize("xdt", [F32, BF16])
def test_ln_fwd_strided(dev, xdt):
    """x and res as column slices of wider tensors (ldx, ldres > D, multiples of 4)"""
    M, D = 5, 260
    wx = _randn((M, D + 12), 31, xdt, 3.0, 1.0)
    wr = _randn((M, D + 20), 32)
    wxd, wrd = wx.to(dev), wr.to(dev)
    g, b = _randn((D,), 33), _randn((D,), 34)
    _check_ln_fwd("strided", dev, wx[:, 4:4 + D], wr[:, 8:8 + D], g, b, 1e-6, F32, xd=wxd[:, 4:4 + D],
                  resd=wrd[:, 8:8 + D])
    assert same_bits(wxd, wx) and same_bits(wrd, wr)


# ----------------------------------------------------------- LayerNorm backward
def _pool_grad(dp, pool_n):
    """avg-pool backward of dp [B, D] (dtype of dp): row r gets dp[r // n] / (n - 1), the cls row 0"""
    Bp, D = dp.shape
    r = dp / torch.full_like(dp, pool_n - 1)
    r = r[:, None, :].expand(Bp, pool_n, D).clone()
    r[:, 0] = 0
    return r.reshape(Bp * pool_n, D)


def _ln_bwd_refs(x, dy, g, eps, mean, rstd, dres=None, dres_pool=None, pool_n=0):
    """fp64 reference: autograd of layer_norm. fp32 run: the same operation from
    the kernel's own inputs, i.e. the backward formula on the saved fp32 mean /
    rstd. (fp32 autograd from x alone recomputes the statistics and does not see
    their rounding, which dominates the error at small D: at D = 4 its dgamma
    error came out at 8.4e-8 where the kernel and this formula have 3.9e-7 and
    2.7e-7.)"""
    D = x.shape[1]
    xx = x.double().clone().requires_grad_(True)
    gg = g.double().clone().requires_grad_(True)
    bb = torch.zeros(D, dtype=torch.float64, requires_grad=True)
    (F.layer_norm(xx, (D,), gg, bb, eps) * dy.double()).sum().backward()
    xh = (x.float() - mean[:, None]) * rstd[:, None]
    gdy = dy.float() * g
    dx32 = rstd[:, None] * (gdy - gdy.mean(-1, keepdim=True) - xh * (gdy * xh).mean(-1, keepdim=True))
    out = []
    for dt, dx, dgamma, dbeta in ((torch.float64, xx.grad, gg.grad, bb.grad),
                                  (F32, dx32, (dy.float() * xh).sum(0), dy.float().sum(0))):
        if dres is not None:
            dx = dx + dres.to(dt)
        if dres_pool is not None:
            dx = dx + _pool_grad(dres_pool.to(dt), pool_n)
        out.append(dict(dx=dx, dgamma=dgamma, dbeta=dbeta, colsum=dx.sum(0)))
    return out


def _stats32(x, eps):
    """the saved statistics the backward is handed: fp64 values rounded to fp32"""
    xs = x.double()
    return xs.mean(-1).float(), (xs.var(-1, unbiased=False) + eps).rsqrt().float()


def _expected_partial_rows(M, D):
    return min((M + 3) // 4, 1024 if D <= 512 else 512)   # include/maeclip.h, maeclip_ln_bwd


def _check_ln_bwd(tag, dev, x, dy, g, eps=1e-6, dres=None, dres_pool=None, pool_n=0, full=True, xd=None, dyd=None):
    M, D = x.shape
    mean, rstd = _stats32(x, f32(eps))
    G = K.ln_bwd_partial_rows(M, D)
    assert G == _expected_partial_rows(M, D)
    # partial buffers one row longer than the kernel may write, NaN-filled
    bufs = [torch.full((G + 1, D), math.nan, device=dev) for _ in range(3)]
    dx, dxb, pg, pb, pc = K.ln_bwd(
        dy.to(dev) if dyd is None else dyd, x.to(dev) if xd is None else xd, mean.to(dev), rstd.to(dev), g.to(dev),
        dres=None if dres is None else dres.to(dev), dres_pool=None if dres_pool is None else dres_pool.to(dev),
        pool_n=pool_n, want_bf16=full, want_colsum=full, pg_out=bufs[0][:G], pb_out=bufs[1][:G],
        pc_out=bufs[2][:G] if full else None)
    r64, r32 = _ln_bwd_refs(x, dy, g, f32(eps), mean, rstd, dres, dres_pool, pool_n)
    check(f"ln_bwd.dx {tag}", dx, r64["dx"], r32["dx"])
    assert pg.shape == pb.shape == (G, D)
    check(f"ln_bwd.dgamma {tag}", K.colsum_reduce(pg), r64["dgamma"], r32["dgamma"])
    check(f"ln_bwd.dbeta {tag}", K.colsum_reduce(pb), r64["dbeta"], r32["dbeta"])
    if full:
        assert same_bits(dxb, dx.to(BF16)), f"ln_bwd.dx_bf16 {tag}"
        check(f"ln_bwd.colsum {tag}", K.colsum_reduce(pc), r64["colsum"], r32["colsum"])
    else:
        assert dxb is None and pc is None
    for t in bufs[:3 if full else 2]:   # G rows written, the row after them untouched
        assert torch.isfinite(t[:G]).all() and torch.isnan(t[G]).all(), tag
    return dx


def _ln_bwd_inputs(M, D, gdt, xdt, seed):
    return (_randn((M, D), seed, xdt, 3.0, 1.0), _randn((M, D), seed + 1, gdt), _randn((D,), seed + 2),
            _randn((M, D), seed + 3))


@pytest.mark.parametrize("D,gdt,xdt", _LN_CASES)
def test_ln_bwd(dev, D, gdt, xdt):
    x, dy, g, dres = _ln_bwd_inputs(7, D, gdt, xdt, 200 + D)
    _check_ln_bwd(f"D{D} dres", dev, x, dy, g, dres=dres, full=True)
    _check_ln_bwd(f"D{D} plain", dev, x, dy, g, eps=1e-12, full=False)


@pytest.mark.parametrize("M,D", [(2053, 768), (4101, 64)])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_ln_bwd_row_loop(dev, M, D, dt):
    """the smallest M at which a wave takes a second row: 4 * 512 + 5 above
    D = 512, 4 * 1024 + 5 at or below it"""
    assert K.ln_bwd_partial_rows(M, D) * 4 < M <= K.ln_bwd_partial_rows(M, D) * 4 + 5
    x, dy, g, dres = _ln_bwd_inputs(M, D, dt, dt, 300 + D)
    _check_ln_bwd(f"M{M} D{D}", dev, x, dy, g, dres=dres, full=True)


_POOL = [(3, 5, 260), (2, 50, 768)]


@pytest.mark.parametrize("Bp,n,D", _POOL)
@pytest.mark.parametrize("dt", [F32, BF16])
def test_ln_bwd_fused_pool(dev, Bp, n, D, dt):
    """dres_pool: the avg-pool backward fused into the LN backward, against the
    explicit fp64 pool gradient, and bitwise against the unfused pair
    (pool_bwd, then ln_bwd with that dres)"""
    x, dy, g, _ = _ln_bwd_inputs(Bp * n, D, dt, dt, 400 + D)
    dp = _randn((Bp, D), 404)
    dx = _check_ln_bwd(f"pool B{Bp} n{n} D{D}", dev, x, dy, g, dres_pool=dp, pool_n=n, full=True)
    dres = K.pool_bwd(dp.to(dev), n).reshape(Bp * n, D)
    mean, rstd = _stats32(x, f32(1e-6))
    dx2 = K.ln_bwd(dy.to(dev), x.to(dev), mean.to(dev), rstd.to(dev), g.to(dev), dres=dres)[0]
    assert same_bits(dx, dx2)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_ln_bwd_strided(dev, dt):
    M, D = 5, 260
    wx, wdy = _randn((M, D + 12), 51, dt, 3.0, 1.0), _randn((M, D + 24), 52, dt)
    g, dres = _randn((D,), 53), _randn((M, D), 54)
    wxd, wdyd = wx.to(dev), wdy.to(dev)
    _check_ln_bwd("strided", dev, wx[:, 8:8 + D], wdy[:, 4:4 + D], g, dres=dres, full=True, xd=wxd[:, 8:8 + D],
                  dyd=wdyd[:, 4:4 + D])


# ------------------------------------------------------------------ multi-tensor
MT_SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 8196, 12289]
MT_ZERO_ENTRY = 1    # g = m = v = 0 there


def _mt_layout(extra=()):
    """(offset, n) of the entries inside one flat allocation: each starts on a
    multiple of 4 elements (16 B of f32, 8 B of bf16), so n and nothing else
    picks the 16-B or the element path; `extra` = (shift, n) entries that start
    `shift` elements past such a boundary."""
    ents, off = [], 0
    for n in MT_SIZES:
        ents.append((off, n))
        off += (n + 3) // 4 * 4
    for shift, n in extra:
        ents.append((off + shift, n))
        off += 4 + (n + 3) // 4 * 4
    return ents, off


def _plan(ents, flats, dev, shadow_of=lambda i: True, shifts=None):
    """flats: device tensors p, g, m, v, shadow (None to leave a pointer unset);
    shifts[i] = further element shifts of entry i's (f32 tensors, shadow)"""
    rows = []
    for i, (off, n) in enumerate(ents):
        ptrs = []
        for j, f in enumerate(flats):
            o = off + (0 if shifts is None else shifts[i][1 if j == 4 else 0])
            use = f is not None and (j != 4 or shadow_of(i))
            ptrs.append(f[o:o + n].data_ptr() if use else None)
        rows.append((*ptrs, n))
    return K.MultiTensorPlan(rows, dev)


ADAMW_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, gs=0.5)


def _adamw_state(ents, total):
    p, g = _randn((total,), 61), _randn((total,), 62)
    m = _randn((total,), 63, F32, 0.1)
    v = torch.rand((total,), generator=_gen(64)) * 0.01
    off, n = ents[MT_ZERO_ENTRY]
    g[off:off + n] = 0
    m[off:off + n] = 0
    v[off:off + n] = 0
    return p, g, m, v


def _adamw_formula(state, ts, dt, by_value):
    """The documented update (include/maeclip.h, torch's _single_tensor_adamw) in
    dtype dt, every hyper-parameter the fp32 value the kernel is handed. by_value:
    step_size and bc2_sqrt are the fp32 values the wrapper computes on the host;
    otherwise they are formed from the fp32 lr / betas as the kernel does from a
    device step count. Returns [(p, m, v)] after each step."""
    T = lambda val: torch.tensor(f32(val), dtype=dt)
    hp = ADAMW_HP
    lr, b1, b2, eps, wd, gs = (T(hp[k]) for k in ("lr", "b1", "b2", "eps", "wd", "gs"))
    p, g, m, v = (t.to(dt).clone() for t in state)
    one = torch.tensor(1.0, dtype=dt)
    out = []
    for t in ts:
        if by_value:
            step_size = T(hp["lr"] / (1.0 - hp["b1"] ** t))
            bc2_sqrt = T((1.0 - hp["b2"] ** t) ** 0.5)
        else:
            tt = torch.tensor(float(t), dtype=dt)
            step_size = lr / (one - torch.pow(b1, tt))
            bc2_sqrt = (one - torch.pow(b2, tt)).sqrt()
        gg = g * gs
        p = p * (one - lr * wd)
        m = b1 * m + (one - b1) * gg
        v = b2 * v + (one - b2) * gg * gg
        p = p - step_size * m / (v.sqrt() / bc2_sqrt + eps)
        out.append((p.clone(), m.clone(), v.clone()))
    return out


def _adamw_torch(state, t0, nsteps):
    """reference B: torch.optim.AdamW in fp64 with Python-double hyper-parameters"""
    hp = ADAMW_HP
    p, g, m, v = (t.double().clone() for t in state)
    w = torch.nn.Parameter(p)
    opt = torch.optim.AdamW([w], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"],
                            foreach=False)
    opt.state[w] = dict(step=torch.tensor(float(t0)), exp_avg=m, exp_avg_sq=v)
    out = []
    for _ in range(nsteps):
        w.grad = g * hp["gs"]
        opt.step()
        out.append((w.detach().clone(), m.clone(), v.clone()))
    return out


def _run_adamw(dev, ents, total, state, ts, by_value, shifts=None):
    flats = [t.to(dev) for t in state] + [torch.zeros(total, dtype=BF16, device=dev)]
    shadowed = lambda i: i % 2 == 0 or i >= len(MT_SIZES)
    plan = _plan(ents, flats, dev, shadowed, shifts)
    hp = ADAMW_HP
    step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    out = []
    for t in ts:
        if by_value:
            K.adamw_multi(plan, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], t, grad_scale=hp["gs"])
        else:
            step_dev.fill_(t)
            # a deliberately wrong host step: the kernel must take t from the device
            K.adamw_multi(plan, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], 7, grad_scale=hp["gs"],
                          step_ptr=step_dev)
        p, g, m, v, sh = (f.cpu() for f in flats)
        assert same_bits(g, state[1]), "the gradient is not written"
        out.append((p, m, v, sh))
    return out, shadowed


def _mask(ents, total, pick=lambda i: True):
    k = torch.zeros(total, dtype=torch.bool)
    for i, (off, n) in enumerate(ents):
        if pick(i):
            k[off:off + n] = True
    return k


@pytest.mark.parametrize("ts", [(1, 2, 3), (1000,)], ids=["t1-3", "t1000"])
@pytest.mark.parametrize("by_value", [True, False], ids=["by_value", "step_ptr"])
def test_adamw_multi(dev, ts, by_value):
    # one more entry one element past a 16-B boundary (4-B aligned only): the element path
    ents, total = _mt_layout(extra=[(1, 8)])
    state = _adamw_state(ents, total)
    got, shadowed = _run_adamw(dev, ents, total, state, ts, by_value)
    ref_a = _adamw_formula(state, ts, torch.float64, by_value)
    e32 = _adamw_formula(state, ts, F32, by_value)
    ref_b = _adamw_torch(state, ts[0] - 1, len(ts))
    inside = _mask(ents, total)
    with_sh, without = _mask(ents, total, shadowed), _mask(ents, total, lambda i: not shadowed(i))
    mode = "by_value" if by_value else "step_ptr"
    for s, t in enumerate(ts):
        p, m, v, sh = got[s]
        for name, o, a, e, b in zip("pmv", (p, m, v), ref_a[s], e32[s], ref_b[s]):
            check(f"adamw.{name} {mode} t{t}", o[inside], a[inside], e[inside])
            # reference B: the kernel differs by design (1 - beta2 from the fp32
            # beta2, ...); its distance is bounded by that of the formula itself,
            # FACTOR * max|A - B|. (On p, |A - B| ~ 7e-8 is below the fp32 spacing
            # of p at |p| >= 2, 2.4e-7: the bound also limits p's own rounding to
            # about one ulp. Measured: kernel 2.6 |A - B| at most, m and v 1.2.)
            dist_ab = (a - b)[inside].abs().max().item()
            dist_kb = (o.double() - b)[inside].abs().max().item()
            print(f"[torch-adamw] {name} {mode} t{t} |A-B| {dist_ab:.3e} |kernel-B| {dist_kb:.3e}")
            assert dist_kb <= FACTOR * dist_ab, (name, mode, t, dist_kb, dist_ab)
            # elements between the entries are nobody's
            assert same_bits(o[~inside], state["pgmv".index(name)][~inside])
        assert same_bits(sh[with_sh], p.to(BF16)[with_sh]), "shadow != bf16(p)"
        assert not sh[without].any() and not sh[~inside].any(), "a shadow nobody asked for was written"
    off, n = ents[MT_ZERO_ENTRY]   # g = m = v = 0: only the decay moves p
    assert not got[-1][1][off:off + n].any() and not got[-1][2][off:off + n].any()


# bf16 conversion edge values: +-0, exact ties to even (down and up), fp32
# subnormals, +-inf, the largest finite fp32 (rounds up to inf), NaN
_CAST_SPECIALS = [0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -20,
                  1e-40, -1e-40, 2.0 ** -133, 2.0 ** -134 * 3, math.inf, -math.inf, 3.4028234663852886e38,
                  -3.4028234663852886e38, 3.3961775292304e38, math.nan, 2.0 ** -126, 65280.0 + 128.0]


def _cast_source(ents, total):
    src = _randn((total,), 71, F32, 3.0)
    S = len(_CAST_SPECIALS)
    sp = torch.tensor(_CAST_SPECIALS, dtype=F32)
    for k, (off, n) in enumerate(ents):
        idx = torch.arange(min(n, S))
        src[off + idx] = sp[(idx + 5 * k) % S]
        if n > 2 * S:   # the last elements too (the ragged end of an entry)
            src[off + n - S + idx] = sp[(idx + k) % S]
    return src


def test_cast_multi(dev):
    """p4 = bf16(p0), bitwise torch's round-to-nearest-even, through the 16-B path,
    the element path (n % 4 != 0) and entries that are not 16-B / 8-B aligned
    (source one element past a boundary, destination 2 or 4 bytes past one)"""
    # (element shift of the source, of the destination) of the extra entries
    mis = [(1, 1), (0, 1), (0, 2), (2, 0), (1, 0)]
    ents, total = _mt_layout(extra=[(0, 8)] * len(mis))
    shifts = [(0, 0)] * len(MT_SIZES) + mis
    src = _cast_source(ents, total)
    want = src.to(BF16)
    assert torch.isinf(want).sum() >= 4 and torch.isnan(want).any()
    srcd = src.to(dev)
    dst = torch.zeros(total, dtype=BF16, device=dev)
    plan = _plan(ents, [srcd, None, None, None, dst], dev, shifts=shifts)
    K.cast_multi(plan)
    got = dst.cpu()
    assert same_bits(srcd, src)
    written = torch.zeros(total, dtype=torch.bool)
    for (off, n), (ss, ds) in zip(ents, shifts):
        g, s = got[off + ds:off + ds + n], src[off + ss:off + ss + n]
        w = s.to(BF16)
        nan = torch.isnan(s)
        assert torch.equal(torch.isnan(g), nan), (off, n)   # NaN stays NaN, nothing else becomes one
        assert same_bits(g[~nan], w[~nan]), (off, n, ss, ds)
        written[off + ds:off + ds + n] = True
    assert not got[~written].view(torch.int16).any(), "a write outside the entries"


# --------------------------------------------------------- reductions and gathers
def test_reduce_batch(dev):
    shapes = [(1, 1), (3, 64), (13, 65), (16, 100), (17, 768), (29, 1), (512, 256), (1024, 4)]
    scale = 0.37
    parts = [_randn(s, 80 + i) for i, s in enumerate(shapes)]
    pd = [p.to(dev) for p in parts]
    outs = []
    for _ in range(2):
        rb = K.ReduceBatch()
        o = [rb.add(p, scale=scale, out=torch.full((p.shape[1],), math.nan, device=dev)) for p in pd]
        rb.flush()
        outs.append(o)
    s32 = torch.tensor(scale, dtype=F32)
    for p, a, b in zip(parts, *outs):
        check(f"colsum_multi P{p.shape[0]} N{p.shape[1]}", a, p.double().sum(0) * f32(scale), p.sum(0) * s32)
        assert same_bits(a, b), "second flush differs"


@pytest.mark.parametrize("D", [4, 260, 768, 2048])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_rows_colsum(dev, D, dt):
    for M in (1, 3, 4, 5, 2049):   # 2049 > 4 * 512: a wave loops over rows
        x = _randn((M, D), 90 + M, dt, 2.0, 0.5)
        ob = torch.zeros((M, D), dtype=BF16, device=dev)
        part = K.rows_colsum(x.to(dev), out_bf16=ob)
        assert part.shape == (min((M + 3) // 4, 512), D)
        check(f"rows_colsum M{M} D{D}", K.colsum_reduce(part), x.double().sum(0), x.float().sum(0))
        assert same_bits(ob, x.to(BF16))


@pytest.mark.parametrize("dt", [F32, BF16])
def test_rows_colsum_strided(dev, dt):
    M, D = 5, 260
    w = _randn((M, D + 16), 95, dt)
    x = w[:, 8:8 + D]
    ob = torch.zeros((M, D), dtype=BF16, device=dev)
    part = K.rows_colsum(w.to(dev)[:, 8:8 + D], out_bf16=ob)
    check("rows_colsum strided", K.colsum_reduce(part), x.double().sum(0), x.float().sum(0))
    assert same_bits(ob, x.to(BF16))


@pytest.mark.parametrize("Bp,n,D", [(1, 2, 4)] + _POOL)
def test_pool(dev, Bp, n, D):
    x = _randn((Bp, n, D), 110, F32, 2.0, 0.5)
    check(f"pool_fwd n{n} D{D}", K.pool_fwd(x.to(dev)), x.double()[:, 1:].mean(1), x[:, 1:].mean(1))
    # backward: one fp32 division per element, cls rows zero
    dout = _randn((Bp, D), 111)
    want = _pool_grad(dout, n).reshape(Bp, n, D)
    assert not want[:, 0].any()
    dx = K.pool_bwd(dout.to(dev), n, dx=torch.full((Bp, n, D), math.nan, device=dev))
    assert same_bits(dx, want)
    pre = _randn((Bp, n, D), 112)
    acc = K.pool_bwd(dout.to(dev), n, dx=pre.to(dev), accumulate=True)
    assert same_bits(acc, pre + want)


def _mask_ids(dev, B, L, keep):
    ids_shuffle, ids_restore, _, _ = K.mask_ids(B, L, keep, seed=5, step=3, sample_offset=0, device=dev)
    s, r = ids_shuffle.cpu().long(), ids_restore.cpu().long()
    assert torch.equal(s.sort(1).values, torch.arange(L).expand(B, L))   # a permutation per sample
    assert torch.equal(torch.gather(s, 1, r), torch.arange(L).expand(B, L))
    return ids_shuffle, ids_restore, s, r


@pytest.mark.parametrize("D", [64, 260])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_tokens_fwd(dev, D, dt):
    """x[b, 0] = cls + pos[0]; x[b, 1 + j] = y[b * keep + j] + pos[1 + ids[b, j]]: one
    fp32 add of gathered rows (bf16 y with a padded row stride)"""
    B, L, keep = 3, 16, 4
    ids_d, _, ids, _ = _mask_ids(dev, B, L, keep)
    wide = _randn((B * keep, D + (8 if dt == BF16 else 0)), 120, dt)
    y = wide[:, :D]
    pos, cls = _randn((L + 1, D), 121), _randn((D,), 122)
    want = torch.empty((B, keep + 1, D))
    want[:, 0] = cls + pos[0]
    want[:, 1:] = y.float().reshape(B, keep, D) + pos[1 + ids[:, :keep]]
    x = K.tokens_fwd(wide.to(dev)[:, :D], ids_d, pos.to(dev), cls.to(dev), B, L, keep)
    assert same_bits(x, want)


@pytest.mark.parametrize("D", [64, 512])
def test_unshuffle_fwd(dev, D):
    """out[b, 0] = y[b, 0] + pos[0]; out[b, 1 + l] = (y[b, 1 + r] if r = restore[b, l] < keep
    else mask_token) + pos[1 + l]"""
    B, L, keep = 3, 16, 4
    _, rest_d, _, rest = _mask_ids(dev, B, L, keep)
    y = _randn((B * (keep + 1), D), 130)
    pos, mt = _randn((L + 1, D), 131), _randn((D,), 132)
    y3 = y.view(B, keep + 1, D)
    kept = rest < keep
    rows = torch.gather(y3[:, 1:], 1, rest.clamp(max=keep - 1)[:, :, None].expand(B, L, D))
    want = torch.empty((B, L + 1, D))
    want[:, 0] = y3[:, 0] + pos[0]
    want[:, 1:] = torch.where(kept[:, :, None], rows, mt.expand(B, L, D)) + pos[1:]
    assert kept.sum().item() == B * keep
    out = K.unshuffle_fwd(y.to(dev), rest_d, mt.to(dev), pos.to(dev), B, L, keep)
    assert same_bits(out, want)


def test_embed_fwd_clamps_ids(dev):
    """ids of -1 and V read rows 0 and V - 1 (documented; clamped before the read)"""
    B, T, D, V = 2, 5, 260, 11
    word, pos = _randn((V, D), 140), _randn((T + 3, D), 141)
    ids = torch.tensor([[0, -1, V, V - 1, 3], [V + 100, 5, -7, 10, 1]])
    want = word[ids.clamp(0, V - 1)] + pos[:T]
    out = K.embed_fwd(ids.to(dev), word.to(dev), pos.to(dev))
    assert same_bits(out, want.reshape(B * T, D))
