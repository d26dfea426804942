"""InfoNCE and SigLIP on the GPU: the fused kernels (K.contrastive_loss,
K.l2_normalize_bwd), their autograd Functions, and CLIPModel with
config.clip_loss = "infonce" / "siglip" through AdamW, graph.CapturedStep,
checkpoints and distributed.DataParallel.

The reference everywhere is fp64 torch autograd written here: F.normalize,
F.cross_entropy on the identity targets, F.logsigmoid, l = I T^T / exp(theta) + b
with theta and b the fp32 values the kernel reads. Bounds (the project's for
the loss kernels, tests/test_kernels_gpu.py::test_clip_loss_kernel_vs_torch and
tests/test_temperature_gpu.py): loss 1e-5 max(1, |ref|); dI, dT 1e-4 of
max |grad_ref|; d theta and d b DTEMP_TOL = 1e-4 of the cancellation-aware
scales sum |dl| |l - b| and sum |dl|. A figure over its bound is not waved
through: torch's own fp32 autograd on the same inputs is then the yardstick,
the figure may be at most twice its deviation, and both are recorded.

Shapes: N = 1, 2, a ragged 16-row block either side of 16, several blocks and
waves (100, 257), and 4100 for several j-splits of the statistics pass with a
ragged last tile; P = 256 (wide and 64-column gradient chunks are both taken:
few gradient blocks -> narrow, N = 4100 -> wide) and P = 128 on strided rows."""
import functools
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from tests.helpers import C0, make_batch, product_config, record_parity, same_bits

pytestmark = pytest.mark.gpu

KW = {k: v for k, v in C0.items() if k != "batch_size"}
DTEMP_TOL = 1e-4
LN007, LN01 = math.log(0.07), math.log(0.1)
# kind -> (theta, b) pairs
PARAMS = {"infonce": [(0.0, None), (LN007, None)], "siglip": [(LN01, -10.0), (0.0, 0.5)]}


def _f32(v):
    return torch.tensor([v], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _inputs(N, P):
    """LayerNorm'd random rows, as the projection heads emit (CPU fp32)"""
    def rows(seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return F.layer_norm(torch.randn((N, P), generator=g), (P,))
    return rows(131 + N), rows(132 + N)


def reference(I, T, kind, theta32, bias32=None, dtype=torch.float64, normalize=False):
    """torch autograd of the loss at `dtype` on CPU: dict of loss, dI, dT,
    dtheta, dbias, row terms and the scales of d theta and d b"""
    Il = I.detach().cpu().to(dtype).requires_grad_(True)
    Tl = T.detach().cpu().to(dtype).requires_grad_(True)
    th = theta32.detach().cpu().to(dtype).reshape(()).clone().requires_grad_(True)
    b = (torch.zeros((), dtype=dtype) if bias32 is None else bias32.detach().cpu().to(dtype).reshape(()).clone())
    b.requires_grad_(True)
    In, Tn = (F.normalize(Il, dim=-1), F.normalize(Tl, dim=-1)) if normalize else (Il, Tl)
    N = Il.shape[0]
    l = In @ Tn.T / th.exp() + b
    l.retain_grad()
    if kind == "infonce":
        tgt = torch.arange(N)
        rows = (F.cross_entropy(l, tgt, reduction="none") + F.cross_entropy(l.T, tgt, reduction="none")) / (2 * N)
    else:
        z = 2 * torch.eye(N, dtype=dtype) - 1
        rows = -F.logsigmoid(z * l).sum(1) / N
    loss = rows.sum()
    loss.backward()
    dl = l.grad
    return dict(loss=loss.item(), dI=Il.grad, dT=Tl.grad, dth=th.grad.item(), db=b.grad.item(), rows=rows.detach(),
                scale_t=(dl.abs() * (l.detach() - b.detach()).abs()).sum().item(), scale_b=dl.abs().sum().item(),
                dl=dl)


def _held(name, err, bound, yard, **info):
    """err <= bound, or else at most twice the deviation `yard()` of torch's fp32
    autograd from the same fp64 reference; both figures are recorded"""
    if err <= bound:
        return
    y = yard()
    record_parity("contrastive_over_bound", what=name, err=err, bound=bound, torch_fp32=y, **info)
    assert err <= 2 * y, (name, err, bound, y, info)


def _compare(tag, kind, out, ref, I, T, th32, b32, **info):
    """loss, dI, dT, d theta, d b of a kernel result against the fp64 reference"""
    loss, dI, dT, dth, db = out
    y32 = functools.lru_cache(maxsize=None)(lambda: reference(I, T, kind, th32, b32, dtype=torch.float32))
    sc = max(ref["dI"].abs().max().item(), ref["dT"].abs().max().item(), 1e-30)
    e_loss = abs(loss.item() - ref["loss"])
    e_I = (dI.double().cpu() - ref["dI"]).abs().max().item()
    e_T = (dT.double().cpu() - ref["dT"]).abs().max().item()
    e_th = abs(dth.item() - ref["dth"])
    rec = dict(kind=kind, loss_rel=e_loss / max(1.0, abs(ref["loss"])), dI=e_I / sc, dT=e_T / sc,
               dtheta_ratio=e_th / ref["scale_t"] if ref["scale_t"] > 0 else e_th, **info)
    if db is not None:
        e_b = abs(db.item() - ref["db"])
        rec["dbias_ratio"] = e_b / ref["scale_b"]
    record_parity(tag, **rec)
    for t in (loss, dI, dT, dth) + ((db,) if db is not None else ()):
        assert torch.isfinite(t).all()
    _held("loss", e_loss, 1e-5 * max(1.0, abs(ref["loss"])), lambda: abs(y32()["loss"] - ref["loss"]), **info)
    _held("dI", e_I, 1e-4 * sc, lambda: (y32()["dI"].double() - ref["dI"]).abs().max().item(), **info)
    _held("dT", e_T, 1e-4 * sc, lambda: (y32()["dT"].double() - ref["dT"]).abs().max().item(), **info)
    _held("dtheta", e_th, DTEMP_TOL * ref["scale_t"], lambda: abs(y32()["dth"] - ref["dth"]), **info)
    if db is not None:
        _held("dbias", e_b, DTEMP_TOL * ref["scale_b"], lambda: abs(y32()["db"] - ref["db"]), **info)


def _run(K, I, T, kind, th, b, **kw):
    """(loss, dI, dT, dtheta, dbias or None) of the device-theta route with every gradient"""
    out = K.contrastive_loss(I, T, kind, 123.0, log_temperature=th, logit_bias=b, want_dtemp=True,
                             want_dbias=kind == "siglip", **kw)
    return out if kind == "siglip" else out + (None,)


def _kernel_case(dev, kind, I, T, theta, bias, tag, **info):
    from mae_clip_amd import kernels as K
    th32, b32 = _f32(theta), None if bias is None else _f32(bias)
    Id, Td = I.to(dev) if I.device.type == "cpu" else I, T.to(dev) if T.device.type == "cpu" else T
    th, b = th32.to(dev), None if b32 is None else b32.to(dev)
    ref = reference(Id, Td, kind, th32, b32)
    out = _run(K, Id, Td, kind, th, b)
    _compare(tag, kind, out, ref, Id, Td, th32, b32, theta=theta, **info)
    N = Id.shape[0]
    if kind == "infonce" and N == 1:
        assert out[0].item() == 0.0 and not out[1].any() and not out[2].any() and out[3].item() == 0.0
    # fixed-order sums: a second call is bitwise equal in every output
    out2 = _run(K, Id, Td, kind, th, b)
    for a, c in zip(out, out2):
        assert a is None or same_bits(a, c)
    # tau by value: the same kernels, tau = f32(exp(theta)) from the host; held to
    # the same bounds, and bit for bit the device route where the two tau are the
    # same float (exp(0) = 1 exactly)
    tau = torch.exp(th32).item()
    lv, dIv, dTv = K.contrastive_loss(Id, Td, kind, tau, logit_bias=b)[:3]
    sc = max(ref["dI"].abs().max().item(), ref["dT"].abs().max().item(), 1e-30)
    if theta == 0.0:
        assert same_bits(lv, out[0]) and same_bits(dIv, out[1]) and same_bits(dTv, out[2])
    else:
        # the host's exp may round tau one ulp apart from the device's: the two
        # routes then differ by that ulp's effect, far inside the bounds
        assert abs(lv.item() - out[0].item()) <= 1e-5 * max(1.0, abs(ref["loss"]))
        assert (dIv - out[1]).abs().max().item() <= 1e-4 * sc and (dTv - out[2]).abs().max().item() <= 1e-4 * sc
    return out, ref


CASES = [(kind, N, th, b) for kind, ps in PARAMS.items() for th, b in ps for N in (1, 2, 15, 16, 17, 100, 257)]


@pytest.mark.parametrize("kind,N,theta,bias", CASES)
def test_kernel_vs_fp64(dev, kind, N, theta, bias):
    I, T = _inputs(N, 256)
    _kernel_case(dev, kind, I, T, theta, bias, "contrastive_kernel_vs_fp64", N=N, P=256)


@pytest.mark.parametrize("kind", ["infonce", "siglip"])
def test_kernel_strided_p128(dev, kind):
    """P = 128 rows that are views into wider buffers (row strides 200 and 144)"""
    N = 50
    I0, T0 = _inputs(N, 128)
    bufI = torch.full((N, 200), 7.0, device=dev)
    bufT = torch.full((N, 144), -3.0, device=dev)
    bufI[:, 8:136] = I0.to(dev)
    bufT[:, 16:144] = T0.to(dev)
    I, T = bufI[:, 8:136], bufT[:, 16:144]
    assert I.stride(0) == 200 and not I.is_contiguous()
    theta, bias = PARAMS[kind][0]
    _kernel_case(dev, kind, I, T, theta, bias, "contrastive_kernel_strided", N=N, P=128)


@pytest.mark.parametrize("kind", ["infonce", "siglip"])
def test_kernel_n4100(dev, kind):
    I, T = _inputs(4100, 256)
    theta, bias = PARAMS[kind][0]
    _kernel_case(dev, kind, I, T, theta, bias, "contrastive_kernel_vs_fp64", N=4100, P=256)


@pytest.mark.parametrize("kind", ["infonce", "siglip"])
@pytest.mark.parametrize("N,rows", [(100, (37, 50)), (1024, (896, 128)), (2500, (2100, 400))])
def test_gradient_rows(dev, kind, N, rows):
    """Data-parallel form: the loss is the full batch's, a slice's dI / dT are the
    full gradient's rows, d theta / d b of a partition of the rows add up to the
    full values; row_loss sums to the loss; want_grad=False gives the same loss."""
    from mae_clip_amd import kernels as K
    I, T = (x.to(dev) for x in _inputs(N, 256))
    theta, bias = PARAMS[kind][0]
    th32, b32 = _f32(theta), None if bias is None else _f32(bias)
    th, b = th32.to(dev), None if b32 is None else b32.to(dev)
    ref = reference(I, T, kind, th32, b32)
    full = _run(K, I, T, kind, th, b)
    gmax = max(full[1].abs().max().item(), full[2].abs().max().item())
    r0, nr = rows
    parts = [(0, r0), (r0, nr)] + ([(r0 + nr, N - r0 - nr)] if r0 + nr < N else [])
    tot_t = tot_b = 0.0
    for p0, pn in parts:
        part = _run(K, I, T, kind, th, b, grad_rows=(p0, pn))
        assert torch.equal(part[0], full[0])
        assert part[1].shape == (pn, 256) and part[2].shape == (pn, 256)
        assert (part[1] - full[1][p0:p0 + pn]).abs().max().item() <= 1e-6 * gmax
        assert (part[2] - full[2][p0:p0 + pn]).abs().max().item() <= 1e-6 * gmax
        tot_t += part[3].item()
        tot_b += part[4].item() if part[4] is not None else 0.0
    assert abs(tot_t - full[3].item()) <= 1e-6 * ref["scale_t"], (tot_t, full[3].item(), ref["scale_t"])
    if kind == "siglip":
        assert abs(tot_b - full[4].item()) <= 1e-6 * ref["scale_b"], (tot_b, full[4].item(), ref["scale_b"])
    loss, dI, dT, rl = K.contrastive_loss(I, T, kind, 1.0, log_temperature=th, logit_bias=b, row_loss=True,
                                          grad_rows=(r0, nr))
    assert torch.equal(loss, full[0]) and rl.shape == (N,)
    assert abs(rl.double().sum().item() - loss.item()) <= 1e-6 * max(1.0, abs(loss.item()))
    # a row's loss N rl_i is held to the loss bound
    per_row = N * ref["rows"]
    assert (N * rl.double().cpu() - per_row).abs().max().item() <= 1e-5 * max(1.0, per_row.abs().max().item())
    ln = K.contrastive_loss(I, T, kind, 1.0, want_grad=False, log_temperature=th, logit_bias=b)
    assert ln[1] is None and ln[2] is None and torch.equal(ln[0], full[0])


def test_siglip_extreme_logits(dev):
    """logits of +-80 at tau = 1 (scaled embeddings): a positive pair at -80, a
    negative pair at +80, positives at +80 -- log sigma and sigma saturate, and
    loss and gradients stay finite and within the bounds"""
    N = 40
    I0, _ = _inputs(N, 256)
    s = math.sqrt(80.0 / 256.0)
    I = I0 * s
    T = I.clone()
    T[N // 2:] = -T[N // 2:]
    T[1] = T[0]
    out, ref = _kernel_case(dev, "siglip", I, T, 0.0, 0.0, "siglip_extremes", N=N, P=256)
    l = I.double() @ T.double().T
    assert l.max().item() > 79 and l.min().item() < -79
    assert l[0, 1].item() > 79 and l[N - 1, N - 1].item() < -79


@pytest.mark.parametrize("M,P", [(1, 64), (5, 256), (300, 64), (300, 256)])
def test_l2_normalize_bwd(dev, M, P):
    """fp64 autograd of F.normalize (eps 1e-12) on row-strided views; the last row
    of the larger cases is all zero (dx = g / eps). Bound per row: 1e-5 of
    max |g| / max(||x||, eps), the size of the terms of (g - y (y.g)) / ||x||, each
    an fp32 sum of P <= 256 products (sqrt(P) 2^-24 ~ 1e-6 typical)."""
    from mae_clip_amd import kernels as K
    g0 = torch.Generator(device="cpu").manual_seed(500 + M + P)
    bx = torch.randn((M, P + 12), generator=g0)
    bg = torch.randn((M, P + 4), generator=g0)
    if M > 1:
        bx[-1] = 0.0
    x, g = bx.to(dev)[:, 4:4 + P], bg.to(dev)[:, :P]
    x64 = x.double().cpu().requires_grad_(True)
    F.normalize(x64, p=2, dim=-1, eps=1e-12).backward(g.double().cpu())
    dx = K.l2_normalize_bwd(x, g, 1e-12)
    y = K.l2_normalize(x, 1e-12)
    assert (y.double().cpu() - F.normalize(x64.detach(), dim=-1)).abs().max().item() < 1e-6
    scale = g.double().cpu().abs().amax(1) / x64.detach().norm(dim=1).clamp_min(1e-12)
    err = (dx.double().cpu() - x64.grad).abs().amax(1) / scale
    record_parity("l2_normalize_bwd_vs_fp64", M=M, P=P, worst=err.max().item())
    assert torch.isfinite(dx).all() and err.max().item() <= 1e-5, err.max().item()
    if M > 1:
        # the g / eps branch (one fp32 division: an ulp from torch's own quotient)
        assert torch.allclose(dx[-1].cpu(), (g[-1] / 1e-12).cpu(), rtol=1e-6, atol=0)
    assert same_bits(dx, K.l2_normalize_bwd(x, g, 1e-12))


@pytest.mark.parametrize("kind", ["infonce", "siglip"])
def test_autograd_wiring(dev, kind):
    """ContrastiveLossFn with grad_output 3.0 == 3 x the kernel gradients, and
    L2NormalizeFn composed with it == fp64 end to end"""
    from mae_clip_amd import functions as Fn, kernels as K
    N = 37
    I0, T0 = (x.to(dev) for x in _inputs(N, 256))
    theta, bias = PARAMS[kind][0]
    th32, b32 = _f32(theta), None if bias is None else _f32(bias)

    def leaves():
        return (I0.clone().requires_grad_(True), T0.clone().requires_grad_(True), th32.to(dev).requires_grad_(True),
                None if b32 is None else b32.to(dev).requires_grad_(True))
    I, T, th, b = leaves()
    k = _run(K, I0, T0, kind, th.detach(), None if b is None else b.detach())
    (Fn.ContrastiveLossFn.apply(I, T, kind, 1.0, None, th, b) * 3.0).backward()
    gm = max(k[1].abs().max().item(), k[2].abs().max().item())
    assert (I.grad - 3 * k[1]).abs().max().item() <= 1e-6 * 3 * gm
    assert (T.grad - 3 * k[2]).abs().max().item() <= 1e-6 * 3 * gm
    assert th.grad.shape == (1,) and abs(th.grad.item() - 3 * k[3].item()) <= 1e-6 * abs(3 * k[3].item()) + 1e-30
    if b is not None:
        assert b.grad.shape == (1,) and abs(b.grad.item() - 3 * k[4].item()) <= 1e-6 * abs(3 * k[4].item()) + 1e-30
    # normalised embeddings, end to end
    I, T, th, b = leaves()
    loss = Fn.ContrastiveLossFn.apply(Fn.L2NormalizeFn.apply(I), Fn.L2NormalizeFn.apply(T), kind, 1.0, None, th, b)
    loss.backward()
    ref = reference(I0, T0, kind, th32, b32, normalize=True)
    out = (loss.detach(), I.grad, T.grad, th.grad, None if b is None else b.grad)
    _compare("contrastive_normalized_autograd", kind, out, ref, I0, T0, th32, b32, N=N, P=256)


# ------------------------------------------------------------------ model level
def _model(kind, seed=0):
    from mae_clip_amd.CLIP import CLIPModel
    with product_config(precision="fp32", learnable_temperature=True, clip_loss=kind, **KW):
        torch.manual_seed(seed)
        m = CLIPModel(temperature=0.5)
    return m.cuda().eval()   # no dropout and one MAE mask: runs are comparable


def _groups(m):
    nodecay = [p for n, p in m.named_parameters() if n in ("log_temperature", "logit_bias")]
    rest = [p for n, p in m.named_parameters() if p.requires_grad and n not in ("log_temperature", "logit_bias")]
    return [dict(params=rest, weight_decay=1e-3), dict(params=nodecay, weight_decay=0.0)]


@pytest.mark.parametrize("kind", ["infonce", "siglip"])
def test_model_loss_and_gradients(dev, kind):
    m = _model(kind)
    seen = {}
    hooks = [m.image_projection.register_forward_hook(lambda mod, a, out: seen.__setitem__("I", out.detach())),
             m.text_projection.register_forward_hook(lambda mod, a, out: seen.__setitem__("T", out.detach()))]
    batch = {k: v.to(dev) for k, v in make_batch(5, 32, seed=5).items()}
    loss = m(batch)
    loss.backward()
    for h in hooks:
        h.remove()
    assert (m.logit_bias is not None) == (kind == "siglip")
    ref = reference(seen["I"], seen["T"], kind, m.log_temperature.detach().cpu(),
                    None if m.logit_bias is None else m.logit_bias.detach().cpu(), normalize=True)
    clip = m.last_losses["clip"].item()
    record_parity("contrastive_model_c0_fp32", kind=kind, clip=clip, ref=ref["loss"])
    assert abs(clip - ref["loss"]) <= 1e-5 * max(1.0, abs(ref["loss"])), (clip, ref["loss"])
    for name, p in m.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all(), name
    assert abs(m.log_temperature.grad.item() - ref["dth"]) <= DTEMP_TOL * ref["scale_t"]
    if kind == "siglip":
        assert abs(m.logit_bias.grad.item() - ref["db"]) <= DTEMP_TOL * ref["scale_b"]
    with torch.no_grad():                    # the no-grad route of contrastive_loss
        m(batch)
    assert abs(m.last_losses["clip"].item() - clip) <= 1e-6 * max(1.0, abs(clip))


def _train(dev, kind, captured, steps=3, first=0, model=None, opt=None):
    from mae_clip_amd.optim import AdamW
    from mae_clip_amd.graph import CapturedStep
    m = _model(kind) if model is None else model
    opt = AdamW(_groups(m), lr=1e-3) if opt is None else opt
    runner = CapturedStep(m, opt, enabled=captured)
    losses = []
    for it in range(first, first + steps):
        batch = {k: v.to(dev) for k, v in make_batch(8, 32, seed=60 + it).items()}
        losses.append(runner.step(batch).detach().clone())
    return losses, m, opt, runner


@pytest.mark.parametrize("kind", ["infonce", "siglip"])
def test_captured_steps_equal_eager(dev, kind):
    le, me, _, _ = _train(dev, kind, False)
    lg, mg, _, runner = _train(dev, kind, True)
    assert runner.captures == 1
    for a, b in zip(le, lg):
        assert same_bits(a, b), (a.item(), b.item())
    for (n, p), (_, q) in zip(me.named_parameters(), mg.named_parameters()):
        assert same_bits(p, q), n
    assert me.log_temperature.item() != torch.tensor(math.log(0.5), dtype=torch.float32).item()
    if kind == "siglip":
        assert me.logit_bias.item() != -10.0


def test_checkpoint_resume_siglip(dev, tmp_path):
    """two steps, save, a third step == load into a fresh model + the third step"""
    from mae_clip_amd.optim import AdamW
    from mae_clip_amd.checkpoint import save_checkpoint, load_checkpoint
    _, m, opt, _ = _train(dev, "siglip", False, steps=2)
    path = str(tmp_path / "c.pt")
    save_checkpoint(path, m, opt)
    (l3,), _, _, _ = _train(dev, "siglip", False, steps=1, first=2, model=m, opt=opt)
    m2 = _model("siglip", seed=9)
    opt2 = AdamW(_groups(m2), lr=1e-3)
    load_checkpoint(path, m2, opt2)
    (r3,), _, _, _ = _train(dev, "siglip", False, steps=1, first=2, model=m2, opt=opt2)
    assert same_bits(l3, r3)
    assert "logit_bias" in m.state_dict() and same_bits(m.logit_bias, m2.logit_bias)
    for (n, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert same_bits(p, q), n


# --------------------------------------------------------------- data parallel
B_LOCAL = 4


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_rank(rank, world, port, kind, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mae_clip_amd import _lib
        from mae_clip_amd.distributed import DataParallel
        _lib.load()
        m = _model(kind)
        dp = DataParallel(m, bucket_mb=0.5)
        full = make_batch(world * B_LOCAL, 32, seed=3)
        b = {k: v[rank * B_LOCAL:(rank + 1) * B_LOCAL].cuda() for k, v in full.items()}
        for p in m.parameters():
            p.grad = None
        m(b).backward()
        dp.sync_gradients()
        torch.cuda.synchronize()
        out[rank] = dict(grads={n: p.grad.cpu() for n, p in m.named_parameters() if p.requires_grad},
                         adopted=dp.adopted, nparams=len(dp.params), clip=m.last_losses["clip"].item())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kind", ["infonce", "siglip"])
def test_data_parallel_equals_full_batch(dev, kind):
    """Two gloo ranks on the one GPU, B = 4 each: after the SUM all-reduce every
    gradient (d theta and d b included) == the single-process gradient on the 8
    samples within tests/test_temperature_gpu.py's bound, 1e-4 of its size."""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_dp_rank, args=(2, _free_port(), kind, out), nprocs=2, join=True)
    res = [out[r] for r in range(2)]
    m = _model(kind)
    m({k: v.to(dev) for k, v in make_batch(2 * B_LOCAL, 32, seed=3).items()}).backward()
    worst = (0.0, "")
    for o in res:
        assert o["adopted"] == o["nparams"]
        assert abs(o["clip"] - m.last_losses["clip"].item()) <= 1e-6 * max(1.0, abs(o["clip"]))
        for n, p in m.named_parameters():
            if not p.requires_grad:
                continue
            g = p.grad.cpu()
            e = (o["grads"][n] - g).abs().max().item() / (g.abs().max().item() + 1e-30)
            worst = max(worst, (e, n))
    record_parity("dp2_gloo_C0_contrastive_vs_single_process", kind=kind, worst_rel=worst[0], worst=worst[1])
    assert worst[0] < 1e-4, worst
    for n in res[0]["grads"]:
        assert torch.equal(res[0]["grads"][n], res[1]["grads"][n]), n
