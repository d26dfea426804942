"""The learnable CLIP temperature on the GPU: theta = ln tau read from device
memory by the loss kernels, d loss / d theta out of the same call, through
CLIPModel, optim.AdamW, graph.CapturedStep and distributed.DataParallel.

The reference everywhere is fp64 autograd of the reference's formula
(CLIP.py:34-43) with tau = exp(theta), theta a leaf, and tau taken from the
fp32 theta the kernel reads. d theta is held to 1e-4 of its natural scale
SCALE = sum |dS S| + sum |dL L| (the terms of the sum it is), the project's
gradient bound for the loss kernel; loss, dI and dT to the bounds of
tests/test_kernels_gpu.py::test_clip_loss_kernel_vs_torch.

Shapes: the smallest that reach each path of the kernel -- a ragged last 16-row
block (N = 3, 5, 17, 33, 100), slices that start and end inside a block, more
than one j-split of the products pass (N = 600), a second 2048-column chunk of
the statistics pass (N = 2100), both ends of the P template (64, 256).

Measured on MI355X (|d theta - ref| / SCALE, worst over theta in {0, -ln 2,
1.5}): see DESIGN.md Round 9."""
import functools
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.helpers import C0, make_batch, oracle_config, product_config, record_parity, same_bits

pytestmark = pytest.mark.gpu

THETAS = {"0": 0.0, "-ln2": -math.log(2.0), "1.5": 1.5}
KW = {k: v for k, v in C0.items() if k != "batch_size"}
DTEMP_TOL = 1e-4      # of SCALE
CURVE_TOL = 1e-4      # |dloss| / loss per step, as tests/test_model_gpu.py's fp32 curves


@functools.lru_cache(maxsize=None)
def _inputs(N, P):
    """LayerNorm'd rows, as the projection heads emit (CPU fp32): the inputs of
    tests/test_kernels_gpu.py::test_clip_loss_kernel_vs_torch, seeds 31 + N and 32 + N"""
    def rows(seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return torch.nn.functional.layer_norm(torch.randn((N, P), generator=g), (P,))
    return rows(31 + N), rows(32 + N)


def _theta(v):
    return torch.tensor([v], dtype=torch.float32)


def ref64(I, T, theta32):
    """fp64 autograd of CLIP.py:34-43 + cross_entropy with tau = exp(theta):
    loss, dI, dT, d theta and SCALE = sum |dS S| + sum |dL L|"""
    I64 = I.detach().double().cpu().requires_grad_(True)
    T64 = T.detach().double().cpu().requires_grad_(True)
    th = theta32.detach().double().cpu().reshape(()).clone().requires_grad_(True)
    tau = th.exp()
    L = T64 @ I64.T / tau
    S = (I64 @ I64.T + T64 @ T64.T) / 2 * tau
    L.retain_grad()
    S.retain_grad()
    tgt = torch.softmax(S, -1)
    lt = (-tgt * torch.log_softmax(L, -1)).sum(1)
    li = (-tgt.T * torch.log_softmax(L.T, -1)).sum(1)
    loss = ((li + lt) / 2).mean()
    loss.backward()
    scale = ((S.grad * S).abs().sum() + (L.grad * L).abs().sum()).item()
    return loss.item(), I64.grad, T64.grad, th.grad.item(), scale


@functools.lru_cache(maxsize=None)
def _ref(N, P, tname):
    I, T = _inputs(N, P)
    return ref64(I, T, _theta(THETAS[tname]))


CASES = [(N, 256) for N in (1, 3, 5, 17, 33, 100, 600, 2100)] + [(33, 64), (100, 64)]


@pytest.mark.parametrize("tname", list(THETAS))
@pytest.mark.parametrize("N,P", CASES)
def test_dtemp_kernel_vs_fp64_autograd(dev, N, P, tname):
    from mae_clip_amd import kernels as K
    I, T = (x.to(dev) for x in _inputs(N, P))
    th = _theta(THETAS[tname]).to(dev)
    loss, dI, dT, dth = K.clip_loss(I, T, 123.0, log_temperature=th, want_dtemp=True)   # the float is ignored
    ref, gI, gT, gth, scale = _ref(N, P, tname)
    sc = max(gI.abs().max().item(), gT.abs().max().item(), 1e-30)
    e_loss = abs(loss.item() - ref) / max(1.0, abs(ref))
    e_I = (dI.double().cpu() - gI).abs().max().item() / sc
    e_T = (dT.double().cpu() - gT).abs().max().item() / sc
    e_th = abs(dth.item() - gth) / scale if scale > 0 else abs(dth.item() - gth)
    record_parity("dtemp_kernel_vs_fp64", N=N, P=P, theta=tname, loss_rel=e_loss, dI=e_I, dT=e_T, dtheta_ratio=e_th,
                  dtheta=gth, scale=scale)
    assert dth.shape == (1,) and dth.dtype == torch.float32
    assert e_loss < 1e-5, (loss.item(), ref)
    assert e_I <= 1e-4 and e_T <= 1e-4, (e_I, e_T)
    if N == 1:
        assert dth.item() == 0.0 and gth == 0.0
    else:
        assert abs(dth.item() - gth) <= DTEMP_TOL * scale, (dth.item(), gth, scale)
    # fixed-order sums: a second call is bitwise equal in all four outputs
    loss2, dI2, dT2, dth2 = K.clip_loss(I, T, 123.0, log_temperature=th, want_dtemp=True)
    assert same_bits(loss, loss2) and same_bits(dI, dI2) and same_bits(dT, dT2) and same_bits(dth, dth2)


@pytest.mark.parametrize("N", [100, 600])
def test_pointer_path_at_theta_0_is_the_by_value_path(dev, N):
    """exp(0) = 1 exactly: theta = 0 from device memory == temperature 1.0 by
    value, bit for bit in loss, dI and dT (the same kernels; only where tau
    comes from differs). Asking for d theta as well takes the other
    instantiation of the gradient kernel: the same expressions, which the
    compiler may contract into fused multiply-adds differently, so dI / dT then
    agree to test_clip_loss_gradient_rows' 1e-6 of the gradient's size; the
    loss, which the statistics pass makes, stays bitwise equal."""
    from mae_clip_amd import kernels as K
    I, T = (x.to(dev) for x in _inputs(N, 256))
    th = _theta(0.0).to(dev)
    lv, dIv, dTv = K.clip_loss(I, T, 1.0)
    lp, dIp, dTp = K.clip_loss(I, T, 7.0, log_temperature=th)
    assert same_bits(lv, lp) and same_bits(dIv, dIp) and same_bits(dTv, dTp)
    ln, _, _ = K.clip_loss(I, T, 7.0, want_grad=False, log_temperature=th)
    assert same_bits(lv, ln)
    ld, dId, dTd, _ = K.clip_loss(I, T, 7.0, log_temperature=th, want_dtemp=True)
    assert same_bits(lv, ld)
    assert torch.allclose(dId, dIv, rtol=0, atol=1e-6 * dIv.abs().max().item())
    assert torch.allclose(dTd, dTv, rtol=0, atol=1e-6 * dTv.abs().max().item())


@pytest.mark.parametrize("N,rows", [(100, (37, 50)), (33, (16, 17)), (300, (290, 10))])
def test_dtemp_row_slices_add_up(dev, N, rows):
    """Data-parallel form: d theta of a row slice is the slice's share of the
    sum. [0, row0), the slice and the rest add up to the full-batch value
    (1e-6 of SCALE: the per-row terms are the same, only the last sums are
    rounded apart), and a slice's dI / dT are the full gradient's rows."""
    from mae_clip_amd import kernels as K
    I, T = (x.to(dev) for x in _inputs(N, 256))
    th32 = _theta(THETAS["-ln2"])
    th = th32.to(dev)
    _, _, _, gth, scale = ref64(I, T, th32)
    lf, dIf, dTf, dthf = K.clip_loss(I, T, 1.0, log_temperature=th, want_dtemp=True)
    r0, nr = rows
    parts = [(0, r0), (r0, nr)] + ([(r0 + nr, N - r0 - nr)] if r0 + nr < N else [])
    total = 0.0
    for p0, pn in parts:
        ls, dIs, dTs, dths = K.clip_loss(I, T, 1.0, grad_rows=(p0, pn), log_temperature=th, want_dtemp=True)
        assert same_bits(ls, lf)
        assert torch.allclose(dIs, dIf[p0:p0 + pn], rtol=0, atol=1e-6 * dIf.abs().max().item())
        assert torch.allclose(dTs, dTf[p0:p0 + pn], rtol=0, atol=1e-6 * dTf.abs().max().item())
        total += float(dths.item())
    record_parity("dtemp_row_slices", N=N, row0=r0, rows=nr, sum_vs_full=abs(total - dthf.item()) / scale,
                  full_vs_ref=abs(dthf.item() - gth) / scale)
    assert abs(total - dthf.item()) <= 1e-6 * scale, (total, dthf.item(), scale)
    assert abs(dthf.item() - gth) <= DTEMP_TOL * scale


# ------------------------------------------------------------------ model level
def _pair(precision="fp32", temperature=0.5, seed=0):
    """(product CLIPModel with the learnable temperature on cuda, fp64 oracle on
    the same weights, theta64): the oracle's temperature is a plain attribute,
    set from outside to exp(theta64) -- theta64 a leaf with the product's fp32
    value"""
    from mae_clip_amd.CLIP import CLIPModel
    from oracle.ref_model import CLIPModel as RefCLIP
    torch.manual_seed(seed)
    with product_config(precision=precision, learnable_temperature=True, **KW):
        prod = CLIPModel(temperature=temperature)
    ref = RefCLIP(oracle_config(**KW))
    sd = {k: v.detach().clone() for k, v in prod.state_dict().items() if k != "log_temperature"}
    ref.load_state_dict(sd, strict=True)
    th = prod.log_temperature.detach().double().clone().requires_grad_(True)
    return prod.cuda(), ref.double(), th


def _ref_batch(batch):
    return {"image": batch["image"].double(), "input_ids": batch["input_ids"],
            "attention_mask": batch["attention_mask"]}


def test_model_dtemp_vs_oracle_fp32(dev, monkeypatch):
    """C0 shapes, fp32 parity mode, B = 5 (a ragged block): loss.backward() with
    the flag on vs the fp64 oracle model with temperature = exp(theta64)."""
    import oracle.ref_model as RM
    prod, ref, th = _pair("fp32", temperature=0.5)
    prod.eval()
    ref.eval()
    seen = []
    real = RM.clip_loss

    def spy(ie, te, temperature):
        seen.append((ie.detach(), te.detach()))
        return real(ie, te, temperature)
    monkeypatch.setattr(RM, "clip_loss", spy)
    batch = make_batch(5, 32, seed=5)
    loss = prod({k: v.to(dev) for k, v in batch.items()})
    loss.backward()
    ref.temperature = th.exp()
    rloss = ref(_ref_batch(batch))
    rloss.backward()
    assert abs(loss.item() - rloss.item()) < 1e-5 * max(1.0, abs(rloss.item())), (loss.item(), rloss.item())
    (ie, te), = seen
    _, _, _, gth, scale = ref64(ie, te, prod.log_temperature.detach().cpu())
    assert abs(gth - th.grad.item()) <= 1e-12 * scale          # the two fp64 routes agree
    g = prod.log_temperature.grad
    assert g is not None and g.shape == (1,) and g.dtype == torch.float32
    ratio = abs(g.item() - th.grad.item()) / scale
    rp = dict(ref.named_parameters())
    worst = []
    for name, p in prod.named_parameters():
        if not p.requires_grad or name == "log_temperature":
            continue
        rg = rp[name].grad
        assert p.grad is not None and rg is not None, name
        worst.append(((p.grad.double().cpu() - rg).abs().max().item() / (rg.abs().max().item() + 1e-30), name))
    worst.sort(reverse=True)
    record_parity("model_c0_fp32_dtemp_vs_oracle", dtheta_ratio=ratio, dtheta=th.grad.item(), scale=scale,
                  worst_grad_maxrel=worst[0][0], worst_grad=worst[0][1])
    assert ratio <= DTEMP_TOL, (g.item(), th.grad.item(), scale)
    assert worst[0][0] < 1e-3, worst[:3]


def _groups(model):
    rest = [p for n, p in model.named_parameters() if p.requires_grad and n != "log_temperature"]
    return [dict(params=rest, weight_decay=1e-3), dict(params=[model.log_temperature], weight_decay=0.0)]


STEPS = 6


def _product_run(dev, captured, max_grad_norm):
    from mae_clip_amd.optim import AdamW
    from mae_clip_amd.graph import CapturedStep
    prod, _, _ = _pair("fp32", temperature=0.5)
    prod.eval()       # no dropout and one MAE mask, as the oracle: the curves are comparable
    opt = AdamW(_groups(prod), lr=1e-3, max_grad_norm=max_grad_norm)
    runner = CapturedStep(prod, opt, enabled=captured)
    losses, thetas = [], []
    for it in range(STEPS):
        batch = {k: v.to(dev) for k, v in make_batch(8, 32, seed=60 + it).items()}
        losses.append(runner.step(batch).item())
        thetas.append(prod.log_temperature.detach().clone())
    return losses, thetas, runner, prod


def _oracle_run(max_grad_norm):
    _, ref, th = _pair("fp32", temperature=0.5)
    ref.eval()
    th = torch.nn.Parameter(th.detach())
    rest = [p for p in ref.parameters() if p.requires_grad]
    opt = torch.optim.AdamW([dict(params=rest, weight_decay=1e-3), dict(params=[th], weight_decay=0.0)], lr=1e-3)
    losses, thetas = [], []
    for it in range(STEPS):
        opt.zero_grad()
        ref.temperature = th.exp()
        loss = ref(_ref_batch(make_batch(8, 32, seed=60 + it)))
        loss.backward()
        if max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_(rest + [th], max_grad_norm)
        opt.step()
        losses.append(loss.item())
        thetas.append(th.item())
    return losses, thetas


@pytest.mark.parametrize("max_grad_norm", [None, 1.0])
def test_temperature_trains_under_capture(dev, max_grad_norm):
    """Six AdamW steps of the C0 model, theta in a weight_decay = 0 group (with
    and without the fused gradient clipping, which counts theta's gradient):
    the captured step == the eager step bit for bit in theta and loss after
    every step from ONE capture (theta is read from device memory, so the graph
    does not bake it in), theta moves, and the loss curve follows the fp64
    oracle + torch.optim.AdamW within CURVE_TOL per step."""
    le, te, _, _ = _product_run(dev, False, max_grad_norm)
    lg, tg, runner, prod = _product_run(dev, True, max_grad_norm)
    assert runner.captures == 1
    assert le == lg, (le, lg)
    for a, b in zip(te, tg):
        assert same_bits(a, b), (a.item(), b.item())
    start = torch.tensor(math.log(0.5), dtype=torch.float32).item()
    assert tg[-1].item() != start and len({t.item() for t in tg}) == STEPS
    assert abs(prod.current_temperature() - math.exp(tg[-1].item())) < 1e-6
    lo, to = _oracle_run(max_grad_norm)
    rels = [abs(a - b) / abs(b) for a, b in zip(lg, lo)]
    dth = [abs(a.item() - b) for a, b in zip(tg, to)]
    record_parity(f"temperature_train_curve_c0_fp32_clip_{max_grad_norm}", worst_loss_rel=max(rels),
                  worst_theta_abs=max(dth), theta_moved=tg[-1].item() - start)
    assert max(rels) < CURVE_TOL, rels


# --------------------------------------------------------------- data parallel
B_LOCAL = 4


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_model():
    from mae_clip_amd.CLIP import CLIPModel
    with product_config(precision="fp32", learnable_temperature=True, **KW):
        torch.manual_seed(0)
        m = CLIPModel(temperature=0.5)
    return m.cuda().eval()


def _dp_rank(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mae_clip_amd import _lib
        from mae_clip_amd.distributed import DataParallel
        _lib.load()
        m = _dp_model()
        dp = DataParallel(m, bucket_mb=0.5)
        full = make_batch(world * B_LOCAL, 32, seed=3)
        b = {k: v[rank * B_LOCAL:(rank + 1) * B_LOCAL].cuda() for k, v in full.items()}
        for p in m.parameters():
            p.grad = None
        m(b).backward()
        dp.sync_gradients()
        torch.cuda.synchronize()
        out[rank] = dict(grad=m.log_temperature.grad.cpu(), owned=dp.arena.owns(m.log_temperature),
                         adopted=dp.adopted, nparams=len(dp.params))
    finally:
        dist.destroy_process_group()


def test_data_parallel_dtemp_equals_full_batch(dev):
    """Two gloo ranks on the one GPU (as tests/test_distributed_gpu.py), B = 4
    each: after sync_gradients() log_temperature.grad on both ranks == the
    single-process gradient on the 8 samples within that file's fp32 bound
    (1e-4 of the gradient's size) -- a plain SUM, no rescale."""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_dp_rank, args=(2, _free_port(), out), nprocs=2, join=True)
    res = [out[r] for r in range(2)]
    m = _dp_model()
    m({k: v.to(dev) for k, v in make_batch(2 * B_LOCAL, 32, seed=3).items()}).backward()
    g = m.log_temperature.grad.cpu()
    sc = g.abs().max().item() + 1e-30
    errs = []
    for o in res:
        assert o["owned"] and o["adopted"] == o["nparams"], (o["owned"], o["adopted"], o["nparams"])
        assert o["grad"].shape == (1,)
        errs.append((o["grad"] - g).abs().max().item() / sc)
    record_parity("dp2_gloo_C0_dtemp_vs_single_process", worst_rel=max(errs), dtheta=g.item())
    assert max(errs) < 1e-4, (errs, [o["grad"] for o in res], g)
    assert torch.equal(res[0]["grad"], res[1]["grad"])
