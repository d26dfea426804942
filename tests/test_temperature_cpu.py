"""config.learnable_temperature on the CPU: the model's surface (parameter,
state_dict key, checkpoint), the C-ABI's argument checks for the two new
maeclip_clip_args fields on the real library (they return before any launch),
and the host plumbing with every launch stubbed: the parameter's gradient
through ClipLossFn, AdamW and the data-parallel GradArena. The numbers are in
tests/test_temperature_gpu.py."""
import ctypes
import json
import math

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.helpers import C0, make_batch, product_config
from tests.test_plumbing_cpu import stubbed_kernels, _free_port

KW = {k: v for k, v in C0.items() if k != "batch_size"}


def _model(precision="fp32", learnable=True, temperature=None, **over):
    from mae_clip_amd.CLIP import CLIPModel
    with product_config(precision=precision, side_stream=False, learnable_temperature=learnable, **dict(KW, **over)):
        torch.manual_seed(0)
        return CLIPModel(temperature=temperature)


# ------------------------------------------------------------ default surface
def test_flag_is_off_by_default_and_adds_no_key():
    from mae_clip_amd import config as CFG
    assert CFG.learnable_temperature is False
    off = _model(learnable=False)
    assert "log_temperature" not in off.state_dict()
    assert off.log_temperature is None and "log_temperature" not in dict(off.named_parameters())
    assert off.temperature == 1.0 and off.current_temperature() == 1.0
    on = _model(learnable=True)
    assert sorted(set(on.state_dict()) - set(off.state_dict())) == ["log_temperature"]
    assert set(off.state_dict()) <= set(on.state_dict())


@pytest.mark.parametrize("tau", [1.0, 0.5, 0.07])
def test_parameter_when_on(tau):
    m = _model(temperature=tau)
    p = m.state_dict()["log_temperature"]
    assert p.shape == (1,) and p.dtype == torch.float32
    assert p.item() == torch.tensor(math.log(tau), dtype=torch.float32).item()
    assert isinstance(m.log_temperature, torch.nn.Parameter) and m.log_temperature.requires_grad
    assert m.temperature == tau                                  # the constructor's float stays
    assert abs(m.current_temperature() - tau) <= 1e-6 * tau
    with torch.no_grad():
        m.log_temperature.fill_(1.5)
    assert abs(m.current_temperature() - math.exp(1.5)) < 1e-5 and m.temperature == tau


def test_checkpoint_round_trips_the_key(tmp_path):
    from mae_clip_amd.checkpoint import save_checkpoint, load_checkpoint
    a = _model(temperature=0.5)
    with torch.no_grad():
        a.log_temperature.fill_(-1.25)
    a.step = 3
    path = tmp_path / "ckpt.pt"
    save_checkpoint(path, a)
    assert "log_temperature" in torch.load(path, weights_only=True)["model"]
    b = _model(temperature=1.0)
    assert load_checkpoint(path, b) == 3
    assert torch.equal(b.log_temperature.detach(), torch.tensor([-1.25]))
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    # a checkpoint saved with the flag off lacks the key: no strict load into a model with it on
    off_path = tmp_path / "off.pt"
    save_checkpoint(off_path, _model(learnable=False))
    with pytest.raises(RuntimeError, match="log_temperature"):
        load_checkpoint(off_path, _model())
    c = _model(temperature=0.5)
    load_checkpoint(off_path, c, strict=False)
    assert c.log_temperature.item() == torch.tensor(math.log(0.5), dtype=torch.float32).item()


# ------------------------------------------- argument checks, real library
def _args(**kw):
    """maeclip_clip_args that pass every check up to the workspace size (ws_bytes
    0 fails it, the last one before the launches): nothing is ever launched and
    no pointer is ever followed"""
    from mae_clip_amd import _lib as L
    base = dict(I=0x1000, T=0x2000, ld_I=64, ld_T=64, N=8, P=64, temperature=1.0, loss=0x3000, workspace=0x4000,
                ws_bytes=0, ld_dI=64, ld_dT=64)
    base.update(kw)
    return L.ClipArgs(**base)


def _rc_err(a):
    from mae_clip_amd import _lib as L
    lib = L.load()
    rc = lib.maeclip_clip_loss(ctypes.byref(a), None)
    return rc, lib.maeclip_last_error().decode()


def test_ctypes_mirror_has_the_fields_and_abi_14():
    from mae_clip_amd import _lib as L
    names = [n for n, _ in L.ClipArgs._fields_]
    assert names[-2:] == ["log_temperature", "d_log_temperature"]
    assert names.index("ws_bytes") == len(names) - 3            # appended: the ABI 13 prefix is unchanged
    assert all(t is ctypes.c_void_p for n, t in L.ClipArgs._fields_ if n.endswith("log_temperature"))
    assert L.ABI_VERSION == 14 and L.load().maeclip_abi_version() == 14


def test_dtemp_argument_validation():
    WS = "workspace too small"
    # as before: both fields null reaches the workspace check, with and without gradients
    for kw in (dict(), dict(dI=0x5000, dT=0x6000)):
        rc, err = _rc_err(_args(**kw))
        assert rc < 0 and WS in err, err
    rc, err = _rc_err(_args(temperature=0.0))
    assert rc < 0 and "temperature must be > 0" in err
    # log_temperature alone is valid, and the by-value temperature is then not looked at
    for kw in (dict(), dict(temperature=0.0), dict(dI=0x5000, dT=0x6000)):
        rc, err = _rc_err(_args(log_temperature=0x7000, **kw))
        assert rc < 0 and WS in err, err
    # d_log_temperature needs log_temperature, dI and dT: the message names the field
    bad = [dict(d_log_temperature=0x8000),
           dict(d_log_temperature=0x8000, dI=0x5000, dT=0x6000),
           dict(d_log_temperature=0x8000, log_temperature=0x7000),
           dict(d_log_temperature=0x8000, log_temperature=0x7000, dI=0x5000),
           dict(d_log_temperature=0x8000, log_temperature=0x7000, dT=0x6000)]
    for kw in bad:
        rc, err = _rc_err(_args(**kw))
        assert rc < 0 and "d_log_temperature" in err and WS not in err, (kw, err)
    rc, err = _rc_err(_args(d_log_temperature=0x8000, log_temperature=0x7000, dI=0x5000, dT=0x6000))
    assert rc < 0 and WS in err, err
    rc, err = _rc_err(_args(log_temperature=0x7002))
    assert rc < 0 and "4-byte aligned" in err


def test_workspace_holds_the_per_row_terms():
    """the region of the per-row terms of d loss / d theta: 16 floats per 16-row
    block of the gradient rows, behind the three N x NP matrices"""
    from mae_clip_amd import _lib as L
    lib = L.load()
    for N in (1, 3, 17, 100, 600, 2100):
        NP = (N + 15) // 16 * 16
        assert lib.maeclip_clip_loss_workspace(N, 256, N) >= 4 * (3 * N * NP + 8 * N + NP)


# --------------------------------------------------- plumbing, stubbed launches
def _train(monkeypatch, learnable, precision, steps=(8, 5)):
    from mae_clip_amd.optim import AdamW
    with stubbed_kernels(monkeypatch) as stub:
        m = _model(precision, learnable=learnable).train()
        named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
        groups = [dict(params=[p for n, p in named if n != "log_temperature"], weight_decay=1e-3)]
        if learnable:
            groups.append(dict(params=[m.log_temperature], weight_decay=0.0))
        opt = AdamW(groups, lr=1e-3, max_grad_norm=1.0)
        for B in steps:
            opt.zero_grad(set_to_none=True)
            loss = m(make_batch(B, 32))
            assert loss.shape == ()
            loss.backward()
            for n, p in named:
                assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32, n
            opt.step()
        return m, opt, list(stub.calls)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_training_step_plumbing_with_temperature(monkeypatch, precision):
    m, opt, calls = _train(monkeypatch, True, precision)
    g = m.log_temperature.grad
    assert g is not None and g.shape == (1,) and g.dtype == torch.float32
    assert calls.count("maeclip_clip_loss") == 2                 # once per forward, none in the backward
    st = opt.state[m.log_temperature]
    assert st["step"] == 2 and st["exp_avg"].shape == (1,) and st["exp_avg"].dtype == torch.float32
    from mae_clip_amd.modules import shadow_of
    assert shadow_of(m.log_temperature) is None                  # no bf16 copy of theta
    # the parameter adds no C-ABI call: its gradient comes out of the loss call and is
    # scaled in the launch that scales dI / dT; its own parameter group costs the optimizer
    # one launch more of each per-group kind per step (update, sum of squares, step counter)
    _, _, off = _train(monkeypatch, False, precision)
    for name in set(off) | set(calls):
        extra = 2 if name in ("maeclip_adamw_multi", "maeclip_sumsq_multi", "maeclip_counter_add") else 0
        assert calls.count(name) == off.count(name) + extra, name


def test_no_grad_forward_reads_the_parameter(monkeypatch):
    """CLIP.clip_loss under no_grad (the validation loop) hands the kernel the
    device theta too; with the flag off it hands it none"""
    for learnable in (True, False):
        with stubbed_kernels(monkeypatch) as stub:
            seen = []
            launch = stub.maeclip_clip_loss

            def spy(a, s, launch=launch, seen=seen):
                o = a._obj
                seen.append((o.log_temperature, o.d_log_temperature, o.dI))
                return launch(a, s)
            stub.maeclip_clip_loss = spy      # an instance attribute: found before the stub's __getattr__
            m = _model(learnable=learnable).eval()
            with torch.no_grad():
                m(make_batch(4, 32))
            m(make_batch(4, 32)).backward()
        (lt0, d0, dI0), (lt1, d1, dI1) = seen
        assert dI0 is None and dI1 is not None and d0 is None
        if learnable:
            assert lt0 == lt1 == m.log_temperature.data_ptr() and d1 is not None
        else:
            assert lt0 is None and lt1 is None and d1 is None


def test_default_launch_sequence_is_the_recorded_one():
    """Flag off: forward + backward issue exactly the launches recorded before
    this feature (tests/golden/launch_sequences.json). Flag on: the same, but
    for the one launch that scales the loss's gradients by grad_output, which
    now takes dI and dT as one tensor and d theta as the other."""
    from tests import launch_trace as LT
    with open(LT.GOLDEN) as f:
        golden = LT.unpack(json.load(f))
    for name in ("fp32_b8", "bf16_b8_mask0"):
        kw = dict(LT.CONFIGS[name])
        off = json.loads(json.dumps(LT.record(**dict(kw, cfg=dict(learnable_temperature=False)))))
        assert off == golden[name], name
        on = json.loads(json.dumps(LT.record(**dict(kw, cfg=dict(learnable_temperature=True)))))
        assert len(on) == len(off)
        diff = [(a, b) for a, b in zip(on, off) if a != b]
        assert len(diff) == 1 and diff[0][0][0] == diff[0][1][0] == "maeclip_scale_by_scalar2", diff
        a, b = diff[0]
        # (name, stream, src0, dst0, n0, src1, dst1, n1, s, w): B x 256 embeddings
        assert b[4] == b[7] == 8 * 256 and a[4] == 2 * 8 * 256 and a[7] == 1


def _dp_rank(rank, world, port, out):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mp_ = pytest.MonkeyPatch()
        with stubbed_kernels(mp_):
            from mae_clip_amd.distributed import DataParallel
            m = _model("bf16").train()
            dp = DataParallel(m, bucket_mb=0.5)
            th = m.log_temperature
            for _ in range(2):
                for p in m.parameters():
                    p.grad = None
                dp.reset_stats()
                m(make_batch(4, 32, seed=rank)).backward()
                dp.sync_gradients()
            off, n, shape = dp.arena.offsets[id(th)]
            out[rank] = dict(slot=(off % 4, n, shape), bucket=id(th) in dp._bucket_of,
                             in_bucket=any(p is th for b in dp.buckets for p in b), owned=dp.arena.owns(th),
                             adopted=dp.adopted, nparams=len(dp.params), grad_shape=tuple(th.grad.shape))
        mp_.undo()
    finally:
        dist.destroy_process_group()


def test_data_parallel_arena_holds_the_temperature():
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_dp_rank, args=(2, _free_port(), out), nprocs=2, join=True)
    for r in range(2):
        o = out[r]
        assert o["slot"] == (0, 1, (1,)) and o["bucket"] and o["in_bucket"]
        assert o["owned"] and o["grad_shape"] == (1,)
        assert o["adopted"] == o["nparams"], (o["adopted"], o["nparams"])
