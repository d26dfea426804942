"""Host plumbing of AdamW(max_grad_norm=..., device_lr=True) with every kernel
launch stubbed (tests/test_plumbing_cpu.py's stub library): which launches a
training step issues and in which order, when the learning rate is pushed to
the device, and that the defaults issue none of the new launches. The argument
validation of the new entry points runs on the real library (no GPU needed:
the checks come before any launch). The real-kernel versions are in
test_optim_schedule_gpu.py."""
import ctypes

import pytest
import torch

from tests.helpers import make_batch
from tests.test_plumbing_cpu import stubbed_kernels, _model

NEW = ("maeclip_sumsq_multi", "maeclip_clip_coef", "maeclip_store_f32")


def _train_step(m, opt, B=8):
    opt.zero_grad(set_to_none=True)
    m(make_batch(B, 32)).backward()
    opt.step()


def test_clip_and_device_lr_launch_sequence(monkeypatch):
    from mae_clip_amd.optim import AdamW
    with stubbed_kernels(monkeypatch) as stub:
        m = _model("fp32").train()
        opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3, max_grad_norm=1.0,
                    device_lr=True)
        _train_step(m, opt)
        for name in NEW:
            assert name in stub.calls, name
        first_adamw = stub.calls.index("maeclip_adamw_multi")
        assert stub.calls.index("maeclip_sumsq_multi") < stub.calls.index("maeclip_clip_coef") < first_adamw
        # one group: one sumsq, one coefficient, one AdamW launch per step
        assert stub.calls.count("maeclip_sumsq_multi") == stub.calls.count("maeclip_clip_coef") == 1
        assert stub.calls.count("maeclip_store_f32") == 1
        assert opt.grad_norm.shape == opt.clip_coef.shape == (1,)
        storage = (opt.grad_norm.data_ptr(), opt.clip_coef.data_ptr())
        # unchanged lr: nothing is pushed again
        _train_step(m, opt)
        assert stub.calls.count("maeclip_store_f32") == 1
        assert stub.calls.count("maeclip_clip_coef") == 2
        # a scheduler's edit of group["lr"]: exactly one more store
        opt.param_groups[0]["lr"] *= 0.5
        _train_step(m, opt)
        assert stub.calls.count("maeclip_store_f32") == 2
        _train_step(m, opt)
        assert stub.calls.count("maeclip_store_f32") == 2
        assert storage == (opt.grad_norm.data_ptr(), opt.clip_coef.data_ptr())
        # group["lr"] stays the Python float schedulers and state_dict see
        assert opt.param_groups[0]["lr"] == 5e-4 and opt.state_dict()["param_groups"][0]["lr"] == 5e-4


def test_norm_is_global_over_parameter_groups(monkeypatch):
    """two groups: both are summed before the first update, one coefficient"""
    from mae_clip_amd.optim import AdamW
    with stubbed_kernels(monkeypatch) as stub:
        m = _model("fp32").train()
        ps = [p for p in m.parameters() if p.requires_grad]
        opt = AdamW([{"params": ps[:5], "lr": 1e-3}, {"params": ps[5:], "lr": 2e-3}], weight_decay=1e-3,
                    max_grad_norm=1.0, device_lr=True)
        _train_step(m, opt)
        seq = [c for c in stub.calls if c in NEW or c == "maeclip_adamw_multi"]
        assert seq == ["maeclip_store_f32", "maeclip_sumsq_multi", "maeclip_sumsq_multi", "maeclip_clip_coef",
                       "maeclip_adamw_multi", "maeclip_adamw_multi"], seq
        assert opt._lr_dev.shape == (2,)


def test_defaults_issue_none_of_the_new_launches(monkeypatch):
    from mae_clip_amd.optim import AdamW
    with stubbed_kernels(monkeypatch) as stub:
        m = _model("fp32").train()
        opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3)
        _train_step(m, opt)
        opt.param_groups[0]["lr"] *= 0.5
        _train_step(m, opt)
        assert "maeclip_adamw_multi" in stub.calls
        for name in NEW:
            assert name not in stub.calls, name
        assert opt.grad_norm is None and opt.clip_coef is None
        opt.push_lr()   # a no-op without device_lr
        assert "maeclip_store_f32" not in stub.calls


def test_max_grad_norm_must_be_positive():
    from mae_clip_amd.optim import AdamW
    p = torch.nn.Parameter(torch.zeros(4))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            AdamW([p], max_grad_norm=bad)


def test_new_entry_points_validate_arguments():
    from mae_clip_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_float * 40)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    # the checks come before any launch: the pointers are never dereferenced on a device
    assert lib.maeclip_store_f32(ptr, buf, 33, None) < 0
    assert b"maeclip_store_f32" in lib.maeclip_last_error()
    assert lib.maeclip_store_f32(ptr, buf, 0, None) < 0
    assert lib.maeclip_store_f32(None, buf, 4, None) < 0
    assert b"maeclip_store_f32" in lib.maeclip_last_error()
    assert lib.maeclip_clip_coef(ptr, 4, 0.0, ptr, ptr, None) < 0
    assert b"max_norm" in lib.maeclip_last_error()
    assert lib.maeclip_clip_coef(ptr, 4, -1.0, ptr, ptr, None) < 0
    for args in ((None, 4, 1.0, ptr, ptr), (ptr, 4, 1.0, None, ptr), (ptr, 4, 1.0, ptr, None)):
        assert lib.maeclip_clip_coef(*args, None) < 0
        assert b"maeclip_clip_coef" in lib.maeclip_last_error()
    e = (L.MtEntry * 1)()
    e[0].n = 16
    assert lib.maeclip_sumsq_multi(ptr, e, 0, ptr, 0, None) < 0
    assert b"maeclip_sumsq_multi" in lib.maeclip_last_error()
    assert lib.maeclip_sumsq_multi(None, e, 1, ptr, 0, None) < 0
    assert lib.maeclip_sumsq_multi(ptr, e, 1, None, 0, None) < 0
    # lr_ptr without the device step count cannot derive the step size
    hp = L.AdamwHparams(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step_size=1e-2, bc2_sqrt=0.03, grad_scale=1.0,
                        lr_ptr=ptr.value)
    assert lib.maeclip_adamw_multi(ptr, e, 1, ctypes.byref(hp), None) < 0
    assert b"lr_ptr" in lib.maeclip_last_error()
