"""Argument rejections of the drop-path entry points on the real library (the
pattern of test_mix_args_cpu.py) and of the public interface. No GPU is
needed: every check comes before any launch, so the host pointers handed in
are never dereferenced on a device; a call that got past its checks would fail
with "launch failed" (-2), which is why each case also looks at the message."""
import ctypes

import pytest
import torch

from mae_clip_amd import _lib as L
from tests.helpers import product_config, C0

_BUF = (ctypes.c_float * 8192)()
PTR = (ctypes.cast(_BUF, ctypes.c_void_p).value + 15) & ~15      # 16-byte aligned
M, D, N = 6, 64, 3                                               # 6 x 64 floats = 1536 bytes a tensor


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _rejected(lib, rc, what):
    msg = lib.maeclip_last_error()
    assert rc == -1, (rc, msg)
    assert what in msg and b"launch failed" not in msg, msg


def _fwd_args(**kw):
    f = dict(resid=PTR, ld_resid=D, branch=PTR + 2048, ld_branch=D, out=PTR + 4096, ld_out=D, M=M, D=D, n=N, p=0.1, k=3,
             seed=1)
    f.update(kw)
    return L.DropPathArgs(**f)


def _bwd_args(**kw):
    f = dict(g=PTR, ld_g=D, gs=PTR + 2048, ld_gs=D, gs_dtype=L.BF16, partial=PTR + 4096, M=M, D=D, n=N, p=0.1, k=3, seed=1)
    f.update(kw)
    return L.DropPathArgs(**f)


COMMON_REJECTS = {
    "p < 0": (dict(p=-0.1), b"p must be in [0, 1)"),
    "p = 1": (dict(p=1.0), b"p must be in [0, 1)"),
    "p nan": (dict(p=float("nan")), b"p must be in [0, 1)"),
    "n = 0": (dict(n=0), b"n must be in [1, 2^31)"),
    "n < 0": (dict(n=-3), b"n must be in [1, 2^31)"),
    "M not a multiple of n": (dict(n=4), b"M (6) must be a multiple of n (4)"),
    "M < 0": (dict(M=-3), b"M must be in [0, 2^31 - 256)"),
    "D % 4": (dict(D=62), b"D must be a positive multiple of 4"),
    "D = 0": (dict(D=0), b"D must be a positive multiple of 4"),
    "k < 0": (dict(k=-1), b"k must be >= 0"),
    "misaligned step_ptr": (dict(step_ptr=PTR + 4), b"step_ptr must be 8-byte aligned"),
}
FWD_REJECTS = dict(COMMON_REJECTS, **{
    "no resid": (dict(resid=None), b"null pointer"),
    "no branch": (dict(branch=None), b"null pointer"),
    "no out": (dict(out=None), b"null pointer"),
    "misaligned out": (dict(out=PTR + 4096 + 4), b"out must be 16-byte aligned"),
    "stride < D": (dict(ld_branch=D - 4), b"branch must be 16-byte aligned with a row stride >= D"),
    "stride % 4": (dict(ld_resid=D + 2), b"resid must be 16-byte aligned with a row stride >= D"),
    "out is resid": (dict(out=PTR), b"out overlaps resid"),
    "out inside resid": (dict(out=PTR + 1520), b"out overlaps resid"),
    "out inside branch": (dict(out=PTR + 2048 + 256), b"out overlaps branch without being branch"),
    "in place with another stride": (dict(out=PTR + 2048, ld_branch=D + 4), b"out overlaps branch without being branch"),
})
BWD_REJECTS = dict(COMMON_REJECTS, **{
    "no g": (dict(g=None), b"null pointer"),
    "no gs": (dict(gs=None), b"null pointer"),
    "no partial": (dict(partial=None), b"null pointer"),
    "dtype 2": (dict(gs_dtype=2), b"gs_dtype must be 0 (fp32) or 1 (bf16)"),
    "D > 2048": (dict(D=2052, ld_g=2052, ld_gs=2052), b"D must be <= 2048"),
    "misaligned fp32 gs": (dict(gs_dtype=L.F32, gs=PTR + 2048 + 8), b"gs must be 16-byte aligned"),
    "misaligned bf16 gs": (dict(gs=PTR + 2048 + 4), b"gs must be 8-byte aligned"),
    "gs is g": (dict(gs_dtype=L.F32, gs=PTR), b"g, gs and partial must not overlap"),
    "partial inside g": (dict(partial=PTR + 1024), b"g, gs and partial must not overlap"),
})


@pytest.mark.parametrize("case", sorted(FWD_REJECTS))
def test_droppath_fwd_rejects(lib, case):
    kw, what = FWD_REJECTS[case]
    a = _fwd_args(**kw)
    _rejected(lib, lib.maeclip_droppath_fwd(ctypes.byref(a), None), b"maeclip_droppath_fwd: " + what)


@pytest.mark.parametrize("case", sorted(BWD_REJECTS))
def test_droppath_bwd_rejects(lib, case):
    kw, what = BWD_REJECTS[case]
    a = _bwd_args(**kw)
    _rejected(lib, lib.maeclip_droppath_bwd(ctypes.byref(a), None), b"maeclip_droppath_bwd: " + what)


def test_null_args_struct(lib):
    _rejected(lib, lib.maeclip_droppath_fwd(None, None), b"maeclip_droppath_fwd: null pointer")
    _rejected(lib, lib.maeclip_droppath_bwd(None, None), b"maeclip_droppath_bwd: null pointer")


def test_scales_host_rejects(lib):
    keys = (ctypes.c_int32 * 1)(0)
    out = (ctypes.c_float * 4)()
    host = lib.maeclip_droppath_scales_host
    _rejected(lib, host(None, 4, ctypes.addressof(keys), 1, 0.1, 0, 0, None), b"maeclip_droppath_scales_host: null pointer")
    _rejected(lib, host(ctypes.addressof(out), 4, None, 1, 0.1, 0, 0, None), b"maeclip_droppath_scales_host: null pointer")
    _rejected(lib, host(ctypes.addressof(out), 4, ctypes.addressof(keys), 1, 1.0, 0, 0, None), b"p must be in [0, 1)")
    _rejected(lib, host(ctypes.addressof(out), -1, ctypes.addressof(keys), 1, 0.1, 0, 0, None), b"B and nk must be >= 0")
    _rejected(lib, host(ctypes.addressof(out), 4, ctypes.addressof(keys), 0, 1.0, 0, 0, None), b"p must be in [0, 1)")   # no key
    bad = (ctypes.c_int32 * 2)(0, -1)
    _rejected(lib, host(ctypes.addressof(out), 2, ctypes.addressof(bad), 2, 0.1, 0, 0, None), b"k must be >= 0")
    assert host(ctypes.addressof(out), 4, ctypes.addressof(keys), 1, 0.1, 0, 0, None) == 0      # step NULL: step 0


def test_partial_rows(lib):
    for m in (0, 1, 63, 64, 65, 400, 50432):
        assert lib.maeclip_droppath_partial_rows(m) == -(-m // 64)


def test_empty_call_is_accepted(lib):
    assert lib.maeclip_droppath_fwd(ctypes.byref(_fwd_args(M=0)), None) == 0
    assert lib.maeclip_droppath_bwd(ctypes.byref(_bwd_args(M=0)), None) == 0


def test_wrappers_refuse_cpu_tensors():
    from mae_clip_amd import kernels as K
    x = torch.zeros(6, 64)
    with pytest.raises(L.MaeClipNativeError):
        K.droppath_fwd(x, x.clone(), 3, 0.1, 0)
    with pytest.raises(L.MaeClipNativeError):
        K.droppath_bwd(x, 3, 0.1, 0, torch.bfloat16)


# ------------------------------------------------------------- public interface
_KW = {k: v for k, v in C0.items() if k != "batch_size"}


def test_config_default_is_off():
    from mae_clip_amd import config as CFG
    from mae_clip_amd.modules import ImageEncoder
    assert CFG.drop_path_rate == 0.0
    with product_config(**_KW):
        assert ImageEncoder().model.drop_path_rate == 0.0
        assert ImageEncoder(drop_path_rate=0.2).model.drop_path_rate == 0.2
    with product_config(drop_path_rate=0.1, **_KW):
        assert ImageEncoder().model.drop_path_rate == 0.1


def test_probe_with_drop_path_raises():
    from mae_clip_amd.classifier import ClassifierModel
    with product_config(**_KW):
        with pytest.raises(ValueError, match="trainable_encoder"):
            ClassifierModel(num_classes=10, trainable_encoder=False, drop_path_rate=0.1)
        m = ClassifierModel(num_classes=10, trainable_encoder=True, drop_path_rate=0.1)
        assert m.image_encoder.model.drop_path_rate == pytest.approx(0.1)
        assert ClassifierModel(num_classes=10, trainable_encoder=False, drop_path_rate=0.0).image_encoder.model.drop_path_rate == 0


@pytest.mark.parametrize("rate", [-0.1, 1.0])
def test_rate_out_of_range_raises(rate):
    from mae_clip_amd.modules import ImageEncoder
    with product_config(**_KW):
        with pytest.raises(ValueError, match="drop_path_rate"):
            ImageEncoder(drop_path_rate=rate)


def test_fp8_with_drop_path_raises(monkeypatch):
    from mae_clip_amd.classifier import ClassifierModel
    from mae_clip_amd import modules as Mo
    from tests.test_plumbing_cpu import stubbed_kernels
    with product_config(precision="fp8", **_KW):
        with pytest.raises(ValueError, match="fp8"):
            ClassifierModel(num_classes=10, trainable_encoder=True, drop_path_rate=0.1)
        ClassifierModel(num_classes=10, trainable_encoder=True)          # rate 0: fp8 as before
    # and run_stack, where a stack's fp8 operands meet its rates, before anything is launched
    with stubbed_kernels(monkeypatch) as stub:
        blocks = torch.nn.ModuleList([Mo.Block(64, 2) for _ in range(2)])
        cache = Mo.WeightCache(fp8=True)
        for blk in blocks:
            for w in blk.gemm_weights():
                cache.register(w, w.shape)
                cache.register_fp8(w)
        cache.refresh(torch.bfloat16)
        n0 = len(stub.calls)
        with pytest.raises(ValueError, match="fp8"):
            Mo.run_stack(blocks, torch.zeros(4, 64, 64), 2, torch.bfloat16, cache, drop_path=[0.0, 0.5])
        assert len(stub.calls) == n0


def test_width_past_the_backward_kernel_raises_at_construction(monkeypatch):
    """maeclip_droppath_bwd takes rows of at most 2048 columns: a wider encoder with a
    rate > 0 fails when it is built, not at its first backward"""
    from mae_clip_amd import kernels as K, modules as Mo
    assert K.DROPPATH_MAX_D == 2048
    monkeypatch.setitem(Mo.VIT_SPECS, "vit_wide_test", (2304, 1, 36, 16, 32))
    with product_config(**dict(_KW, model_name="vit_wide_test")):
        with pytest.raises(ValueError, match="embed_dim <= 2048"):
            Mo.VisionTransformer("vit_wide_test", 32, drop_path_rate=0.1)
        assert Mo.VisionTransformer("vit_wide_test", 32).drop_path_rate == 0.0
