"""Argument rejections of the Mixup / CutMix entry points on the real library
(the pattern of test_augment_args_cpu.py) and of their Python wrappers. No GPU
is needed: every check comes before any launch, so the host pointers handed in
are never dereferenced on a device; a call that got past its checks would fail
with "launch failed" (-2), which is why each case also looks at the message.
Also here: the struct mirrors, the config flags, Chain."""
import ctypes
import os
import re

import pytest
import torch

from mae_clip_amd import _lib as L
from tests.helpers import product_config

_BUF = (ctypes.c_int32 * 4096)()
PTR = ctypes.cast(_BUF, ctypes.c_void_p).value       # 16-byte aligned or not: the checks below do not depend on it


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _rejected(lib, rc, what):
    msg = lib.maeclip_last_error()
    assert rc == -1, (rc, msg)
    assert what in msg and b"launch failed" not in msg, msg


def _params_args(**kw):
    f = dict(params=PTR, B=2, H=32, W=32, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode=0, seed=1)
    f.update(kw)
    return L.MixParamsArgs(**f)


PARAMS_REJECTS = {
    "no params": (dict(params=None), b"null pointer"),
    "B < 0": (dict(B=-1), b"B must be >= 0"),
    "H = 0": (dict(H=0), b"H and W must be in [1, 32768]"),
    "W too large": (dict(W=32769), b"H and W must be in [1, 32768]"),
    "alpha < 0": (dict(mixup_alpha=-0.1), b"alphas must be finite and >= 0"),
    "alpha inf": (dict(cutmix_alpha=float("inf")), b"alphas must be finite and >= 0"),
    "alpha nan": (dict(cutmix_alpha=float("nan")), b"alphas must be finite and >= 0"),
    "prob > 1": (dict(prob=1.5), b"prob must be in [0, 1]"),
    "switch_prob < 0": (dict(switch_prob=-0.5), b"switch_prob must be in [0, 1]"),
    "mode 2": (dict(mode=2), b"mode must be 0 (batch) or 1 (elem)"),
    "misaligned params": (dict(params=PTR + 2), b"params must be 4-byte aligned"),
}


@pytest.mark.parametrize("case", sorted(PARAMS_REJECTS))
def test_mix_params_rejects(lib, case):
    """the device entry point and its host twin share one set of checks, each under its own name"""
    kw, what = PARAMS_REJECTS[case]
    a = _params_args(**kw)
    _rejected(lib, lib.maeclip_mix_params(ctypes.byref(a), None), b"maeclip_mix_params: " + what)
    _rejected(lib, lib.maeclip_mix_params_host(ctypes.byref(a)), b"maeclip_mix_params_host: " + what)


def _images_args(**kw):
    # B = 2, S = 8, uint8: 384 bytes a side; dst right behind src
    f = dict(src=PTR, dst=PTR + 384, params=PTR + 8192, B=2, S=8, dtype=0)
    f.update(kw)
    return L.MixImagesArgs(**f)


IMAGES_REJECTS = {
    "no src": (dict(src=None), b"null pointer"),
    "no dst": (dict(dst=None), b"null pointer"),
    "no params": (dict(params=None), b"null pointer"),
    "dtype 2": (dict(dtype=2), b"dtype must be 0 (uint8 HWC) or 1 (fp32 CHW)"),
    "S = 0": (dict(S=0), b"bad sizes"),
    "S > 8192": (dict(S=8193), b"bad sizes"),
    "B < 0": (dict(B=-1), b"bad sizes"),
    "in place": (dict(dst=PTR), b"dst overlaps src"),
    "dst inside src": (dict(dst=PTR + 383), b"dst overlaps src"),
    "src inside dst": (dict(src=PTR + 384, dst=PTR + 1), b"dst overlaps src"),
    "fp32 overlap by one element": (dict(dtype=1, dst=PTR + 4 * 383), b"dst overlaps src"),
    "fp32 misaligned": (dict(dtype=1, src=PTR + 2, dst=PTR + 4096), b"params and fp32 images must be 4-byte aligned"),
}


@pytest.mark.parametrize("case", sorted(IMAGES_REJECTS))
def test_mix_images_rejects(lib, case):
    kw, what = IMAGES_REJECTS[case]
    a = _images_args(**kw)
    _rejected(lib, lib.maeclip_mix_images(ctypes.byref(a), None), b"maeclip_mix_images: " + what)


def _targets_args(**kw):
    f = dict(labels=PTR, label_dtype=1, params=PTR + 64, targets=PTR + 1024, ld_t=12, B=2, C=10)
    f.update(kw)
    return L.MixTargetsArgs(**f)


TARGETS_REJECTS = {
    "no labels": (dict(labels=None), b"null pointer"),
    "no targets": (dict(targets=None), b"null pointer"),
    "label_dtype 2": (dict(label_dtype=2), b"label_dtype must be 0 (int32) or 1 (int64)"),
    "C = 0": (dict(C=0), b"C must be in [1, 2^31)"),
    "B < 0": (dict(B=-1), b"B must be in [0, 2^31)"),
    "ld_t < C": (dict(ld_t=9), b"ld_t must be >= C"),
    "int64 labels at 4 bytes": (dict(labels=PTR + 4 if PTR % 8 == 0 else PTR),
                                b"float / int32 pointers must be 4-byte aligned, int64 labels 8-byte aligned"),
    "targets misaligned": (dict(targets=PTR + 1022), b"float / int32 pointers must be 4-byte aligned"),
}


@pytest.mark.parametrize("case", sorted(TARGETS_REJECTS))
def test_mix_targets_rejects(lib, case):
    kw, what = TARGETS_REJECTS[case]
    a = _targets_args(**kw)
    _rejected(lib, lib.maeclip_mix_targets(ctypes.byref(a), None), b"maeclip_mix_targets: " + what)


def test_null_args(lib):
    _rejected(lib, lib.maeclip_mix_params(None, None), b"maeclip_mix_params: null pointer")
    _rejected(lib, lib.maeclip_mix_params_host(None), b"maeclip_mix_params_host: null pointer")
    _rejected(lib, lib.maeclip_mix_images(None, None), b"maeclip_mix_images: null pointer")
    _rejected(lib, lib.maeclip_mix_targets(None, None), b"maeclip_mix_targets: null pointer")


def test_empty_batch_launches_nothing(lib):
    a = _params_args(B=0)
    assert lib.maeclip_mix_params(ctypes.byref(a), None) == 0 and lib.maeclip_mix_params_host(ctypes.byref(a)) == 0
    b = _images_args(B=0, dst=PTR)                     # nothing to overlap
    assert lib.maeclip_mix_images(ctypes.byref(b), None) == 0
    c = _targets_args(B=0)
    assert lib.maeclip_mix_targets(ctypes.byref(c), None) == 0


def test_struct_mirrors_match_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "maeclip.h")).read()
    for cname, n_py in (("maeclip_mix_params_args", len(L.MixParamsArgs._fields_)),
                        ("maeclip_mix_images_args", len(L.MixImagesArgs._fields_)),
                        ("maeclip_mix_targets_args", len(L.MixTargetsArgs._fields_)), ("maeclip_mix_record", 8)):
        body = re.search(r"typedef struct \{([^{}]*)\}\s*" + cname + ";", src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        n = sum(len(d.split(",")) for d in body.split(";") if d.strip())
        assert n == n_py, (cname, n, n_py)
    assert ctypes.sizeof(L.MixParamsArgs) == 64 and ctypes.sizeof(L.MixImagesArgs) == 48
    assert ctypes.sizeof(L.MixTargetsArgs) == 56
    assert re.search(r"#define MAECLIP_ABI_VERSION 14\b", src) and L.ABI_VERSION == 14      # additive: the ABI stays


def test_python_wrappers_check_forms_and_refuse_cpu_tensors():
    """wrong dtypes / shapes are ValueErrors; right forms on the CPU are refused (no CPU fallback)"""
    from mae_clip_amd import data
    rec = torch.zeros((2, 8), dtype=torch.int32)
    u8 = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    f32 = torch.zeros((2, 3, 8, 8), dtype=torch.float32)
    y = torch.zeros(2, dtype=torch.int64)
    for bad in (torch.zeros((2, 8, 8, 3), dtype=torch.int8), torch.zeros((2, 8, 8, 3), dtype=torch.float32),
                torch.zeros((2, 3, 8, 8), dtype=torch.uint8), torch.zeros((2, 8, 6, 3), dtype=torch.uint8),
                torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((2, 3, 8, 8), dtype=torch.float64),
                f32.permute(0, 1, 3, 2)[:, :, ::2]):
        with pytest.raises(ValueError, match="images must be"):
            data.mix_images(bad, rec)
    for bad in (rec.float(), torch.zeros((2, 5), dtype=torch.int32), torch.zeros((3, 8), dtype=torch.int32), None):
        with pytest.raises(ValueError, match="params must be"):
            data.mix_images(u8, bad)
        with pytest.raises(ValueError, match="params must be"):
            data.mix_targets(y, bad, 10)
    with pytest.raises(ValueError, match="out must be"):
        data.mix_images(u8, rec, out=f32)
    with pytest.raises(ValueError, match="labels must be"):
        data.mix_targets(y.float(), rec, 10)
    with pytest.raises(ValueError, match="ld_t >= C"):
        data.mix_targets(y, rec, 10, out=torch.zeros((2, 9)))
    with pytest.raises(ValueError, match="ld_t >= C"):
        data.mix_targets(y, rec, 10, out=torch.zeros((2, 24))[:, :12])
    with pytest.raises(ValueError, match="mode must be"):
        data.mix_params_host(2, 8, 8, mode="pair")
    with pytest.raises(L.MaeClipNativeError):
        data.mix_images(u8, rec)
    with pytest.raises(L.MaeClipNativeError):
        data.mix_images(f32, rec, out=torch.zeros_like(f32))
    with pytest.raises(L.MaeClipNativeError):
        data.mix_targets(y, rec, 10)
    with pytest.raises(L.MaeClipNativeError):
        data.mix_params(2, 8, 8, device="cpu")
    with pytest.raises(L.MaeClipNativeError):
        data.mix_params(2, 8, 8, step_ptr=torch.zeros(1, dtype=torch.int64))


def test_config_flags_and_helper():
    from mae_clip_amd import config as CFG, data
    assert (CFG.mixup_alpha, CFG.cutmix_alpha, CFG.mix_prob, CFG.mix_switch_prob, CFG.mix_mode) == (0.0, 0.0, 1.0, 0.5, "batch")
    assert data.mix_augment_from_config() is None                      # off by default
    with product_config(mixup_alpha=0.8, cutmix_alpha=1.0, mix_prob=0.9, mix_switch_prob=0.25, mix_mode="elem",
                        mix_seed=11, num_classes=7):
        m = data.mix_augment_from_config()
        assert data.MixAugment(3).seed == 11
    assert (m.num_classes, m.mixup_alpha, m.cutmix_alpha, m.prob, m.switch_prob, m.mode, m.seed) == \
        (7, 0.8, 1.0, 0.9, 0.25, L.MIX_ELEM, 11)
    with product_config(cutmix_alpha=1.0):
        assert data.mix_augment_from_config().mixup_alpha == 0.0
    with pytest.raises(ValueError, match="mode must be"):
        data.MixAugment(10, mode="pair")
    with pytest.raises(ValueError, match="num_classes"):
        data.MixAugment(0)


def test_chain_applies_in_order_with_one_contract():
    from mae_clip_amd import data
    seen = []

    def t(tag):
        def f(batch, step_ptr, sample_offset=0):
            seen.append((tag, step_ptr, sample_offset, batch["image"]))
            return {**batch, "image": batch["image"] + [tag]}
        return f

    out = data.Chain(t("a"), None, t("b"))({"image": [], "label": 5}, "ctr", 16)
    assert out == {"image": ["a", "b"], "label": 5}
    assert seen == [("a", "ctr", 16, []), ("b", "ctr", 16, ["a"])]
    assert data.Chain()({"image": 1}, None) == {"image": 1}
