"""Argument rejections of the augmentation entry points on the real library
(the pattern of test_rowwise_args_cpu.py). No GPU is needed: every check comes
before any launch, so the host pointers handed in are never dereferenced on a
device; a call that got past its checks would fail with "launch failed" (-2),
which is why each case also looks at the message. The kernels themselves are
compared with the CPU restatement in test_augment_gpu.py."""
import ctypes

import pytest

from mae_clip_amd import _lib as L

_BUF = (ctypes.c_int32 * 64)()
PTR = ctypes.cast(_BUF, ctypes.c_void_p).value
F2 = ctypes.c_float * 2
F3 = ctypes.c_float * 3


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _rejected(lib, rc, what):
    msg = lib.maeclip_last_error()
    assert rc == -1, (rc, msg)
    assert what in msg and b"launch failed" not in msg, msg


def _augment_args(**kw):
    f = dict(batch=PTR, Hmax=8, Wmax=8, boxes=PTR, dst_u8=PTR, B=2, S=8, mean=F3(0.5, 0.5, 0.5),
             std=F3(0.25, 0.25, 0.25), max_pixel=255.0)
    f.update(kw)
    return L.AugmentArgs(**f)


def _crop_args(**kw):
    f = dict(H=32, W=32, boxes=PTR, B=2, scale=F2(0.08, 1.0), ratio=F2(0.75, 4 / 3), flip_p=0.5, seed=1)
    f.update(kw)
    return L.CropParamsArgs(**f)


AUGMENT_REJECTS = {
    "no boxes": (dict(boxes=None), b"null pointer"),
    "S = 0": (dict(S=0), b"bad sizes"),
    "S > 8192": (dict(S=8193), b"bad sizes"),
    "B > 65535": (dict(B=65536), b"bad sizes"),
    "B < 0": (dict(B=-1), b"bad sizes"),
    "no source": (dict(batch=None), b"exactly one source"),
    "both sources": (dict(images=PTR), b"exactly one source"),
    "empty slot": (dict(Hmax=0), b"bad batch slot size"),
    "no destination": (dict(dst_u8=None), b"no destination"),
    "std = 0": (dict(std=F3(0.25, 0.0, 0.25)), b"std and max_pixel must be > 0"),
    "max_pixel = 0": (dict(max_pixel=0.0), b"std and max_pixel must be > 0"),
}


@pytest.mark.parametrize("case", sorted(AUGMENT_REJECTS))
def test_augment_rejects(lib, case):
    kw, what = AUGMENT_REJECTS[case]
    a = _augment_args(**kw)
    _rejected(lib, lib.maeclip_image_augment_u8(ctypes.byref(a), None), b"maeclip_image_augment_u8: " + what)


def test_augment_rejects_null_args(lib):
    _rejected(lib, lib.maeclip_image_augment_u8(None, None), b"maeclip_image_augment_u8: null pointer")


CROP_REJECTS = {
    "no boxes": (dict(boxes=None), b"null pointer"),
    "B < 0": (dict(B=-1), b"B must be >= 0"),
    "no sizes": (dict(H=0), b"needs image descriptors or H, W > 0"),
    "s0 = 0": (dict(scale=F2(0.0, 1.0)), b"scale must satisfy"),
    "s0 > s1": (dict(scale=F2(0.5, 0.25)), b"scale must satisfy"),
    "s1 > 1": (dict(scale=F2(0.5, 1.5)), b"scale must satisfy"),
    "scale nan": (dict(scale=F2(float("nan"), 1.0)), b"scale must satisfy"),
    "r0 = 0": (dict(ratio=F2(0.0, 1.0)), b"ratio must satisfy"),
    "r0 > r1": (dict(ratio=F2(2.0, 1.0)), b"ratio must satisfy"),
    "r1 = inf": (dict(ratio=F2(1.0, float("inf"))), b"ratio must satisfy"),
    "flip_p < 0": (dict(flip_p=-0.1), b"flip_p must be in [0, 1]"),
    "flip_p > 1": (dict(flip_p=1.5), b"flip_p must be in [0, 1]"),
}


@pytest.mark.parametrize("case", sorted(CROP_REJECTS))
def test_crop_params_rejects(lib, case):
    """the device entry point and its host twin share one set of checks, each under its own name"""
    kw, what = CROP_REJECTS[case]
    a = _crop_args(**kw)
    _rejected(lib, lib.maeclip_crop_params(ctypes.byref(a), None), b"maeclip_crop_params: " + what)
    _rejected(lib, lib.maeclip_crop_params_host(ctypes.byref(a)), b"maeclip_crop_params_host: " + what)


def test_struct_field_counts_match_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "maeclip.h")).read()
    for cname, py in (("maeclip_crop_params_args", L.CropParamsArgs), ("maeclip_augment_args", L.AugmentArgs)):
        body = re.search(r"typedef struct \{([^{}]*)\}\s*" + cname + ";", src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        n = sum(len(d.split(",")) for d in body.split(";") if d.strip())
        assert n == len(py._fields_), (cname, n, len(py._fields_))


def test_python_wrappers_refuse_cpu_tensors():
    """no CPU fallback: the wrappers raise before any library call"""
    import torch
    from mae_clip_amd import data
    batch = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(L.MaeClipNativeError):
        data.crop_params(batch)
    with pytest.raises(L.MaeClipNativeError):
        data.augment_images(batch, torch.zeros((2, 5), dtype=torch.int32), 8)
