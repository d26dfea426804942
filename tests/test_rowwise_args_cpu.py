"""Argument rejections of the row-wise and multi-tensor entry points on the
real library. No GPU is needed: every check comes before any launch, so the
(host) pointers handed in are never dereferenced on a device. A call that got
past its checks would fail differently ("launch failed", return -2), which is
why each case also looks at the message. The kernels themselves are compared
with fp64 references in test_rowwise_kernels_gpu.py."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from mae_clip_amd import _lib as L
    return L.load()


_BUF = (ctypes.c_float * 64)()


@pytest.fixture(scope="module")
def ptr():
    return ctypes.cast(_BUF, ctypes.c_void_p)


def _rejected(lib, rc, what):
    msg = lib.maeclip_last_error()
    assert rc == -1, (rc, msg)
    assert what in msg and b"launch failed" not in msg, msg


def _ln_fwd_args(ptr, M, D):
    from mae_clip_amd import _lib as L
    return L.LnFwdArgs(x=ptr.value, x_dtype=L.F32, gamma=ptr.value, beta=ptr.value, y=ptr.value, y_dtype=L.F32,
                       M=M, D=D, ldx=D, ldy=D, eps=1e-6)


def _ln_bwd_args(ptr, M, D, **kw):
    from mae_clip_amd import _lib as L
    return L.LnBwdArgs(dy=ptr.value, dy_dtype=L.F32, x=ptr.value, x_dtype=L.F32, mean=ptr.value, rstd=ptr.value,
                       gamma=ptr.value, dx=ptr.value, M=M, D=D, ldx=D, lddy=D, lddx=D, **kw)


@pytest.mark.parametrize("D", [6, 2052, 0])
def test_ln_rejects_unsupported_row_length(lib, ptr, D):
    """D must be a multiple of 4 in (0, 2048]"""
    a = _ln_fwd_args(ptr, 4, D)
    _rejected(lib, lib.maeclip_ln_fwd(ctypes.byref(a), None), b"maeclip_ln_fwd: D=")
    b = _ln_bwd_args(ptr, 4, D)
    _rejected(lib, lib.maeclip_ln_bwd(ctypes.byref(b), None), b"maeclip_ln_bwd: D unsupported")


def test_ln_rejects_null_pointers(lib, ptr):
    a = _ln_fwd_args(ptr, 4, 8)
    a.gamma = None
    _rejected(lib, lib.maeclip_ln_fwd(ctypes.byref(a), None), b"maeclip_ln_fwd: null pointer")
    b = _ln_bwd_args(ptr, 4, 8)
    b.rstd = None
    _rejected(lib, lib.maeclip_ln_bwd(ctypes.byref(b), None), b"maeclip_ln_bwd: null pointer")


def test_ln_bwd_rejects_bad_pool_arguments(lib, ptr):
    cases = {
        "dres_pool together with dres": dict(M=12, dres_pool=ptr.value, pool_n=4, dres=ptr.value),
        "pool_n not dividing M": dict(M=10, dres_pool=ptr.value, pool_n=4),
        "pool_n = 1": dict(M=12, dres_pool=ptr.value, pool_n=1),
        "pool_n = 0": dict(M=12, dres_pool=ptr.value, pool_n=0),
    }
    for name, kw in cases.items():
        M = kw.pop("M")
        b = _ln_bwd_args(ptr, M, 8, **kw)
        rc = lib.maeclip_ln_bwd(ctypes.byref(b), None)
        assert rc == -1 and b"dres_pool" in lib.maeclip_last_error(), (name, rc, lib.maeclip_last_error())


def test_pool_rejects_a_lone_prefix_token(lib, ptr):
    """n = 1 leaves no token to average (the mean divides by n - 1)"""
    _rejected(lib, lib.maeclip_pool_fwd(ptr, 2, 1, 8, ptr, None), b"maeclip_pool_fwd: bad args")
    _rejected(lib, lib.maeclip_pool_bwd(ptr, 2, 1, 8, ptr, 0, None), b"maeclip_pool_bwd: bad args")
    _rejected(lib, lib.maeclip_pool_fwd(None, 2, 3, 8, ptr, None), b"maeclip_pool_fwd: bad args")


def test_multi_tensor_launches_reject_empty_plans(lib, ptr):
    from mae_clip_amd import _lib as L
    ce = (L.ColsumEntry * 1)()
    ce[0].P, ce[0].N = 4, 8
    _rejected(lib, lib.maeclip_colsum_multi(ptr, ce, 0, None), b"maeclip_colsum_multi: bad args")
    _rejected(lib, lib.maeclip_colsum_multi(None, ce, 1, None), b"maeclip_colsum_multi: bad args")
    me = (L.MtEntry * 1)()
    me[0].n = 16
    _rejected(lib, lib.maeclip_cast_multi(ptr, me, 0, None), b"maeclip_cast_multi: bad args")
    _rejected(lib, lib.maeclip_cast_multi(None, me, 1, None), b"maeclip_cast_multi: bad args")
    hp = L.AdamwHparams(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step_size=1e-2, bc2_sqrt=0.03, grad_scale=1.0)
    _rejected(lib, lib.maeclip_adamw_multi(ptr, me, 0, ctypes.byref(hp), None), b"maeclip_adamw_multi: bad args")


def test_rows_colsum_rejects_bad_shapes(lib, ptr):
    from mae_clip_amd import _lib as L
    for M, D, ld in ((4, 6, 8), (4, 2052, 2052), (0, 8, 8), (4, 8, 10)):
        _rejected(lib, lib.maeclip_rows_colsum(ptr, L.F32, M, D, ld, None, ptr, None), b"maeclip_rows_colsum: bad args")
