"""Argument rejections of maeclip_gemm and its host-side queries on the real
library. No GPU is needed: every check comes before any launch, so the (host)
pointers handed in are never dereferenced on a device. A call that got past
its checks would fail differently ("launch failed", return -2), which is why
each case also looks at the message. The kernels themselves are compared with
fp64 references in test_gemm_reference_gpu.py."""
import ctypes
import os

import pytest

from mae_clip_amd import _lib as L

_BUF = (ctypes.c_float * 64)()
P = ctypes.addressof(_BUF) // 16 * 16 + 16      # a 16-byte aligned host address


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _args(**kw):
    """a valid small fp32 call; kw overrides"""
    d = dict(A=P, B=P, C=P, M=8, N=8, K=8, lda=8, ldb=8, ldc=8, batch=1, dtype=L.F32, out_dtype=L.F32, a_layout=0,
             b_layout=0, epilogue=0, alpha=1.0, beta=0.0, splitk=1)
    d.update(kw)
    return L.GemmArgs(**d)


def _rejected(lib, a, what):
    rc = lib.maeclip_gemm(ctypes.byref(a) if a is not None else None, None)
    msg = lib.maeclip_last_error()
    assert rc == -1, (rc, msg)
    assert what in msg and b"launch failed" not in msg, msg


BF = dict(dtype=L.BF16)
CASES = {
    "negative M": (dict(M=-1), b"bad sizes"),
    "negative N": (dict(N=-4), b"bad sizes"),
    "negative K": (dict(K=-8), b"bad sizes"),
    "batch 0": (dict(batch=0), b"bad sizes"),
    "M >= 2^31": (dict(M=1 << 31), b"dims too large"),
    "N >= 2^31": (dict(N=1 << 31), b"dims too large"),
    "K >= 2^31": (dict(K=1 << 31), b"dims too large"),
    "dtype 7": (dict(dtype=7), b"bad dtype"),
    "fp8 dtype": (dict(dtype=2), b"bad dtype"),
    "out dtype 2": (dict(out_dtype=2), b"bad out dtype"),
    "fp32 K % 4 (A and B K-contiguous)": (dict(K=6), b"A contiguous dim"),
    "bf16 K % 8": (dict(K=12, lda=16, ldb=16, **BF), b"A contiguous dim"),
    "fp32 M % 4, row-contiguous A": (dict(M=6, a_layout=1), b"A contiguous dim"),
    "bf16 M % 8, row-contiguous A": (dict(M=12, lda=16, a_layout=1, **BF), b"A contiguous dim"),
    "bf16 N % 8, row-contiguous B": (dict(N=12, ldb=16, ldc=12, b_layout=1, **BF), b"B contiguous dim"),
    "fp32 K % 4, row-contiguous A": (dict(K=6, a_layout=1), b"B contiguous dim"),
    "lda % 4": (dict(lda=10), b"A contiguous dim"),
    "ldb % 4": (dict(ldb=10), b"B contiguous dim"),
    "bf16 lda % 8": (dict(lda=12, **BF), b"A contiguous dim"),
    "bf16 ldb % 8": (dict(ldb=12, **BF), b"B contiguous dim"),
    "N % 4": (dict(N=6), b"N and ldc"),
    "ldc % 4": (dict(ldc=10), b"N and ldc"),
    "A not 16-byte aligned": (dict(A=P + 8), b"operands must be 16-byte aligned"),
    "B not 16-byte aligned": (dict(B=P + 4), b"operands must be 16-byte aligned"),
    "C not 8-byte aligned": (dict(C=P + 4), b"operands must be 16-byte aligned"),
    "epilogue 3 without aux": (dict(epilogue=3), b"DGELU / MUL_AUX epilogue needs aux"),
    "epilogue 5 without aux": (dict(epilogue=5), b"DGELU / MUL_AUX epilogue needs aux"),
    "epilogue 2 without resid": (dict(epilogue=2), b"RESID epilogue"),
    "epilogue 2 with bf16 output": (dict(epilogue=2, resid=P, ldr=8, out_dtype=L.BF16), b"RESID epilogue"),
    "split-K without workspace": (dict(splitk=2), b"split-K needs"),
    "split-K with an epilogue": (dict(splitk=2, workspace=P, epilogue=1), b"split-K needs"),
    "split-K with colsum": (dict(splitk=2, workspace=P, colsum_partial=P), b"split-K needs"),
    "split-K with ldc != N": (dict(splitk=2, workspace=P, ldc=12), b"split-K output must be dense"),
    "S > 64": (dict(splitk=65, workspace=P), b"split-K needs"),
    # before the fix an unknown epilogue fell through each path's `default:` into another epilogue's kernel
    # (mul-aux on gemm_small, dGELU on v2 / v4, both with a null aux) instead of being rejected
    "epilogue 6, fp32 (gemm_small)": (dict(epilogue=6), b"bad epilogue"),
    "epilogue 6, bf16 K % 64 = 0 (v2)": (dict(epilogue=6, K=64, lda=64, ldb=64, **BF), b"bad epilogue"),
    "epilogue 6, bf16 (v4)": (dict(epilogue=6, M=256, N=256, K=64, lda=64, ldb=64, ldc=256, **BF), b"bad epilogue"),
    "epilogue 6, bf16 (v1)": (dict(epilogue=6, K=8, **BF), b"bad epilogue"),
    "epilogue -1": (dict(epilogue=-1), b"bad epilogue"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_gemm_rejects(lib, name):
    kw, what = CASES[name]
    _rejected(lib, _args(**kw), b"maeclip_gemm: " + what)


def test_gemm_rejects_null_args(lib):
    _rejected(lib, None, b"maeclip_gemm: null args")


def test_gemm_impl_checks_like_gemm(lib):
    """the route query runs maeclip_gemm's argument checks first: -1 and a message of its own"""
    for a, what in ((_args(epilogue=6), b"bad epilogue 6"), (_args(epilogue=-1), b"bad epilogue -1"),
                    (None, b"null args"), (_args(K=6), b"A contiguous dim")):
        rc = lib.maeclip_gemm_impl(ctypes.byref(a) if a is not None else None)
        msg = lib.maeclip_last_error()
        assert rc == -1 and msg.startswith(b"maeclip_gemm_impl: ") and what in msg, (rc, msg)
    assert lib.maeclip_gemm_impl(ctypes.byref(_args(M=0))) == 0   # an empty output: valid, runs on no kernel
    if os.environ.get("MAECLIP_GEMM_VARIANT", "0").strip() in ("", "0"):     # a pinned variant moves the route
        assert lib.maeclip_gemm_impl(ctypes.byref(_args())) == 1   # the valid small fp32 call: gemm_small


def test_gemm_empty_output_is_a_no_op(lib):
    """M = 0 or N = 0 returns 0 before the remaining checks and launches nothing"""
    for kw in (dict(M=0), dict(N=0), dict(M=0, N=0)):
        a = _args(A=None, B=None, C=None, **kw)
        assert lib.maeclip_gemm(ctypes.byref(a), None) == 0, kw


def test_colsum_rows(lib):
    for M in (0, 1, 63, 64, 65, 127, 128, 129, 1000, 50432, (1 << 31) - 1):
        assert lib.maeclip_gemm_colsum_rows(M) == -(-M // 64)


def test_splitk_query(lib):
    for M in (1, 8, 128, 136, 255, 256, 264, 768, 3072):
        for N in (4, 128, 256, 520, 2304):
            for Kd in (4, 8, 64, 504, 512, 1016, 1024, 4096, 50432, 1 << 20):
                s = lib.maeclip_gemm_splitk(M, N, Kd)
                assert 1 <= s <= 64, (M, N, Kd, s)
                if Kd < 512:    # shorter than one slice of either plan
                    assert s == 1, (M, N, Kd, s)


def test_workspace_query(lib):
    assert lib.maeclip_gemm_workspace(None) == 0
    for kw in (dict(), dict(M=96, N=64, K=4096), dict(M=512, N=512, K=1024, lda=1024, ldb=1024, ldc=512, **BF)):
        a = _args(splitk=2, workspace=P, **kw)
        assert lib.maeclip_gemm_workspace(ctypes.byref(a)) == 0, kw
    # without a caller split the long-K small fp32 shape does ask for its K-slice partials
    a = _args(M=96, N=64, K=4096, lda=4096, ldb=4096, ldc=64)
    assert lib.maeclip_gemm_workspace(ctypes.byref(a)) > 0
