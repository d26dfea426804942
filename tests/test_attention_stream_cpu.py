"""Routing and rejections of the streamed bf16 attention kernels (option
ATTN_STREAM) on the real library. No GPU is needed: the streamed path decides
and rejects before any HIP call, so the host pointers handed in are never
dereferenced. A call that got past its checks would fail differently ("launch
failed", return -2), which is why each case also looks at the message. The
kernels themselves are compared with fp64 in test_attention_stream_gpu.py."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from mae_clip_amd import _lib as L
    return L.load()


@pytest.fixture
def stream_opt(lib):
    """set ATTN_STREAM for one test and restore it"""
    from mae_clip_amd import _lib as L
    key = L.OPTIONS.index("ATTN_STREAM")
    prev = []

    def set_(v):
        prev.append(lib.maeclip_set_option(key, v))

    yield set_
    if prev:
        lib.maeclip_set_option(key, prev[0])


_BUF = (ctypes.c_float * 64)()


def _args(n, hd=64, H=2, key_mask=False, dropout_p=0.0):
    from mae_clip_amd import _lib as L
    p = ctypes.cast(_BUF, ctypes.c_void_p).value
    D = H * hd
    return L.AttnArgs(qkv=p, o=p, lse=p, dout=p, dqkv=p, key_mask=p if key_mask else None, colsum_partial=None,
                      ld_qkv=3 * D, ld_o=D, ld_dqkv=3 * D, B=1, n=n, H=H, head_dim=hd, dtype=L.BF16,
                      scale=hd ** -0.5, dropout_p=dropout_p, seed=0, step_ptr=None)


def _rejected(lib, rc, *what):
    msg = lib.maeclip_last_error()
    assert rc == -1, (rc, msg)
    assert all(w in msg for w in what) and b"launch failed" not in msg, msg


@pytest.mark.parametrize("bwd", [False, True])
@pytest.mark.parametrize("kw", [dict(key_mask=True), dict(dropout_p=0.1)])
def test_streamed_path_rejects_mask_and_dropout(lib, bwd, kw):
    """n = 700 at head_dim 64 is past the resident limit (576): the streamed
    path takes the call, and it has neither a key mask nor dropout"""
    a = _args(700, **kw)
    fn = lib.maeclip_attn_bwd if bwd else lib.maeclip_attn_fwd
    _rejected(lib, fn(ctypes.byref(a), None), b"streamed path", b"n > 576 at head_dim 64")


@pytest.mark.parametrize("bwd", [False, True])
def test_forced_streamed_path_rejects_mask_below_the_limit(lib, bwd, stream_opt):
    stream_opt(1)
    a = _args(25, key_mask=True)
    fn = lib.maeclip_attn_bwd if bwd else lib.maeclip_attn_fwd
    _rejected(lib, fn(ctypes.byref(a), None), b"streamed path")


@pytest.mark.parametrize("bwd", [False, True])
def test_stream_off_keeps_the_lds_rejection(lib, bwd, stream_opt):
    stream_opt(0)
    a = _args(700)
    fn = lib.maeclip_attn_bwd if bwd else lib.maeclip_attn_fwd
    _rejected(lib, fn(ctypes.byref(a), None), b"maeclip_attn: n=700 needs", b"of LDS")


def test_option_round_trip_and_table(lib):
    from mae_clip_amd import _lib as L
    from mae_clip_amd import kernels as K
    assert len(L.OPTIONS) == 14 and L.OPTIONS[13] == "ATTN_STREAM"
    assert lib.maeclip_abi_version() == 14 == L.ABI_VERSION
    prev = K.set_option("ATTN_STREAM", 1)
    try:
        assert K.get_option("ATTN_STREAM") == 1
        assert K.set_option("ATTN_STREAM", 0) == 1
        assert K.get_option("ATTN_STREAM") == 0
        assert K.set_option("ATTN_STREAM", None) == 0
        assert K.get_option("ATTN_STREAM") == -1
    finally:
        K.set_option("ATTN_STREAM", prev)
    # one past the table is no option
    assert lib.maeclip_set_option(14, 1) == -2 ** 31
