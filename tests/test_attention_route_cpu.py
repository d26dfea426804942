"""The routing table of tests/attn_cases.py against the library, without a GPU:
maeclip_attn_impl runs the argument checks of maeclip_attn_fwd / _bwd and
maeclip::attn_route (host arithmetic only: no launch, no device) and returns
the path as a number, or -1 and the message of a rejection. The pointers
handed in are dummies and never dereferenced."""
import ctypes

import pytest

from tests import attn_cases as A

CASES = A.cases()


@pytest.fixture
def attn_opts():
    """set ATTN_* options for one test (every other one unset) and restore them all"""
    from mae_clip_amd import _lib as L
    lib = L.load()
    keys = {name: L.OPTIONS.index(name) for name in A.ATTN_OPTS}
    prev = {name: lib.maeclip_set_option(k, -1) for name, k in keys.items()}

    def set_(**kw):
        for name, v in kw.items():
            lib.maeclip_set_option(keys[name], v)

    yield set_
    for name, k in keys.items():
        lib.maeclip_set_option(k, prev[name])


def test_table_is_well_formed():
    assert len({c.id for c in CASES}) == len(CASES)
    assert 80 <= len(CASES) <= 300
    seen = {c.expect for c in CASES if isinstance(c.expect, int)}
    assert seen == set(range(11)), sorted(set(range(11)) - seen)   # every path is reached by some case
    assert any(isinstance(c.expect, bytes) for c in CASES)
    for c in CASES:
        assert set(c.opts) <= set(A.ATTN_OPTS) and set(c.kw) <= {"key_mask", "dropout_p", "q8", "ld_qkv"}, c.id


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_library_routes_the_case_as_labelled(case, attn_opts):
    attn_opts(**case.opts)
    rc, msg = A.impl(case.dtype, case.n, case.H, case.hd, case.bwd, **case.kw)
    if isinstance(case.expect, bytes):
        assert rc == -1 and case.expect in msg and b"launch failed" not in msg, (rc, msg)
    else:
        assert rc == case.expect, (A.NAMES[rc] if rc >= 0 else msg, A.NAMES[case.expect])


@pytest.mark.parametrize("bwd", [False, True])
def test_impl_checks_like_the_entry_points(bwd):
    """the argument checks come first, with the entry points' messages"""
    from mae_clip_amd import _lib as L
    lib = L.load()
    assert lib.maeclip_attn_impl(None, int(bwd)) == -1 and b"null pointer" in lib.maeclip_last_error()
    a = A.attn_args("bf16", 25, 2, 48, bwd=bwd)
    assert lib.maeclip_attn_impl(ctypes.byref(a), int(bwd)) == -1
    assert b"head_dim must be 32 or 64 (got 48)" in lib.maeclip_last_error()
    a = A.attn_args("bf16", 25, 2, 64, bwd=bwd, ld_qkv=3 * 128 + 4)
    assert lib.maeclip_attn_impl(ctypes.byref(a), int(bwd)) == -1
    assert b"row strides must be 16-byte multiples" in lib.maeclip_last_error()


def test_rejections_are_the_entry_points(attn_opts):
    """a rejected route gives maeclip_attn_fwd / _bwd the same return code and message"""
    from mae_clip_amd import _lib as L
    lib = L.load()
    for c in CASES:
        if not isinstance(c.expect, bytes):
            continue
        attn_opts(**{name: -1 for name in A.ATTN_OPTS})
        attn_opts(**c.opts)
        a = A.attn_args(c.dtype, c.n, c.H, c.hd, bwd=c.bwd, **c.kw)
        assert lib.maeclip_attn_impl(ctypes.byref(a), int(c.bwd)) == -1
        want = lib.maeclip_last_error()
        fn = lib.maeclip_attn_bwd if c.bwd else lib.maeclip_attn_fwd
        assert fn(ctypes.byref(a), None) == -1 and lib.maeclip_last_error() == want, (c.id, want)


def test_fwd_bwd_mode_table_names_every_kernel():
    """the table the GPU test asserts with reaches every backward kernel a mode names, and says where one does not"""
    assert A.fwd_bwd_paths("bf16", "two3", (2, 50, 3, 64)) == (A.FWD, A.BWD_TWO)
    assert A.fwd_bwd_paths("bf16", "two3", (2, 37, 4, 32)) == (A.FWD, A.BWD_TWO3)
    assert A.fwd_bwd_paths("bf16", "bw16", (1, 577, 2, 32)) == (A.FWD16, A.BWD_16)
    assert A.fwd_bwd_paths("f32", "four", (1, 577, 2, 32)) == (A.ROWS, A.ROWS)
