"""Retrieval evaluation (maeclip_sim_topk and its two host-only queries) at the
C-ABI boundary, without a GPU: the symbols are exported and bound, every
argument error is reported before any device call, the split plan and the
workspace size follow include/maeclip.h, and the Python wrappers refuse CPU
tensors and wrong dtypes / ranks."""
import ctypes

import pytest
import torch

from mae_clip_amd import _lib as L

NAMES = {"maeclip_sim_topk_splits": 5, "maeclip_sim_topk_workspace": 5, "maeclip_sim_topk": 17}
PTR = 0x1000   # a non-null pointer that is never followed: every call here fails its argument checks


def sim_topk(lib, Q=4, N=100, P=64, ldq=None, ldg=None, k=5, splits=0, q=PTR, g=PTR, vals=PTR, idx=PTR, ql=None,
             gl=None, fh=None, ws=None, ws_bytes=0):
    return lib.maeclip_sim_topk(q, g, Q, N, P, P if ldq is None else ldq, P if ldg is None else ldg, k, splits, vals,
                                idx, ql, gl, fh, ws, ws_bytes, None)


def test_symbols_exported_bound_and_abi_unchanged():
    lib = L.load()
    for name, nargs in NAMES.items():
        assert hasattr(lib, name), name
        assert name in L.EXPORTED_SYMBOLS, name
        assert len(L._SIGS[name][1]) == nargs, name
    assert L._SIGS["maeclip_sim_topk_workspace"][0] is ctypes.c_int64
    assert lib.maeclip_abi_version() == 14 and L.ABI_VERSION == 14
    assert len(L.OPTIONS) == 14


@pytest.mark.parametrize("kw", [
    dict(k=0), dict(k=65), dict(N=9, k=10),
    dict(P=24), dict(P=528),
    dict(P=64, ldq=63),
    dict(vals=None),
    dict(ql=PTR), dict(gl=PTR, fh=PTR), dict(ql=PTR, gl=PTR),
    dict(splits=2, ws=PTR, ws_bytes=2 * 4 * 5 * 12 - 1), dict(splits=2),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_argument_errors_name_the_call(kw):
    lib = L.load()
    assert sim_topk(lib, **kw) < 0
    assert b"maeclip_sim_topk" in lib.maeclip_last_error()


def test_queries_reject_bad_shapes():
    lib = L.load()
    for fn in (lib.maeclip_sim_topk_splits, lib.maeclip_sim_topk_workspace):
        for Q, N, P, k, s in [(1, 10, 64, 11, 0), (1, 10, 24, 1, 0), (1, 0, 64, 1, 0), (-1, 10, 64, 1, 0),
                              (1, 10, 64, 1, -1), (1, 100, 528, 1, 0), (1, 100, 64, 65, 0)]:
            assert fn(Q, N, P, k, s) < 0, (Q, N, P, k, s)
            assert b"maeclip_sim_topk" in lib.maeclip_last_error()


def test_split_plan():
    lib = L.load()
    splits = lib.maeclip_sim_topk_splits
    # forced: taken as given up to the number of 16-row gallery tiles
    for N, forced, want in [(300, 1, 1), (300, 2, 2), (300, 7, 7), (300, 19, 19), (300, 20, 19), (300, 1000, 19),
                            (1001, 1000, 63), (129, 7, 7), (16, 2, 1), (17, 1000, 2), (1, 5, 1)]:
        assert splits(3, N, 64, 1, forced) == want, (N, forced)
    # automatic: one slice when the query blocks fill the chip, many for one query
    assert splits(25000, 5000, 256, 10, 0) == 1
    s1 = splits(1, 100000, 256, 45, 0)
    assert 1 < s1 <= (100000 + 15) // 16
    assert splits(0, 100, 64, 5, 0) >= 1


def test_workspace_size():
    lib = L.load()
    ws = lib.maeclip_sim_topk_workspace
    assert ws(25000, 5000, 256, 10, 0) == 0
    assert ws(7, 300, 64, 5, 1) == 0
    for Q, N, P, k, forced in [(7, 300, 64, 5, 2), (1, 100000, 256, 45, 0), (33, 1001, 512, 45, 1000)]:
        S = lib.maeclip_sim_topk_splits(Q, N, P, k, forced)
        assert S > 1
        assert ws(Q, N, P, k, forced) >= S * Q * k * 12


def test_wrappers_refuse_cpu_tensors_and_wrong_types():
    from mae_clip_amd import retrieval as R
    q, g = torch.randn(3, 64), torch.randn(20, 64)
    with pytest.raises(L.MaeClipNativeError):
        R.similarity_topk(q, g, 5)
    with pytest.raises(L.MaeClipNativeError):
        R.recall_at_k(q, g, torch.arange(3), torch.arange(20))
    with pytest.raises(L.MaeClipNativeError):
        R.zero_shot_accuracy(q, g, torch.arange(3))
    with pytest.raises(ValueError):
        R.similarity_topk(q.bfloat16(), g, 5)
    with pytest.raises(ValueError):
        R.similarity_topk(q, g[0], 5)
    for name in ("get_text_embeddings", "evaluate_retrieval"):
        assert callable(getattr(R, name))
