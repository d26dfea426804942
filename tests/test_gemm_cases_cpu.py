"""The case table of test_gemm_reference_gpu.py checked without a GPU: every
case is legal and predicted onto the path it is meant for, its reference is
finite, its bound is meaningful (E32 > 0) and, for a bf16 output, tight enough
to tell round-to-nearest-even from truncation."""
import os

import pytest
import torch

from tests import gemm_cases as G
from tests.helpers import FACTOR, _bf16_half_ulp

GROUPS = {
    "shapes": G.shape_cases, "scalars": G.scalar_cases, "epilogues": G.epilogue_cases, "colsum": G.colsum_cases,
    "batched": G.batch_cases, "splitk": G.splitk_cases, "v4_split": G.v4_split_cases,
    "small_split": G.small_split_cases,
}


def _truncate_bf16(x64):
    """x rounded toward zero onto the bf16 grid"""
    bits = x64.float().view(torch.int32) & ~0xFFFF
    return bits.view(torch.float32).double()


@pytest.mark.parametrize("group", list(GROUPS))
def test_case_table(group):
    cases = GROUPS[group]()
    assert len({c.id for c in cases}) == len(cases)
    for c in cases:
        e = c.epc
        assert G.predict(c) == c.path, (c.id, G.predict(c))
        assert c.N % 4 == 0 and (c.la == G.RC or c.K % e == 0) and (c.lb == G.RC or c.K % e == 0), c.id
        assert (c.la == G.KC or c.M % e == 0) and (c.lb == G.KC or c.N % e == 0), c.id
        d = G.build(c)
        for name in ("C", "aux_out", "colsum"):
            if name == "aux_out" and "aux_out" not in d["bufs"]:
                continue
            if name == "aux_out" and name not in d["ref64"]:
                continue
            r64, r32 = d["ref64"][name], d["ref32"][name]
            assert torch.isfinite(r64).all(), (c.id, name)
            e32 = (r32.double() - r64).abs().max().item()
            assert e32 > 0, (c.id, name, "E32 = 0: choose another seed or scale")
            dt = c.out if name == "C" else (c.dt if name == "aux_out" else torch.float32)
            if dt == torch.bfloat16:
                err = (_truncate_bf16(r64) - r64).abs()
                assert (err > _bf16_half_ulp(r64, FACTOR * e32) + FACTOR * e32).any(), (c.id, name, "truncation passes")


ROUTE = {"v1f": 0, "v1b": 0, "small": 1, "v2": 2, "v4": 4}    # maeclip::GemmRoute
# the library reads MAECLIP_GEMM_VARIANT once per process and routes by it: the labels hold for the default only
PINNED = os.environ.get("MAECLIP_GEMM_VARIANT", "0").strip() not in ("", "0")


@pytest.mark.skipif(PINNED, reason="MAECLIP_GEMM_VARIANT pins a GEMM path in this environment")
@pytest.mark.parametrize("group", list(GROUPS))
def test_library_routes_every_case_to_its_path(group):
    """maeclip_gemm_impl (host arithmetic only: no launch, no device) against the label of every case"""
    import ctypes
    from mae_clip_amd import _lib as L
    lib = L.lib()
    for c in GROUPS[group]():
        a = G.gemm_args(c)
        assert lib.maeclip_gemm_impl(ctypes.byref(a)) == ROUTE[c.path], (c.id, lib.maeclip_last_error())


def test_total_is_a_few_hundred():
    n = sum(len(f()) for f in GROUPS.values())
    assert 200 <= n <= 800, n


def test_small_k_split_is_found_by_query():
    cs = G.small_split_cases()
    assert all(G.plan_workspace(c) > 0 for c in cs) and cs[0].K < 8192
