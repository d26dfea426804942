"""The launch plans of the v4 GEMM family against the hand-labelled tables of
tests/gemm_cases.py, without a GPU: maeclip_gemm_plan, maeclip_gemm_fp8_plan
and maeclip_wgrad_grouped_plan run the entry points' argument checks and the
plan functions the launches use (mae_clip_amd/csrc/gemm4_plan.h: host
arithmetic only, the CU count is an argument) and launch nothing. The pointers
handed in are dummies and never dereferenced."""
import ctypes
import dataclasses
import os

import pytest

from tests import gemm_cases as G
from tests.test_gemm_cases_cpu import GROUPS

PLANS = G.plan_cases()
WGRADS = G.wgrad_plan_cases()
NCUS = (256, 64)
# the library reads MAECLIP_GEMM_VARIANT once per process and routes by it: v4 plans exist for the default only
PINNED = os.environ.get("MAECLIP_GEMM_VARIANT", "0").strip() not in ("", "0")
pytestmark = pytest.mark.skipif(PINNED, reason="MAECLIP_GEMM_VARIANT pins a GEMM path in this environment")


@pytest.fixture
def plan_opts():
    """set plan options for one test (every other one of the family unset) and restore them all"""
    from mae_clip_amd import kernels as K
    prev = {name: K.set_option(name, None) for name in G.PLAN_OPTS}

    def set_(pairs):
        for name, v in pairs:
            K.set_option(name, v)

    yield set_
    for name, v in prev.items():
        K.set_option(name, v)


def _plan(c, ncu):
    from mae_clip_amd import kernels as K
    fp8 = {"bf16": None, "fp8rows": "rows", "fp8blocks": "blocks"}[c.family]
    return K.gemm_plan(G.plan_args(c), ncu, fp8=fp8)


def test_tables_are_well_formed():
    assert len({c.id for c in PLANS}) == len(PLANS) and len({c.id for c in WGRADS}) == len(WGRADS)
    assert {c.family for c in PLANS} == {"bf16", "fp8rows", "fp8blocks"}
    for c in PLANS + WGRADS:
        assert set(c.want) == set(NCUS) and {k for k, _ in c.opts} <= set(G.PLAN_OPTS), c.id
    # every tile height, a split and a plan that the CU count changes are in the table
    assert {w[0] for c in PLANS for w in c.want.values()} == {256, 192, 128}
    assert any(c.want[256][1] == 2 for c in PLANS) and any(c.want[256] != c.want[64] for c in PLANS)
    assert {w["mode"] for c in WGRADS for w in c.want.values()} == {"streamk", "split", "whole"}


@pytest.mark.parametrize("ncu", NCUS)
@pytest.mark.parametrize("case", PLANS, ids=lambda c: c.id)
def test_gemm_plan_is_as_labelled(case, ncu, plan_opts):
    plan_opts(case.opts)
    p = _plan(case, ncu)
    bm, S, L0, grid, persistent = case.want[ncu]
    assert p["route"] == 4
    assert (p["bm"], p["S"], p["L0"], p["grid"], p["persistent"]) == (bm, S, L0, grid, persistent), p
    assert p["lds_bytes"] == G.LDS[bm]
    # the workspace the launch would ask for: the split's, if a split is taken once a workspace is offered
    offered = _plan(dataclasses.replace(case, ws=True), ncu)
    assert p["workspace_bytes"] == (G.sk_ws(ncu) if offered["S"] > 0 else 0)
    assert p["workspace_bytes"] > 0 or S == 0


@pytest.mark.parametrize("ncu", NCUS)
@pytest.mark.parametrize("case", WGRADS, ids=lambda c: c.id)
def test_wgrad_plan_is_as_labelled(case, ncu, plan_opts):
    from mae_clip_amd import kernels as K
    plan_opts(case.opts)
    p = K.wgrad_plan(G.wgrad_problems(case.shapes), len(case.shapes), case.M, ncu=ncu)
    want = case.want[ncu]
    assert {k: p[k] for k in want} == want, p


def test_wgrad_plan_outside_the_grouped_kernel():
    """fp32, a ragged token count or a narrow dW run as one GEMM per problem: no plan"""
    from mae_clip_amd import _lib as L
    from mae_clip_amd import kernels as K
    probs = G.wgrad_problems(G.ENC_LAYER)
    assert K.wgrad_plan(probs, 4, 3200, ncu=256) is not None
    assert K.wgrad_plan(probs, 4, 3200, dtype=L.F32, ncu=256) is None
    assert K.wgrad_plan(probs, 4, 3232, ncu=256) is None
    assert K.wgrad_plan(G.wgrad_problems([(768, 128)]), 1, 3200, ncu=256) is None
    with pytest.raises(L.MaeClipNativeError, match="bad problem list"):
        K.wgrad_plan(probs, 0, 3200, ncu=256)


def test_options_are_restored(plan_opts):
    from mae_clip_amd import kernels as K
    before = {name: K.get_option(name) for name in G.PLAN_OPTS}
    with K.options(GEMM_BM=192, GEMM_SPLIT=2, WG_SK=0):
        c = next(c for c in PLANS if c.id == "split2_k256")
        assert _plan(c, 256)["S"] == 2
    assert {name: K.get_option(name) for name in G.PLAN_OPTS} == before
    assert _plan(next(c for c in PLANS if c.id == "split2_k256"), 256)["S"] == 0


def test_plan_checks_like_the_entry_points():
    """the argument checks come first, with maeclip_gemm's / maeclip_gemm_fp8's messages; other routes carry no plan"""
    from mae_clip_amd import _lib as L
    from mae_clip_amd import kernels as K
    lib = L.lib()
    out = (ctypes.c_int32 * 8)()
    assert lib.maeclip_gemm_plan(None, 256, ctypes.byref(out), None) == -1 and b"null args" in lib.maeclip_last_error()
    bad = G.plan_args(G.PlanCase("bad", 264, 262, 128, {}))
    assert lib.maeclip_gemm_plan(ctypes.byref(bad), 256, ctypes.byref(out), None) == -1
    assert b"N and ldc must be multiples of 4" in lib.maeclip_last_error()
    f8 = G.plan_args(G.PlanCase("bad8", 264, 264, 192, {}, family="fp8rows"))
    with pytest.raises(L.MaeClipNativeError, match="multiple of 128"):
        K.gemm_plan(f8, 256, fp8="rows")
    v2 = K.gemm_plan(G.gemm_args(G._rep("v2")), 256)
    assert v2["route"] == 2 and v2["bm"] == 0 and v2["grid"] == (0, 0, 0) and v2["workspace_bytes"] == 0


@pytest.mark.parametrize("group", list(GROUPS))
def test_workspace_query_is_the_plans(group, plan_opts):
    """maeclip_gemm_workspace == the plan's workspace_bytes for this machine's CU count (ncu = 0: the device's, 256
    without one), over the whole table of the reference tests, each case under its own options; the v4 cases with
    a forced split are the only ones that can ask for any"""
    from mae_clip_amd import _lib as L
    from mae_clip_amd import kernels as K
    lib = L.lib()
    asked = 0
    for c in GROUPS[group]():
        plan_opts(tuple((k, None) for k in G.PLAN_OPTS))
        plan_opts(c.opts)
        a = G.gemm_args(c)
        p = K.gemm_plan(a, 0)
        ws = int(lib.maeclip_gemm_workspace(ctypes.byref(a)))
        assert p["route"] == {"v1f": 0, "v1b": 0, "small": 1, "v2": 2, "v4": 4}[c.path], c.id
        assert ws == p["workspace_bytes"], (c.id, ws, p)
        asked += ws > 0 and c.path == "v4"
    assert asked == 0 or group == "v4_split"
