"""Launch sequence of a dropping block, recorded on the CPU by tests/launch_trace
(every launch stubbed, streams faked): a two-block encoder at drop_path_rate
0.5 has the per-block rates [0, 0.5], so block 0 must issue exactly the
launches of a model without drop-path and block 1 those plus two
maeclip_droppath_fwd and two maeclip_droppath_bwd, on the stream of the chain
they belong to. That the default rate moves nothing is the unchanged
test_launch_sequence_cpu.py (its golden file is reproduced with rate 0)."""
import difflib
import json

import pytest
import torch

from tests import launch_trace as LT

RATE = 0.5
P1 = float(torch.linspace(0, RATE, 2)[1])


@pytest.fixture()
def traced(monkeypatch):
    """record(**kw) -> (events, the drop-path wrappers' calls); the new host-only
    query keeps its real implementation like the others of launch_trace._QUERIES"""
    from mae_clip_amd import kernels as K
    monkeypatch.setattr(LT, "_QUERIES", LT._QUERIES | {"maeclip_droppath_partial_rows"})
    calls = []
    fwd, bwd = K.droppath_fwd, K.droppath_bwd

    def rec_fwd(resid, branch, n, **kw):
        calls.append(("fwd", tuple(branch.shape), n, kw["p"], kw["k"], kw["sample_offset"], kw["step_ptr"] is not None))
        return fwd(resid, branch, n, **kw)

    def rec_bwd(g, n, dtype, **kw):
        calls.append(("bwd", tuple(g.shape), n, kw["p"], kw["k"], kw["sample_offset"], kw["step_ptr"] is not None))
        return bwd(g, n, dtype=dtype, **kw)
    monkeypatch.setattr(K, "droppath_fwd", rec_fwd)
    monkeypatch.setattr(K, "droppath_bwd", rec_bwd)

    def run(**kw):
        del calls[:]
        ev = LT.record(**kw)
        return ev, list(calls)
    return run


def _changes(base, drop):
    """(removed events, added events) per changed place, in order"""
    sm = difflib.SequenceMatcher(a=[json.dumps(e) for e in base], b=[json.dumps(e) for e in drop], autojunk=False)
    return [(base[i0:i1], drop[j0:j1]) for op, i0, i1, j0, j1 in sm.get_opcodes() if op != "equal"]


def _gemm_without_resid(ev):
    """a maeclip_gemm event with the residual epilogue taken out: epilogue 2 -> 0, resid, ldr -> 0"""
    from mae_clip_amd import _lib as L
    names = [f[0] for f in L.GemmArgs._fields_]
    a = list(ev[2])
    assert a[names.index("epilogue")] == 2 and a[names.index("resid")] == 1
    a[names.index("epilogue")] = a[names.index("resid")] = a[names.index("ldr")] = 0
    return [ev[0], ev[1], a]


def test_default_rate_issues_no_droppath_launch(traced):
    ev, calls = traced(precision="bf16", B=8)
    assert not calls and not any(e[0].startswith("maeclip_droppath") for e in ev)


def test_two_block_encoder_whole_batch(traced):
    """bf16, B = 8, one chain: 16 encoder rows (n = 2 visible tokens), D = 192"""
    from mae_clip_amd import _lib as L
    base, _ = traced(precision="bf16", B=8)
    drop, calls = traced(precision="bf16", B=8, cfg=dict(drop_path_rate=RATE))
    ch = _changes(base, drop)
    chain = ch[0][0][0][1]          # the stream of the encoder's chain
    # forward of block 1: proj and fc2 lose the residual epilogue, a drop-path launch follows each
    for (old, new), K_ in zip(ch[:2], (192, 768)):
        assert len(old) == 1 and old[0][0] == "maeclip_gemm" and old[0][2][5] == K_
        assert new == [_gemm_without_resid(old[0]), ["maeclip_droppath_fwd", old[0][1], "*"]]
    # backward of block 1 (the top block): its own scaled copy of g instead of the copy from above ...
    old, new = ch[2]
    assert [e[0] for e in old] == ["maeclip_rows_colsum"] and new == [["maeclip_droppath_bwd", old[0][1], "*"]]
    # ... and the norm2 backward without its bf16 copy and column partials, then the scaled dx1
    old, new = ch[3]
    names = [f[0] for f in L.LnBwdArgs._fields_]
    assert len(old) == 1 and old[0][0] == "maeclip_ln_bwd" and len(new) == 2
    want = list(old[0][2])
    assert want[names.index("dx_bf")] == 1 and want[names.index("dx_colsum_partial")] == 1
    want[names.index("dx_bf")] = want[names.index("dx_colsum_partial")] = 0
    assert new == [["maeclip_ln_bwd", old[0][1], want], ["maeclip_droppath_bwd", old[0][1], "*"]]
    # the column reduction sees the drop-path partial row counts (64-row groups) for proj.bias and fc2.bias
    old, new = ch[4]
    assert [e[0] for e in old] == [e[0] for e in new] == ["maeclip_colsum_multi"]
    assert len(ch) == 5
    assert all(e[1] == chain for _, new in ch for e in new)
    # block 1 of the WHOLE encoder: keys 2 (attention) and 3 (MLP); forward 2, 3, backward 3, 2
    assert calls == [("fwd", (16, 192), 2, P1, 2, 0, True), ("fwd", (16, 192), 2, P1, 3, 0, True),
                     ("bwd", (16, 192), 2, P1, 3, 0, True), ("bwd", (16, 192), 2, P1, 2, 0, True)]
    # block 0 (rate 0) issues today's launches. Forward: the first changed event is launch 4 of
    # block 1 (its proj GEMM), so the ten launches of the chain in front of it are block 0's seven
    # and block 1's first three, the same events in both traces
    FWD = ["maeclip_ln_fwd", "maeclip_gemm", "maeclip_attn_fwd", "maeclip_gemm", "maeclip_ln_fwd", "maeclip_gemm",
           "maeclip_gemm"]
    BWD = ["maeclip_gemm", "maeclip_gemm", "maeclip_ln_bwd", "maeclip_gemm", "maeclip_attn_bwd", "maeclip_gemm",
           "maeclip_ln_bwd"]
    first = next(i for i, (a, b) in enumerate(zip(base, drop)) if a != b)
    assert base[first] == ch[0][0][0] and drop[:first] == base[:first]
    on_chain = lambda ev: [e for e in ev if e[1] == chain and e[0].startswith("maeclip_")]
    assert [e[0] for e in on_chain(base[:first])[-10:]] == FWD + FWD[:3]
    # backward: behind block 1's last drop-path launch come its launches 4 .. 7 and block 0's seven,
    # the events the base issues behind its norm2 backward
    jb = max(i for i, e in enumerate(drop) if e[0] == "maeclip_droppath_bwd") + 1
    ib = base.index(ch[3][0][0]) + 1
    tail_d, tail_b = on_chain(drop[jb:])[:11], on_chain(base[ib:])[:11]
    assert [e[0] for e in tail_d] == BWD[3:] + BWD and tail_d == tail_b


def test_two_block_encoder_micro_batches(traced):
    """bf16, B = 128, two micro-batches on two streams: each chain issues its own
    four launches with its first sample as the offset"""
    base, _ = traced(precision="bf16", B=128, microbatches=2)
    drop, calls = traced(precision="bf16", B=128, microbatches=2, cfg=dict(drop_path_rate=RATE))
    dp = [e for e in drop if e[0].startswith("maeclip_droppath")]
    streams = sorted({e[1] for e in dp})
    assert len(streams) == 2 and len(dp) == 8
    for st in streams:
        assert [e[0] for e in dp if e[1] == st] == ["maeclip_droppath_fwd"] * 2 + ["maeclip_droppath_bwd"] * 2
    rows = 64 * 2
    assert sorted(calls) == sorted(
        [(d, (rows, 192), 2, P1, k, off, True) for d, ks in (("fwd", (2, 3)), ("bwd", (3, 2))) for k in ks
         for off in (0, 64)])
    # per kind of launch, the two models differ only in the launches named in the whole-batch test
    count = lambda ev, name: sum(e[0] == name for e in ev)
    for name in ("maeclip_gemm", "maeclip_ln_fwd", "maeclip_ln_bwd", "maeclip_attn_fwd", "maeclip_attn_bwd",
                 "maeclip_wgrad_grouped", "maeclip_colsum_multi"):
        assert count(base, name) == count(drop, name), name
    assert count(base, "maeclip_rows_colsum") == count(drop, "maeclip_rows_colsum") + 1


def test_eval_mode_issues_no_droppath_launch(traced):
    ev, calls = traced(precision="bf16", B=8, mode="eval", cfg=dict(drop_path_rate=RATE))
    base, _ = traced(precision="bf16", B=8, mode="eval")
    assert not calls and ev == base
