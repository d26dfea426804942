"""The launch sequences of the product, pinned on the CPU.

tests/launch_trace.py records, for one forward + backward of CLIPModel with
every kernel launch stubbed, which entry point is issued on which stream with
which scalar arguments, and every stream / event dependency between them.
tests/golden/launch_sequences.json holds those traces as recorded on the
commit before the per-block launch sequences were stated once
(functions.block_forward / block_backward / text_forward); the code must
reproduce every one of them exactly: the set of launches, their arguments,
their order on each stream, the fork / join / stagger points of the
micro-batch chains and the positions of the side-stream weight gradients.

A deliberate change of a launch sequence re-records the file
(python -m tests.launch_trace) and is reviewed as its diff.
"""
import json

import pytest

from tests import launch_trace as LT


@pytest.fixture(scope="module")
def golden():
    with open(LT.GOLDEN) as f:
        return LT.unpack(json.load(f))


def test_golden_covers_every_configuration(golden):
    assert sorted(golden) == sorted(LT.CONFIGS)


@pytest.mark.parametrize("name", list(LT.CONFIGS))
def test_launch_sequence(golden, name):
    # record() also asserts the micro-batch count of both stacks (2 at B = 128)
    got = json.loads(json.dumps(LT.record(**LT.CONFIGS[name])))
    want = golden[name]
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{name}: event {k} differs\n  got  {a}\n  want {b}"
    assert len(got) == len(want), f"{name}: {len(got)} events, golden has {len(want)}"


def test_traces_tell_the_configurations_apart(golden):
    """what each configuration is there for shows in its trace"""
    def names(t, stream=None):
        return [ev[0] for ev in t if stream is None or ev[1] == stream]

    def streams(t):
        return {ev[1] for ev in t if ev[0].startswith("maeclip_")}

    # micro-batches: a second chain on its own stream, gated by events under the stagger
    assert len(streams(golden["bf16_b128"])) == len(streams(golden["bf16_b8"])) + 1
    assert "wait_event" in names(golden["bf16_b128_stagger2"]) and "wait_event" not in names(golden["bf16_b128"])
    # fp8 attention writing its consumer's operand replaces the standalone quantisation passes
    q = lambda t: names(t).count("maeclip_quant_blocks_fp8")
    assert q(golden["fp8_b8_q8_00"]) > q(golden["fp8_b8_q8_11"])
    assert q(golden["fp8_b128_q8_00"]) > q(golden["fp8_b128_q8_11"])
    # ungrouped weight gradients: one GEMM each instead of the grouped launches
    assert "maeclip_wgrad_grouped" not in names(golden["bf16_b8_side_wgrad"])
    # the int64 mask is converted inside the embedding launch (mask pointers non-null)
    emb = lambda t: [ev for ev in t if ev[0] == "maeclip_embed_fwd"][0]
    assert emb(golden["frozen_train_i64mask"]) != emb(golden["frozen_train_f32mask"])
    assert golden["frozen_train_i64mask"] != golden["frozen_eval_i64mask"]
    assert "maeclip_embed_bwd" in names(golden["text_trainable_bf16"])
    assert "maeclip_embed_bwd" in names(golden["text_trainable_fp32"])
