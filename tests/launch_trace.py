"""Launch-sequence recorder behind tests/test_launch_sequence_cpu.py.

One forward + backward of CLIPModel on the CPU with every kernel launch
stubbed (tests/test_plumbing_cpu.py::stubbed_kernels) and torch's streams and
events replaced by fakes with distinct ids. The ordered trace holds, per
launch, the entry-point name, the stream it was issued on and its scalar
arguments (pointers only as null / non-null); per wait_stream / wait_event /
Event.record, the streams involved. Stream and event ids are renumbered by
first appearance, so a trace does not depend on what ran before it.

`python -m tests.launch_trace [out.json]` records every configuration of
CONFIGS and writes tests/golden/launch_sequences.json: a table of the distinct
events and, per configuration, the indices into it. The golden file is
recorded with this module on the commit BEFORE a change of the launch
sequences and must be reproduced exactly after it.
"""
import contextlib
import ctypes
import json
import os
import sys

import pytest
import torch

from tests.helpers import product_config, make_batch, C0
from tests import test_plumbing_cpu as plumbing

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_sequences.json")

# host-only entry points beyond test_plumbing_cpu._QUERIES (sizes of fp8 scale
# layouts and reduction scratch): the real implementation
_QUERIES = plumbing._QUERIES | {"maeclip_fp8b_scale_bytes", "maeclip_colsum_scratch",
                                "maeclip_quant_cols_fp8_workspace", "maeclip_quant_weights_fp8_prepare"}


class Trace:
    def __init__(self):
        self.events = []
        self.ids = {}        # raw stream / event id -> number of first appearance

    def sid(self, raw):
        if raw is None:
            return None
        return self.ids.setdefault(raw, len(self.ids))

    def add(self, *ev):
        self.events.append(list(ev))


_NEXT = [1000]
_CURRENT = [None]
_TRACE = [None]


def _new_id():
    _NEXT[0] += 1
    return _NEXT[0]


class FakeStream:
    def __init__(self, *a, **k):
        self.cuda_stream = _new_id()

    def wait_stream(self, other):
        _TRACE[0].add("wait_stream", _TRACE[0].sid(self.cuda_stream), _TRACE[0].sid(other.cuda_stream))

    def wait_event(self, ev):
        _TRACE[0].add("wait_event", _TRACE[0].sid(self.cuda_stream), _TRACE[0].sid(ev.id))

    def synchronize(self):
        pass


class FakeEvent:
    def __init__(self, *a, **k):
        self.id = _new_id()

    def record(self, stream=None):
        s = stream if stream is not None else _CURRENT[0]
        _TRACE[0].add("event_record", _TRACE[0].sid(self.id), _TRACE[0].sid(s.cuda_stream))

    def synchronize(self):
        pass


@contextlib.contextmanager
def _fake_stream_scope(st):
    prev, _CURRENT[0] = _CURRENT[0], st
    try:
        yield
    finally:
        _CURRENT[0] = prev


def _struct_fields(obj):
    """non-pointer fields by value, pointer fields as 0 (null) / 1"""
    out = []
    for name, ty in obj._fields_:
        v = getattr(obj, name)
        out.append(int(bool(v)) if ty is ctypes.c_void_p else v)
    return out


class TraceLib:
    """libmaeclip with every launch recorded instead of run"""

    def __init__(self, real):
        from mae_clip_amd import _lib
        self._real = real
        self._full = (_lib.GemmArgs, _lib.AttnArgs, _lib.LnFwdArgs, _lib.LnBwdArgs)
        self._arrays = (_lib.ColsumEntry, _lib.WgradProblem)

    def __getattr__(self, name):
        if name in _QUERIES:
            return getattr(self._real, name)
        fn = getattr(self._real, name)
        types = fn.argtypes

        def launch(*args):
            assert len(args) == len(types), (name, len(args), len(types))
            tr = _TRACE[0]
            args, tys = list(args), list(types)
            stream = None
            if tys and tys[-1] is ctypes.c_void_p:
                stream = tr.sid(args.pop())
                tys.pop()
            rec = []
            for a, ty in zip(args, tys):
                if ty is ctypes.c_void_p:
                    rec.append(int(bool(a)))
                elif hasattr(ty, "contents"):         # POINTER(struct)
                    obj = getattr(a, "_obj", a)
                    if isinstance(obj, self._full):
                        rec.append(_struct_fields(obj))
                    elif isinstance(obj, ctypes.Array) and issubclass(obj._type_, self._arrays):
                        rec.append([_struct_fields(e) for e in obj])
                    else:
                        rec.append("*")
                else:
                    rec.append(a)
            tr.add(name, stream, *rec)
            return 0
        return launch


@contextlib.contextmanager
def tracing():
    """stubbed_kernels with the launches recorded and streams / events faked;
    yields the Trace"""
    from mae_clip_amd import _lib, config as CFG
    mp = pytest.MonkeyPatch()
    side = CFG.side_stream
    try:
        with plumbing.stubbed_kernels(mp):
            mp.setattr(CFG, "side_stream", side)      # stubbed_kernels turns it off
            mp.setattr(_lib, "lib", lambda lib=TraceLib(_lib.load()): lib)
            tr = Trace()
            _TRACE[0] = tr
            _CURRENT[0] = FakeStream()
            mp.setattr(torch.cuda, "current_stream", lambda *a, **k: _CURRENT[0])
            mp.setattr(torch.cuda, "current_device", lambda: 0)
            mp.setattr(torch.cuda, "stream", _fake_stream_scope)
            mp.setattr(torch.cuda, "Stream", FakeStream)
            mp.setattr(torch.cuda, "Event", FakeEvent)
            mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
            mp.setattr(torch.Tensor, "record_stream", lambda self, s: None)
            yield tr
    finally:
        mp.undo()
        _TRACE[0] = _CURRENT[0] = None


# name -> dict(precision, B, and optionally: mask_ratio, env, cfg (config overrides),
# mode ("train" / "eval"), pad (ragged masks), float_mask)
CONFIGS = {
    "fp32_b8": dict(precision="fp32", B=8),
    "bf16_b8": dict(precision="bf16", B=8),
    "bf16_b8_mask0": dict(precision="bf16", B=8, mask_ratio=0.0),
    "bf16_b128": dict(precision="bf16", B=128, microbatches=2),
    "bf16_b128_stagger2": dict(precision="bf16", B=128, microbatches=2, env={"MAECLIP_MB_STAGGER": "2"}),
    "fp8_b8_q8_11": dict(precision="fp8", B=8, cfg=dict(fp8_attn_q8=(True, True))),
    "fp8_b8_q8_00": dict(precision="fp8", B=8, cfg=dict(fp8_attn_q8=(False, False))),
    "fp8_b128_q8_11": dict(precision="fp8", B=128, microbatches=2, cfg=dict(fp8_attn_q8=(True, True))),
    "fp8_b128_q8_00": dict(precision="fp8", B=128, microbatches=2, cfg=dict(fp8_attn_q8=(False, False))),
    "bf16_b8_side_wgrad": dict(precision="bf16", B=8, cfg=dict(wgrad_grouped=False, side_stream=True)),
    "frozen_train_i64mask": dict(precision="bf16", B=8),
    "frozen_train_f32mask": dict(precision="bf16", B=8, float_mask=True),
    "frozen_eval_i64mask": dict(precision="bf16", B=8, mode="eval"),
    "frozen_eval_f32mask": dict(precision="bf16", B=8, mode="eval", float_mask=True),
    "text_trainable_bf16": dict(precision="bf16", B=8, pad=True, cfg=dict(text_trainable=True)),
    "text_trainable_fp32": dict(precision="fp32", B=8, pad=True, cfg=dict(text_trainable=True)),
}


def record(precision, B, mask_ratio=0.75, env=None, cfg=None, mode="train", pad=False, float_mask=False,
           microbatches=1):
    """The trace of one forward + backward of CLIPModel at C0 shapes (2 encoder
    blocks, 2 decoder blocks, 2 text layers)."""
    from mae_clip_amd.CLIP import CLIPModel
    from mae_clip_amd import functions as Fn
    kw = {k: v for k, v in C0.items() if k != "batch_size"}
    kw.update(mask_ratio=mask_ratio, **(cfg or {}))
    old_env = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        with tracing() as tr, product_config(precision=precision, **kw):
            torch.manual_seed(0)
            m = CLIPModel()
            m.image_encoder.model.blocks = m.image_encoder.model.blocks[:2]
            m.train() if mode == "train" else m.eval()
            seen = []
            real_count = Fn.microbatch_count

            def count(spec):
                seen.append(real_count(spec))
                return seen[-1]
            Fn.microbatch_count = count
            try:
                batch = make_batch(B, C0["size"], pad=pad)
                if float_mask:
                    batch["attention_mask"] = batch["attention_mask"].float()
                m(batch).backward()
            finally:
                Fn.microbatch_count = real_count
            stacks = 2 if mask_ratio > 0 else 1
            assert seen == [microbatches] * stacks, (seen, microbatches)
            return tr.events
    finally:
        for k, v in old_env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def record_all():
    return {name: record(**kw) for name, kw in CONFIGS.items()}


def pack(traces):
    """{"events": distinct events, "traces": {name: indices into events}}"""
    table, index, packed = [], {}, {}
    for name, events in traces.items():
        ids = []
        for ev in events:
            key = json.dumps(ev)
            if key not in index:
                index[key] = len(table)
                table.append(ev)
            ids.append(index[key])
        packed[name] = ids
    return {"events": table, "traces": packed}


def unpack(packed):
    return {name: [packed["events"][i] for i in ids] for name, ids in packed["traces"].items()}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    traces = record_all()
    with open(out, "w") as f:
        json.dump(pack(traces), f, separators=(",", ":"))
        f.write("\n")
    print({k: len(v) for k, v in traces.items()}, os.path.getsize(out), "bytes")
