"""Trainable text tower (TextEncoder(trainable=True), config.text_trainable) on
the host side: construction, parameter flags, state_dict keys, and -- with
every kernel launch stubbed out as in test_plumbing_cpu.py -- a training step
through functions.TextStackFn and the data-parallel gradient arena. Numbers
from stubbed launches are meaningless; shapes, call sequences and gradient
ownership are what is checked. The real-kernel tests are
test_text_kernels_gpu.py / test_text_trainable_gpu.py."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.helpers import product_config, make_batch, C0
from tests.test_plumbing_cpu import stubbed_kernels, _free_port


def _model(precision, **over):
    from mae_clip_amd.CLIP import CLIPModel
    kw = {k: v for k, v in C0.items() if k != "batch_size"}
    kw.update(over)
    with product_config(precision=precision, side_stream=False, **kw):
        torch.manual_seed(0)
        return CLIPModel()


def test_text_encoder_trainable_constructs():
    from mae_clip_amd.modules import TextEncoder
    with product_config(text_layers=2):
        frozen = TextEncoder()
        enc = TextEncoder(trainable=True)
    assert enc.model.trainable and not frozen.model.trainable
    assert all(p.requires_grad for p in enc.parameters())
    assert not any(p.requires_grad for p in frozen.parameters())
    assert list(enc.state_dict().keys()) == list(frozen.state_dict().keys())
    # the reference's positional order: (model_name, pretrained, trainable)
    with product_config(text_layers=1):
        assert TextEncoder("distilbert-base-uncased", False, True).model.trainable


def test_config_text_trainable_reaches_clip_model():
    from mae_clip_amd import config as CFG
    assert CFG.text_trainable is False
    m = _model("bf16")
    assert not any(p.requires_grad for p in m.text_encoder.parameters())
    mt = _model("bf16", text_trainable=True)
    assert all(p.requires_grad for p in mt.text_encoder.parameters())
    assert list(mt.state_dict().keys()) == list(m.state_dict().keys())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_trainable_text_step_plumbing(monkeypatch, precision):
    from mae_clip_amd.optim import AdamW
    with stubbed_kernels(monkeypatch) as stub:
        m = _model(precision, text_trainable=True).train()
        opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3)
        for B, pad in ((8, False), (5, True)):
            opt.zero_grad(set_to_none=True)
            del stub.calls[:]
            loss = m(make_batch(B, 32, pad=pad))
            loss.backward()
            for n, p in m.text_encoder.named_parameters():
                assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32, n
                assert p.grad.is_contiguous(), n
            opt.step()
            layers = len(m.text_encoder.model.transformer.layer)
            assert stub.calls.count("maeclip_embed_bwd") == 1
            # one masked + dropout attention backward per text layer (the image stacks add theirs)
            assert stub.calls.count("maeclip_attn_bwd") >= layers
        assert len(opt.state) == sum(1 for p in m.parameters() if p.requires_grad)


def test_trainable_text_standalone_encoder_plumbing(monkeypatch):
    """TextEncoder(trainable=True) outside CLIPModel: its own WeightCache."""
    from mae_clip_amd.modules import TextEncoder
    with stubbed_kernels(monkeypatch):
        with product_config(precision="bf16", text_layers=2, side_stream=False):
            enc = TextEncoder(trainable=True).train()
        b = make_batch(3, 32, pad=True)
        out = enc(b["input_ids"], b["attention_mask"])
        assert out.shape == (3, 768) and out.requires_grad
        out.sum().backward()
        assert all(p.grad is not None and p.grad.shape == p.shape for p in enc.parameters())


def _dp_rank(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mp_ = pytest.MonkeyPatch()
        with stubbed_kernels(mp_):
            from mae_clip_amd.distributed import DataParallel
            m = _model("bf16", text_trainable=True).train()
            dp = DataParallel(m, bucket_mb=0.5)
            for _ in range(2):
                for p in m.parameters():
                    p.grad = None
                dp.reset_stats()
                m(make_batch(4, 32, seed=rank, pad=True)).backward()
                dp.sync_gradients()
            text = list(m.text_encoder.parameters())
            in_dp = {id(p) for p in dp.params}
            out[rank] = (dp.adopted, len(dp.params), all(id(p) in in_dp for p in text),
                         all(dp.arena.owns(p) for p in text))
        mp_.undo()
    finally:
        dist.destroy_process_group()


def test_trainable_text_data_parallel_arena():
    """Two gloo ranks: every text-tower gradient is produced in its GradArena slot."""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_dp_rank, args=(2, _free_port(), out), nprocs=2, join=True)
    for r in range(2):
        adopted, nparams, listed, owned = out[r]
        assert listed and owned
        assert adopted == nparams, (adopted, nparams)
