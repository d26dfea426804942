"""World-2 data parallelism with a trainable text tower on the GPU box (two
gloo ranks on cuda:0, as tests/test_distributed_gpu.py): the ranks' result must
equal one process on the concatenated batch."""
import gc

import pytest
import torch

from tests.helpers import make_batch, record_parity, product_config, C0

pytestmark = pytest.mark.gpu

DP_B = 4   # samples per rank (tests/test_distributed_gpu.py's C0 shape)


def _dp_model():
    from mae_clip_amd.CLIP import CLIPModel
    kw = {k: v for k, v in C0.items() if k != "batch_size"}
    # a 1024-row word table (make_batch's ids are below 300) and 4 MB buckets keep the
    # host-staged gloo all-reduce and the gradients sent back to the test small
    with product_config(precision="fp32", text_trainable=True, text_vocab_size=1024, **kw):
        torch.manual_seed(0)
        m = CLIPModel()
    return m.cuda().eval()


def _dp_batch():
    return make_batch(2 * DP_B, 32, seed=3, pad=True)


def _dp_rank(rank, world, port, out):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    torch.set_num_threads(2)   # two ranks beside the test process: no oversubscribed host reductions
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mae_clip_amd import _lib
        from mae_clip_amd.distributed import DataParallel
        _lib.load()
        m = _dp_model()
        dp = DataParallel(m, bucket_mb=4.0)
        b = {k: v[rank * DP_B:(rank + 1) * DP_B].cuda() for k, v in _dp_batch().items()}
        for p in m.parameters():
            p.grad = None
        m(b).backward()
        dp.sync_gradients()
        torch.cuda.synchronize()
        text = [p for p in m.text_encoder.parameters()]
        out[rank] = dict(clip=m.last_losses["clip"].item(), mae=m.last_losses["mae"].item(), adopted=dp.adopted,
                         nparams=len(dp.params), nbuckets=len(dp.buckets),
                         text_owned=all(dp.arena.owns(p) for p in text),
                         grads={n: p.grad.cpu() for n, p in m.named_parameters() if p.requires_grad})
    finally:
        dist.destroy_process_group()


def test_text_trainable_data_parallel_equals_full_batch(dev):
    """World 2 (gloo, both ranks on the one GPU) at C0 with a trainable text
    tower, 4 ragged samples per rank, vs one process on the 8 concatenated
    samples, fp32 parity mode, with the bounds of
    test_distributed_gpu.test_product_data_parallel_equals_full_batch: the
    local-row CLIP gradient into TextStackFn, the arena slots of every text
    gradient (the word table's among them) and their SUM all-reduce."""
    import torch.multiprocessing as mp
    from tests.test_plumbing_cpu import _free_port
    gc.collect()   # the manager process is forked from this one: drop what earlier tests left behind
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_dp_rank, args=(2, _free_port(), out), nprocs=2, join=True)
    res = [out[r] for r in range(2)]
    m = _dp_model()
    m({k: v.to(dev) for k, v in _dp_batch().items()}).backward()
    ref_clip, ref_mae = m.last_losses["clip"].item(), m.last_losses["mae"].item()
    for o in res:
        assert abs(o["clip"] - ref_clip) < 1e-5 * max(1.0, abs(ref_clip)), (o["clip"], ref_clip)
        assert o["adopted"] == o["nparams"], (o["adopted"], o["nparams"])
        assert o["text_owned"] and o["nbuckets"] >= 2
    assert abs((res[0]["mae"] + res[1]["mae"]) / 2 - ref_mae) < 1e-5 * max(1.0, abs(ref_mae))
    worst, ntext = (0.0, None), 0
    for n, p in m.named_parameters():
        if not p.requires_grad:
            continue
        ntext += n.startswith("text_encoder.")
        g = p.grad.cpu()
        sc = g.abs().max().item() + 1e-30
        for o in res:
            e = (o["grads"][n] - g).abs().max().item() / sc
            worst = max(worst, (e, n))
            assert e < 1e-4, (n, e)
        assert torch.equal(res[0]["grads"][n], res[1]["grads"][n]), n
    assert ntext == len(list(m.text_encoder.parameters())) > 0
    record_parity("dp2_gloo_C0_text_trainable_vs_single_process",
                  clip_rel=abs(res[0]["clip"] - ref_clip) / max(1.0, ref_clip), worst_grad_maxrel=worst[0],
                  worst_grad=worst[1])
