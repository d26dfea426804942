"""Host-side plumbing of the augmentation on CPU with every launch stubbed out
(the harness of test_plumbing_cpu.py): TrainAugment's buffers and dict
handling, the config flags, to_device_batch and CapturedStep(transform=).
Numbers are meaningless here; test_augment_gpu.py runs the real kernels."""
import pytest
import torch

from tests.helpers import make_batch, product_config
from tests.test_plumbing_cpu import _model, stubbed_kernels


@pytest.fixture
def stub(monkeypatch):
    from mae_clip_amd import data
    with stubbed_kernels(monkeypatch) as s:
        monkeypatch.setattr(data, "_dev", lambda *ts: None)
        monkeypatch.setattr(data, "_stream", lambda: 0)
        yield s


def _raw(B=4):
    b = make_batch(B, 32)
    return {"image": torch.zeros((B, 40, 48, 3), dtype=torch.uint8),
            "image_sizes": torch.full((B, 2), 30, dtype=torch.int32),
            "input_ids": b["input_ids"], "attention_mask": b["attention_mask"], "extra": torch.zeros(B)}


def test_train_augment_reuses_its_buffers_and_passes_keys_through(stub):
    from mae_clip_amd import data
    aug = data.TrainAugment(32)
    counter = torch.zeros(1, dtype=torch.int64)
    raw = _raw()
    out = aug(raw, counter)
    assert set(out) == {"image", "input_ids", "attention_mask", "extra"} and "image_sizes" in raw
    assert out["image"].shape == (4, 32, 32, 3) and out["image"].dtype == torch.uint8
    assert out["extra"] is raw["extra"]
    assert stub.calls == ["maeclip_crop_params", "maeclip_image_augment_u8"]
    ptrs = (aug.out.data_ptr(), aug.boxes.data_ptr())
    aug(_raw(3), counter, sample_offset=3)                  # another batch size: its own buffers
    assert aug.out.shape[0] == 3
    again = aug(raw, counter)
    assert (again["image"].data_ptr(), aug.boxes.data_ptr()) == ptrs
    f32 = data.TrainAugment(32, out_dtype=torch.float32)(raw, counter)["image"]
    assert f32.shape == (4, 3, 32, 32) and f32.dtype == torch.float32
    lst = data.TrainAugment(32)({"image": [torch.zeros((9, 7, 3), dtype=torch.uint8)] * 2}, None)
    assert lst["image"].shape == (2, 32, 32, 3)


def test_wrappers_validate_shapes(stub):
    from mae_clip_amd import data
    batch = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    boxes = torch.zeros((2, 5), dtype=torch.int32)
    with pytest.raises(ValueError, match="sizes must be"):
        data.crop_params(batch, torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="padded-batch form"):
        data.crop_params([batch[0]], torch.zeros((1, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="boxes must be"):
        data.augment_images(batch, boxes[:1], 8)
    with pytest.raises(ValueError, match="boxes is required"):
        data.augment_images(batch, None, 8)
    with pytest.raises(ValueError, match="out_dtype"):
        data.augment_images(batch, boxes, 8, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="out must be"):
        data.augment_images(batch, boxes, 8, out=torch.zeros((2, 3, 8, 8)))
    with pytest.raises(ValueError, match="expected a list of images or"):
        data.augment_images(batch.float(), boxes, 8)


def test_config_flags_are_inert_by_default(stub):
    from mae_clip_amd import config as CFG, data
    assert CFG.augment is False and data.train_augment_from_config() is None
    with product_config(augment=True, size=32, augment_scale=(0.2, 1.0), augment_flip_p=0.0, augment_seed=9):
        aug = data.train_augment_from_config()
    assert (aug.size, aug.scale, aug.ratio, aug.flip_p, aug.seed) == (32, (0.2, 1.0), CFG.augment_ratio, 0.0, 9)
    assert data.TrainAugment(32).seed == CFG.augment_seed


def test_to_device_batch_with_and_without_augment(stub):
    from mae_clip_amd import data
    raw = _raw()
    args = (raw["image"], raw["input_ids"], raw["attention_mask"], "cpu")
    plain = data.to_device_batch(*args)
    assert list(plain) == ["image", "input_ids", "attention_mask"] and plain["image"].shape == (4, 3, 40, 48)
    assert stub.calls == ["maeclip_image_normalize_u8"]
    out = data.to_device_batch(*args, augment=data.TrainAugment(32), step_ptr=torch.zeros(1, dtype=torch.int64))
    assert out["image"].shape == (4, 32, 32, 3) and stub.calls[1:] == ["maeclip_crop_params",
                                                                      "maeclip_image_augment_u8"]


def test_captured_step_runs_the_transform_before_the_forward(stub, monkeypatch):
    """eager path (a graph cannot be captured without a device): the transform
    sees the raw batch, the model's step counter and offset 0, and its output is
    what the model gets; without a transform the launches are today's"""
    from mae_clip_amd import data
    from mae_clip_amd.graph import CapturedStep
    from mae_clip_amd.optim import AdamW
    seen = []
    aug = data.TrainAugment(32)
    raw = _raw()
    monkeypatch.setattr(CapturedStep, "_publish", lambda self, loss: None)

    def second_step_calls(batch, transform):
        m = _model("bf16").train()
        opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3)
        runner = CapturedStep(m, opt, enabled=False, transform=transform)
        runner.step(batch)
        del stub.calls[:]
        runner.step(batch)
        return m, list(stub.calls)

    def transform(batch, step_ptr, sample_offset):
        seen.append((batch, step_ptr, sample_offset))
        return aug(batch, step_ptr, sample_offset)
    m, with_t = second_step_calls(raw, transform)
    assert len(seen) == 2 and seen[1][0] is raw and seen[1][1] is m.step_counter and seen[1][2] == 0
    assert with_t[:2] == ["maeclip_crop_params", "maeclip_image_augment_u8"]
    fed = {"image": aug.out, "input_ids": raw["input_ids"], "attention_mask": raw["attention_mask"]}
    assert second_step_calls(fed, None)[1] == with_t[2:]
