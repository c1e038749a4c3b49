"""VanillaTracker.forward_test_batch with test_cfg.all_blocks=True (every residual block of the evaluated stage is a feature level)
== forward_test per video, for both precisions, on the batched kernels of the precision and never through forward_test.

A group holds one set of stacked banks and one descriptor table per level; the tables share the schedule and differ in the
class-count column only.  The reference chains the levels: level l + 1 starts from the map level l resized to the output size, so
a label map's class count (F.one_hot of the PIL-nearest resized map) can differ from level to level and from the map's maximum."""
import numpy as np
import pytest
import torch

from tests.test_labelprop_batch import _assert_same, _per_video, _tracker, _videos
from tests.test_labelprop_batch_bf16 import batch_calls
from vfs_amd.labelprop import pil_nearest_resize, torch_nearest_resize

LEVELS = 2      # ResNet-18 layer3


def _thin_object(H, W):
    """a label map whose highest class is one pixel column between the PIL-nearest sample points of the stride-8 feature map: the
    first level sees 3 classes where the map has 4, the second - from the map torch-nearest resized to 15/16 of the size - all 4"""
    lab = torch.zeros(H, W, dtype=torch.uint8)
    lab[H // 8:5 * H // 8, W // 10:W // 2] = 1
    lab[H // 2:15 * H // 16, 2 * W // 5:15 * W // 16] = 2
    lab[:, 8 * (W // 16) + 3] = 3
    out = (15 * H // 16, 15 * W // 16)
    first = pil_nearest_resize(lab.numpy(), H // 8, W // 8)
    second = pil_nearest_resize(torch_nearest_resize(lab.numpy(), *out), H // 8, W // 8)
    assert (int(lab.max()) + 1, int(first.max()) + 1, int(second.max()) + 1) == (4, 3, 4)
    return lab[None], out


def _level_videos(lengths, sizes, soft, dev):
    """the videos of the one-level tests; label maps: video 0 carries the thin object and every video of its frame size the output
    size that goes with it (a group is one output size)"""
    imgs_list, refs, metas = _videos(lengths, sizes, soft, dev)
    if not soft:
        refs[0], out = _thin_object(*sizes[0])
        metas = [[dict(original_shape=out + (3,))] if size == sizes[0] else m for size, m in zip(sizes, metas)]
    return imgs_list, refs, metas


def _check(backend, precision, soft, lengths, sizes, batch):
    model = _tracker(backend.dev, precision=precision, all_blocks=True)
    imgs_list, refs, metas = _level_videos(lengths, sizes, soft, backend.dev)
    want = _per_video(model, imgs_list, refs, metas)
    for w, T, ref, meta in zip(want, lengths, refs, metas):      # [levels, T, H, W] / [levels, T, CO, H, W] at the output size
        assert w.shape == (LEVELS, T) + ((ref.shape[1],) if soft else ()) + tuple(meta[0]['original_shape'][:2])
    assert any(not np.array_equal(w[0], w[1]) for w in want)      # the levels are different features
    got, calls = batch_calls(backend, model, imgs_list, refs, metas, batch)
    _assert_same(got, want)
    f32_steps, bf16_steps = calls['labelprop_f32_2pass_batch'] + calls['labelprop_f32_batch'], calls['labelprop_batch']
    mine, other = (f32_steps, bf16_steps) if precision == 'fp32' else (bf16_steps, f32_steps)
    assert mine >= LEVELS and mine % LEVELS == 0 and other == 0, dict(calls)      # one launch set per level and step
    assert calls['labelprop'] == 0 and calls['labelprop_f32'] == 0 and calls['labelprop_f32_2pass'] == 0, dict(calls)
    post = 'bilinear_resize_f32_batch' if soft else ('seg_postprocess_batch' if precision == 'bf16' else 'seg_postprocess_exact_batch')
    assert calls[post] >= LEVELS and calls['seg_postprocess'] == 0 and calls['seg_postprocess_exact'] == 0, dict(calls)
    return model, imgs_list, refs, metas, want


@pytest.mark.gpu
@pytest.mark.parametrize('soft', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_forward_test_batch_all_blocks_equals_per_video(gpu_backend, precision, soft):
    """five videos of two frame sizes through two slots: refills, a one-frame clip, the thin object (label maps)"""
    _check(gpu_backend, precision, soft, [3, 1, 5, 2, 4], [(64, 96), (64, 96), (72, 88), (64, 96), (72, 88)], 2)


@pytest.mark.parametrize('soft', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_forward_test_batch_all_blocks_small_clips_on_the_emulator(emu_backend, tmp_path, monkeypatch, precision, soft):
    """the CPU counterpart at 32 x 48 (4 x 6 features); the label maps once more with test_cfg.save_np: the paths of the levels"""
    monkeypatch.chdir(tmp_path)
    model, imgs_list, refs, metas, want = _check(emu_backend, precision, soft, [2, 1, 2], [(32, 48)] * 3, 2)
    if not soft:
        model.save_np = True
        got = model.forward_test_batch(imgs_list, refs, metas, batch=1)
        assert all(isinstance(p, list) and len(p) == LEVELS and all(q.endswith('.npy') for q in p) for p in got)
        _assert_same([np.stack([np.load(q) for q in p]) for p in got], want)
