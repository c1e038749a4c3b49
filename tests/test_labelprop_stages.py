"""Label propagation over SEVERAL backbone stages in one pass: test_cfg.out_indices = (0, 1, 2) without all_blocks.

The reference's test entry point sets the backbone's out_indices / strides from the test-time config (tools/test.py:130-131); with
more than one entry ResNet.forward returns a tuple and VanillaTracker.forward_test propagates once per stage and stacks the label
maps [num_feats, T, H, W] (trackers/vanilla_tracker.py:86-93, 199-205).  Here the levels are the outputs of the listed stages of ONE
backbone pass: each level has its own h x w (stage 0 at stride 4, stages 1 and 2 at stride 8 with the test strides), its own channel
count (ResNet-18: 64 / 128 / 256), workspace and kernel choice, through forward_test, forward_test_batch (whole-clip and ring banks) and
the streaming interface, in both precisions, for label maps and soft maps."""
import os

import numpy as np
import pytest
import torch

from oracle import vfs_oracle as O
from tests.test_exact_f32 import _davis_model
from tests.test_labelprop_batch import _assert_same, _per_video, _tracker, _videos

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
STAGES = (0, 1, 2)
SIZE = (32, 48)      # 8 x 12 features at stride 4 (two query tiles), 4 x 6 at stride 8


def _set_stages(model, stages):
    """as tools/test.py:130-131: the test-time config names the stages, the backbone returns them"""
    model.test_cfg['out_indices'] = tuple(stages)
    model.backbone.out_indices = tuple(stages)
    return model


def test_forward_test_stages_equals_reference(backend):
    """fp32 forward_test with the fixture's config: [3, T, H, W], every pixel of every level the reference's.  original_shape
    (90 x 120) differs from the first-frame map's 96 x 128: levels 1 and 2 resize the map from the map already resized to 90 x 120,
    as the reference does (vanilla_tracker.py:101-104)"""
    g = np.load(os.path.join(G, 'forward_test_r18_stages.npz'))
    model, _, _ = _davis_model(backend.dev, out_indices=STAGES)
    imgs = O.fill_tensor([int(v) for v in g['imgs_shape']], int(g['imgs_seed']), scale=float(g['imgs_scale']))
    assert np.array_equal(imgs.flatten()[::997].numpy(), g['imgs_sample'])
    out_shape = tuple(int(v) for v in g['original_shape'])
    assert out_shape[:2] != g['ref_seg'].shape
    out = model(imgs.to(backend.dev), return_loss=False, ref_seg_map=torch.from_numpy(g['ref_seg'])[None], img_meta=[dict(original_shape=out_shape)])
    want = g['seg_preds']
    assert isinstance(out, list) and len(out) == 1 and out[0].dtype == np.uint8
    assert out[0].shape == want.shape == (3, imgs.shape[3]) + out_shape[:2]
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])      # the levels are different features
    agree = [float((a == b).mean()) for a, b in zip(out[0], want)]
    assert agree == [1.0, 1.0, 1.0], f'label agreement with the reference per level: {agree}'


def test_single_entry_out_indices_unchanged(backend):
    """a single entry returns the array it returned before: [T, H, W], the reference's label maps of forward_test_r18.npz"""
    g = np.load(os.path.join(G, 'forward_test_r18.npz'))
    model, _, tc = _davis_model(backend.dev)
    assert tuple(tc['out_indices']) == (2,)
    imgs = O.fill_tensor([1, 1, 3, 6, 96, 128], 41, scale=2.0)
    out = model(imgs.to(backend.dev), return_loss=False, ref_seg_map=torch.from_numpy(g['ref_seg'])[None], img_meta=[dict(original_shape=(96, 128, 3))])
    assert out[0].shape == (6, 96, 128) and np.array_equal(out[0], g['seg_preds'])


@pytest.mark.parametrize('soft', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_level_equals_single_stage_run(backend, precision, soft):
    """level i of the multi-stage result == forward_test with out_indices = (stage i,), bit for bit (original_shape = the map's own
    size: the chained resize of the first-frame map is the identity)"""
    model = _tracker(backend.dev, precision=precision, out_indices=STAGES)
    imgs_list, refs, metas = _videos([3], [SIZE], soft, backend.dev)
    multi = _per_video(model, imgs_list, refs, metas)[0]
    assert multi.shape == (3, 3) + ((refs[0].shape[1],) if soft else ()) + SIZE
    assert not np.array_equal(multi[0], multi[1]) and not np.array_equal(multi[1], multi[2])
    for i, stage in enumerate(STAGES):
        single = _per_video(_set_stages(model, (stage,)), imgs_list, refs, metas)[0]
        assert single.dtype == multi.dtype and single.shape == multi.shape[1:]
        assert np.array_equal(multi[i], single), (stage, float((multi[i] != single).mean()))


def test_levels_have_their_own_shapes_and_kernels(emu_backend):
    """ResNet-18 at 32 x 48: (8, 12, 64), (4, 6, 128), (4, 6, 256); the split copy of the two-pass kernels where two_pass_ok says so"""
    from vfs_amd.labelprop import extract_feature_levels, two_pass_ok
    model = _tracker(emu_backend.dev, out_indices=STAGES)
    imgs_list, _, _ = _videos([2], [SIZE], False, emu_backend.dev)
    banks, hls, shapes = extract_feature_levels(model, emu_backend.eng, imgs_list[0][0], 10, False, 'fp32', True)
    assert shapes == [(8, 12, 64), (4, 6, 128), (4, 6, 256)]
    assert [tuple(b.shape) for b in banks] == [(2, 96, 64), (2, 24, 128), (2, 24, 256)]
    assert [hl is not None for hl in hls] == [two_pass_ok('fp32', True, C) for _, _, C in shapes] and hls[2] is not None
    assert model.backbone.out_indices == STAGES


@pytest.mark.parametrize('ring', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_forward_test_batch_stages_equals_per_video(backend, precision, ring):
    """three videos of two lengths through two slots (a refill), class counts 2, 3 and 4: whole-clip banks and ring banks"""
    model = _tracker(backend.dev, precision=precision, out_indices=STAGES)
    imgs_list, refs, metas = _videos([3, 2, 3], [SIZE] * 3, False, backend.dev)
    assert [int(r.max()) + 1 for r in refs] == [2, 3, 4]
    want = _per_video(model, imgs_list, refs, metas)
    assert [w.shape for w in want] == [(3, T) + SIZE for T in (3, 2, 3)]
    _assert_same(model.forward_test_batch(imgs_list, refs, metas, batch=2, ring=ring), want)


def test_forward_test_batch_stages_soft_maps_and_one_frame_clip(backend):
    model = _tracker(backend.dev, out_indices=STAGES)
    imgs_list, refs, metas = _videos([2, 1, 3], [SIZE] * 3, True, backend.dev)
    want = _per_video(model, imgs_list, refs, metas)
    assert [w.shape for w in want] == [(3, T, 4) + SIZE for T in (2, 1, 3)]
    for ring in (False, True):
        _assert_same(model.forward_test_batch(imgs_list, refs, metas, batch=2, ring=ring), want)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_stream_stages_equals_forward_test(backend, precision):
    """open_stream + push one frame at a time + close == forward_test, row for row; precede_frames = 2 and 6 frames: the ring wraps"""
    model = _tracker(backend.dev, precision=precision, out_indices=STAGES)
    imgs_list, refs, metas = _videos([6], [SIZE], False, backend.dev)
    imgs, ref, meta = imgs_list[0], refs[0], metas[0]
    want = model(imgs, return_loss=False, ref_seg_map=ref, img_meta=meta)[0]
    frames = imgs[0]      # [1,3,T,H,W]
    s = model.open_stream(frames[:, :, 0], ref, meta)
    assert len(s.levels) == 3 and [tuple(lv.bank.shape[1:]) for lv in s.levels] == [(96, 64), (24, 128), (24, 256)]
    rows = [s.first] + [s.push(frames[:, :, f]) for f in range(1, 6)]
    s.close()
    assert all(r.shape == (3, 1) + SIZE for r in rows)
    got = np.concatenate(rows, axis=1)
    assert got.dtype == want.dtype and got.shape == want.shape == (3, 6) + SIZE
    assert np.array_equal(got, want), [float((a != b).mean()) for a, b in zip(got, want)]


def test_evaluator_keys_of_a_multi_stage_result(backend):
    """DavisEvaluator.evaluate on the [3, T, H, W] results: the metrics of every level under feat_0. .. feat_2."""
    import vfs_amd
    from vfs_amd import davis_eval as DE
    from vfs_amd._lib import get_lib, set_lib
    model = _tracker(backend.dev, out_indices=STAGES)
    imgs_list, refs, metas = _videos([3, 3], [SIZE] * 2, False, backend.dev)
    results = _per_video(model, imgs_list, refs, metas)
    gts = [np.repeat(r.numpy(), 3, axis=0) for r in refs]
    try:
        prev = get_lib()
    except Exception:
        prev = None
    try:
        set_lib(backend.lib)
        got = vfs_amd.DavisEvaluator(gts, device=backend.dev).evaluate(results, metrics='davis')
    finally:
        set_lib(prev)
    assert sorted(k for k in got if k.endswith('J&F-Mean')) == ['feat_0.J&F-Mean', 'feat_1.J&F-Mean', 'feat_2.J&F-Mean']
    assert {k.split('.')[0] for k in got} == {'feat_0', 'feat_1', 'feat_2'}
    assert all(f'feat_{i}.{m}' in got for i in range(3) for m in DE.G_MEASURES)
