"""Ring banks and the streaming interface of the label propagation (vfs_amd/labelprop.py): VanillaTracker.open_stream / push and
forward_test_batch(..., ring=True) == forward_test, BIT FOR BIT, from banks of precede_frames + 2 positions.

Frames of 32 x 48 (4 x 6 features of the shallow tracker of tests/test_labelprop_batch.py), precede_frames = 2 and clips of 8 frames: a
ring of 4 positions that wraps twice, frame 0 twice in the key lists of frames 1 and 2.  Ring and stream extract their frames in other
batches than forward_test (one frame, a pushed chunk, the active slots of a step against chunks of batch_step frames): that the
features do not depend on the batch a frame is extracted in is part of what these tests establish, in both precisions."""
import numpy as np
import pytest
import torch

from tests.test_labelprop_batch import _assert_same, _per_video, _tracker, _videos
from tests.test_labelprop_batch_bf16 import CountingLib
from tests.test_labelprop_batch_levels import LEVELS, _level_videos
from vfs_amd import labelprop

T, SIZE, R = 8, (32, 48), 4


def _clip(dev, soft):
    imgs_list, refs, metas = _videos([T], [SIZE], soft, dev)
    return imgs_list[0], refs[0], metas[0]


def _stream_rows(model, imgs, ref, meta, chunk, axis):
    """the clip through a stream, `chunk` frames per push -> the rows of s.first and of every push joined along the frame axis"""
    frames = imgs.reshape((-1,) + tuple(imgs.shape[2:]))      # [1,3,T,H,W]
    s = model.open_stream(frames[:, :, 0], ref, meta)
    assert s.bank_positions == R
    rows = [s.first]
    for t0 in range(1, T, chunk):
        rows.append(s.push(frames[:, :, t0] if chunk == 1 else frames[:, :, t0:t0 + chunk]))
        assert rows[-1].shape[axis] == min(chunk, T - t0)
    s.close()
    return np.concatenate(rows, axis=axis)


CONFIGS = {
    'fp32_two_pass': dict(),
    'fp32_dense': dict(),
    'bf16': dict(precision='bf16'),
    'soft': dict(),
    'no_first': dict(with_first=False),
    'first_masked': dict(with_first_neighbor=False),
    'no_norm': dict(with_norm=False),
    'all_blocks': dict(all_blocks=True),
}


@pytest.mark.parametrize('name', list(CONFIGS))
def test_stream_equals_forward_test(backend, monkeypatch, name):
    """push one frame at a time and in chunks of 3 (the last push holds one frame)"""
    if name == 'fp32_dense':
        monkeypatch.setenv('VFS_LP_TWO_PASS', '0')
    model = _tracker(backend.dev, **CONFIGS[name])
    imgs, ref, meta = _clip(backend.dev, 'soft' in name)
    want = model(imgs, return_loss=False, ref_seg_map=ref, img_meta=meta)[0]
    axis = 1 if name == 'all_blocks' else 0
    assert want.shape[axis] == T and (name != 'all_blocks' or want.shape[0] == 2)
    last = want[-1] if axis == 0 else want[0, -1]
    assert len(np.unique(last.argmax(0) if 'soft' in name else last)) > 1      # not degenerate
    for chunk in (1, 3):
        got = _stream_rows(model, imgs, ref, meta, chunk, axis)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got, want), (chunk, [float((a != b).mean()) for a, b in zip(np.moveaxis(got, axis, 0), np.moveaxis(want, axis, 0))])


def test_two_pass_configuration_uses_the_split_bank(emu_backend, monkeypatch):
    """what the two fp32 cases above run: a split copy in the stream's banks by default, none with VFS_LP_TWO_PASS=0"""
    imgs, ref, meta = _clip(emu_backend.dev, False)
    s = _tracker(emu_backend.dev).open_stream(imgs[0][:, :, 0], ref, meta)
    assert s.levels[0].hl is not None and tuple(s.levels[0].hl.shape) == (R, 24, 512)
    monkeypatch.setenv('VFS_LP_TWO_PASS', '0')
    s = _tracker(emu_backend.dev).open_stream(imgs[0][:, :, 0], ref, meta)
    assert s.levels[0].hl is None


def test_stream_buffers_do_not_grow(backend):
    model = _tracker(backend.dev)
    imgs, ref, meta = _clip(backend.dev, False)
    frames = imgs[0]
    s = model.open_stream(frames[:, :, 0], ref, meta)
    assert s.bank_positions == R == model.test_cfg['precede_frames'] + 2
    sizes = []
    for f in range(1, T):
        s.push(frames[:, :, f])
        sizes.append((s.bank_bytes, [tuple(t.shape) for lv in s.levels for t in (lv.bank, lv.hl, lv.sbank)]))
    assert sizes[2] == sizes[6] and s.bank_bytes > 0
    assert sizes[6][1] == [(R, 24, 256), (R, 24, 512), (R, 24, 2)]      # 4 x 6 features of 256 channels, 2 classes


def test_stream_argument_errors(emu_backend):
    model = _tracker(emu_backend.dev)
    imgs, ref, meta = _clip(emu_backend.dev, False)
    frames = imgs[0]
    with pytest.raises(ValueError):
        model.open_stream(frames[:, :, :2], ref, meta)      # two first frames
    s = model.open_stream(frames[:, :, :1], ref, meta)      # [1,3,1,H,W]
    with pytest.raises(ValueError):
        s.push(frames[:, :, 1, :, :40])                     # another frame size
    with pytest.raises(ValueError):
        s.push(frames[0, :, 1])                             # not [1,3,H,W]
    assert s.push(frames[:, :, 1]).shape == (1,) + SIZE
    s.close()
    with pytest.raises(ValueError):
        s.push(frames[:, :, 2])
    # the limits and the error texts are labelprop_config's, as forward_test's
    big = _tracker(emu_backend.dev, topk=11)
    with pytest.raises(NotImplementedError) as single:
        big(imgs, return_loss=False, ref_seg_map=ref, img_meta=meta)
    with pytest.raises(NotImplementedError) as stream:
        big.open_stream(frames[:, :, 0], ref, meta)
    assert str(single.value) == str(stream.value)


# ---- forward_test_batch(..., ring=True) --------------------------------------------------------------------------------------------
LENGTHS = [5, 2, 7, 1]


@pytest.mark.parametrize('precision,soft', [('fp32', False), ('bf16', False), ('fp32', True)])
def test_ring_batch_equals_per_video(backend, precision, soft):
    """two slots, refilled: the 2-frame clip makes room for the 7-frame clip, whose ring wraps; a one-frame clip"""
    model = _tracker(backend.dev, precision=precision)
    imgs_list, refs, metas = _videos(LENGTHS, [SIZE] * 4, soft, backend.dev)
    want = _per_video(model, imgs_list, refs, metas)
    assert [w.shape[0] for w in want] == LENGTHS
    _assert_same(model.forward_test_batch(imgs_list, refs, metas, batch=2, ring=True), want)


def test_ring_batch_all_blocks_equals_per_video(backend):
    """the same clips with all_blocks=True: two feature levels, each writing its own maps in place; video 0's thin object gives level 2
    (whose class counts come from level 1's map) another class count than level 1"""
    model = _tracker(backend.dev, all_blocks=True)
    imgs_list, refs, metas = _level_videos(LENGTHS, [SIZE] * 4, False, backend.dev)
    want = _per_video(model, imgs_list, refs, metas)
    assert [w.shape[:2] for w in want] == [(LEVELS, T) for T in LENGTHS]
    _assert_same(model.forward_test_batch(imgs_list, refs, metas, batch=2, ring=True), want)


def _groups(backend, precision, channels):
    """a whole-clip and a ring group of the clips above (two slots); channels: of their soft maps, None: label maps"""
    model = _tracker(backend.dev, precision=precision)
    lengths = [n for n in LENGTHS if n > 1]
    imgs_list, refs, metas = _videos(lengths, [SIZE] * 3, False, backend.dev)
    if channels:
        g = torch.Generator().manual_seed(11)
        refs = [torch.softmax(2.0 * torch.randn((1, channels) + SIZE, generator=g), dim=1) for _ in lengths]
    cfg = labelprop.labelprop_config(model)
    videos = [v.reshape((-1,) + tuple(v.shape[2:])) for v in imgs_list]
    return {ring: labelprop._Group(model, backend.eng, cfg, videos, refs, SIZE, 2, ring=ring) for ring in (False, True)}, max(lengths)


def _tensors(obj):
    return {name: t for name, t in vars(obj).items() if torch.is_tensor(t)}


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_ring_bank_shapes(emu_backend, precision):
    """the memory condition: a slot's banks hold R positions with ring=True and Tcap, the longest clip, without - R / Tcap of the bytes;
    the maps are the same in both modes, one buffer per level, so a ring group never holds more bytes than the whole-clip group - label
    maps and 16-channel soft maps alike"""
    for channels in (None, 16):
        groups, Tcap = _groups(emu_backend, precision, channels)
        for ring, frames in ((False, Tcap), (True, R)):
            (lv,) = groups[ring].levels
            assert tuple(lv.fb.shape) == (2, frames, 24, 256)
            assert (lv.hl is not None) == (precision == 'fp32') and (lv.hl is None or tuple(lv.hl.shape) == (2, frames, 24, 512))
            assert tuple(lv.sb.shape) == (2, frames * 24 * lv.COcap) and lv.COcap == (channels or 4)
            assert tuple(lv.preds.shape) == ((2, Tcap * 16 * SIZE[0] * SIZE[1]) if channels else (2, Tcap, SIZE[0] * SIZE[1]))
            assert lv.preds.dtype == (torch.float32 if channels else torch.uint8)
            # no second map buffer: these are all the tensors of a level
            assert set(_tensors(lv)) - {'hl'} == {'fb', 'sb', 'preds', 'table'} | ({'ingest'} if ring else set())
        for name in ('fb', 'hl', 'sb'):
            a, b = (getattr(groups[ring].levels[0], name) for ring in (True, False))
            assert a is None and b is None or a.numel() * Tcap == b.numel() * R      # bank bytes per slot: R / Tcap of today's
        nbytes = {ring: sum(t.numel() * t.element_size() for obj in [g] + g.levels for t in _tensors(obj).values()) for ring, g in groups.items()}
        assert nbytes[True] <= nbytes[False], (channels, nbytes)


@pytest.mark.parametrize('precision,channels', [('fp32', None), ('bf16', None), ('fp32', 4)])
def test_ring_step_issues_the_whole_clip_calls(emu_backend, monkeypatch, precision, channels):
    """a ring step makes the post-processing library calls of a whole-clip step - one per level, into the maps - and no Tensor.copy_"""
    groups, _ = _groups(emu_backend, precision, channels)
    eng, calls, copies = emu_backend.eng, {}, {}
    lib = eng.lib
    for ring, group in groups.items():
        group.admit(0)
        eng.lib = counted = CountingLib(lib)
        copied = []
        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, 'copy_', lambda *a, _copy=torch.Tensor.copy_, **k: copied.append(1) or _copy(*a, **k))
            try:
                group.step(0)
            finally:
                eng.lib = lib
        post = {k: v for k, v in counted.calls.items() if k.startswith(('seg_postprocess', 'bilinear_resize'))}
        calls[ring], copies[ring] = post, len(copied)
    name = 'bilinear_resize_f32_batch' if channels else ('seg_postprocess_batch' if precision == 'bf16' else 'seg_postprocess_exact_batch')
    assert calls[True] == calls[False] == {name: 1}
    assert copies == {False: 0, True: 0}


def test_ring_is_off_by_default(emu_backend):
    import inspect
    assert inspect.signature(type(_tracker(emu_backend.dev)).forward_test_batch).parameters['ring'].default is False
    assert inspect.signature(labelprop.forward_test_batch_hip).parameters['ring'].default is False
