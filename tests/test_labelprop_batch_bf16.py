"""Lock-step label propagation with the bf16 kernels (csrc/labelprop.hip: vfs_labelprop_batch, vfs_seg_postprocess_batch) == the
single-video calls vfs_labelprop / vfs_seg_postprocess on every slot's own banks, BIT FOR BIT, and
VanillaTracker.forward_test_batch(precision='bf16') == forward_test per video - on the batched kernels, never through forward_test.

The single-video bf16 calls are pinned to their float64 references by tests/test_labelprop_exact.py, so they are the yardstick here.
The batched launches run the single-video kernel bodies; what is at stake is the plumbing: slot strides of the banks, descriptor
rows, class counts packed per slot, the key-frame split of every slot (the bf16 top-k keeps the first of equal scores, so the split
belongs to the result), a grid sized for the slot with the most key frames, inactive slots."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from tests.test_labelprop_batch import _assert_same, _desc_rows, _features, _per_video, _tracker, _videos, check_map_positions, same_bits

TEMP = 0.07


class Batch16:
    """stacked bf16 banks of `nslots` slots in the layout of include/vfs_hip.h; label rows packed per slot with the slot's class count"""

    def __init__(self, lib, nslots, Tcap, H, W, C, COcap):
        self.lib, self.N, self.Tcap, self.H, self.W, self.C, self.COcap = lib, nslots, Tcap, H, W, C, COcap
        self.fb = torch.zeros(nslots, Tcap, H * W, C, dtype=torch.bfloat16)
        self.sb = torch.full((nslots, Tcap * H * W * COcap), float('nan'))
        self.videos = {}

    def put(self, n, feats, seg):
        T, HW, C = feats.shape
        self.lib.l2norm_rows(feats.reshape(-1, C).to(torch.bfloat16).contiguous(), self.fb[n, :T], T * HW, C, None)
        CO = seg.shape[-1]
        self.sb[n, :T * HW * CO] = seg.reshape(-1)
        self.videos[n] = (T, CO, seg.clone())

    def rows(self, n, frame):
        CO, HW = self.videos[n][1], self.H * self.W
        return self.sb[n, frame * HW * CO:(frame + 1) * HW * CO].reshape(HW, CO)

    def workspace(self):
        nb = torch.zeros(1, dtype=torch.int64)
        self.lib.labelprop_batch_workspace_bytes(self.H, self.W, self.N, nb)
        return torch.zeros((int(nb.item()) + 3) // 4), int(nb.item())

    def single(self, n, qframe, keys, radius, topk, nml):
        """vfs_labelprop on slot n's own banks"""
        T, CO, seg = self.videos[n]
        lib, H, W = self.lib, self.H, self.W
        nb = torch.zeros(1, dtype=torch.int64)
        lib.labelprop_workspace_bytes(H, W, nb)
        ws = torch.zeros((int(nb.item()) + 3) // 4)
        out = torch.full((H * W, CO), float('nan'))
        ks = (ctypes.c_int * len(keys))(*keys)
        lib.labelprop(self.fb[n, :T].contiguous(), seg, out, ws, ws.numel() * 4, qframe, ks, len(keys), H, W, self.C, CO, radius, nml, topk, TEMP, None)
        assert torch.isfinite(out).all()
        return out


def _check_slots(b, rows, radius, topk, run):
    """rows {slot: (qframe, keys, non_mask_len, CO)}: after run(desc) every row's slot holds the bits of its single-video call in its
    query frame, and nothing else of the label rows has changed (the other frames, the padding, the slots without a row: all as before)"""
    for n, (q, keys, nml, CO) in rows.items():
        b.rows(n, q).fill_(float('nan'))
    before = b.sb.clone()
    run(_desc_rows(b.N, rows))
    for n, (q, keys, nml, CO) in rows.items():
        want = b.single(n, q, keys, radius, topk, nml).numpy()
        got = b.rows(n, q).numpy()
        assert same_bits(got, want), (n, float(np.nanmax(np.abs(got - want))))
        before[n, q * b.H * b.W * CO:(q + 1) * b.H * b.W * CO] = b.rows(n, q).reshape(-1)
    assert np.array_equal(b.sb.numpy().view(np.uint32), before.numpy().view(np.uint32))


def _four_slots(lib, H, W, C, seed):
    """0 = duplicated first frame (exact ties), 1 = five keys, 2 = inactive, 3 = one key; 5, 3 and 2 classes inside COcap = 5"""
    b = Batch16(lib, 4, 6, H, W, C, 5)
    for n, T, CO in ((0, 4, 5), (1, 6, 3), (3, 2, 2)):
        b.put(n, *_features(T, H * W, C, CO, seed + n))
    return b, {0: (3, [0, 0, 1, 2]), 1: (5, [0, 1, 2, 3, 4]), 3: (1, [0])}


@pytest.mark.parametrize('C', [64, 128])
@pytest.mark.parametrize('H,W,radius,topk', [(9, 13, 3, 10), (8, 8, 0, 5)])
@pytest.mark.parametrize('nml', [0, 1])
def test_batched_bf16_kernel_equals_single_video(backend, H, W, radius, topk, nml, C):
    lib = backend.hostlib
    b, plan = _four_slots(lib, H, W, C, seed=70)
    ws, nbytes = b.workspace()
    # (a single video refuses non_mask_len = nkeys under a spatial mask: the one-key slot keeps 0)
    rows = {n: (q, keys, nml if (len(keys) > 1 or radius <= 0) else 0, b.videos[n][1]) for n, (q, keys) in plan.items()}

    def run(desc):
        lib.labelprop_batch(b.fb, b.sb, ws, nbytes, desc, 4, 3, 5, 6, H, W, C, 5, radius, topk, TEMP, None)
    _check_slots(b, rows, radius, topk, run)
    assert torch.isnan(b.sb[2]).all()


def test_every_slot_splits_its_own_key_frames(backend):
    """9 x 13 is four query tiles: 26 key frames (above the 24 splits a launch may have) go two to a workgroup in 13 splits, three key
    frames one to a workgroup.  Frame 0 is duplicated in both slots: ties, whose order follows the split.  The grid is sized for the
    26; the three-key slot must still use ITS split, and its merge must read three partial lists, not thirteen"""
    lib = backend.hostlib
    H, W, C = 9, 13, 64
    b = Batch16(lib, 2, 8, H, W, C, 3)
    b.put(0, *_features(8, H * W, C, 3, 80))
    b.put(1, *_features(3, H * W, C, 2, 81))
    rows = {0: (7, [0, 0] + [1, 2, 3, 4, 5, 6] * 4, 0, 3), 1: (2, [0, 0, 1], 0, 2)}
    assert len(rows[0][1]) == 26
    ws, nbytes = b.workspace()
    ws.fill_(float('nan'))      # stale partial lists: a merge that read beyond its slot's splits would show

    def run(desc):
        lib.labelprop_batch(b.fb, b.sb, ws, nbytes, desc, 2, 2, 26, 8, H, W, C, 3, 3, 10, TEMP, None)
    _check_slots(b, rows, 3, 10, run)


def test_batched_bf16_postprocessing(backend):
    """the slots of the kernel test (5, 3, - and 2 classes inside COcap = 5; query frames 3, 5, -, 1), 9 x 13 -> 37 x 50: label maps
    byte-equal to seg_postprocess per slot (class 1 of slot 1 is <= 0 throughout: not normalised); every other byte of preds stays"""
    lib = backend.hostlib
    H, W, Ho, Wo, Tcap, COcap = 9, 13, 37, 50, 6, 5
    HW = H * W
    plan = {0: (3, 5), 1: (5, 3), 3: (1, 2)}      # slot: (query frame, classes)
    g = torch.Generator().manual_seed(90)
    sb = torch.full((4, Tcap * HW * COcap), float('nan'))
    segs = {}
    for n, (q, CO) in plan.items():
        seg = torch.randn(HW, CO, generator=g)
        if n == 1:
            seg[:, 1] = -seg[:, 1].abs()
            seg[0, 1] = 0.0
        segs[n] = seg
        sb[n, q * HW * CO:(q + 1) * HW * CO] = seg.reshape(-1)
    desc = _desc_rows(4, {n: (q, [0], 0, CO) for n, (q, CO) in plan.items()})
    preds = torch.full((4, Tcap, Ho * Wo), 255, dtype=torch.uint8)
    partial = torch.zeros(4, 64, COcap, 2)
    lib.seg_postprocess_batch(sb, partial, preds, desc, 4, Tcap, Tcap, H, W, COcap, Ho, Wo, None)
    want = torch.full_like(preds, 255)
    for n, (q, CO) in plan.items():
        lab = torch.zeros(Ho * Wo, dtype=torch.uint8)
        lib.seg_postprocess(segs[n], torch.zeros(64 * CO * 2), lab, H, W, CO, Ho, Wo, None)
        assert len(set(lab.tolist())) > 1
        want[n, q] = lab
    assert torch.equal(preds, want)


def test_batched_bf16_postprocessing_map_positions(backend):
    """label rows at one position, the map at another (descriptor column 5), against vfs_seg_postprocess"""
    check_map_positions(backend.hostlib, backend.hostlib.seg_postprocess_batch, backend.hostlib.seg_postprocess)


def test_bf16_batch_arguments_and_invalid_rows(emu_backend):
    """the host-side refusals return their error and write nothing; a row outside the single-video ranges sits the step out while its
    valid neighbour is computed"""
    from vfs_amd._lib import VfsError
    lib = emu_backend.hostlib
    H, W, C = 8, 8, 64
    b = Batch16(lib, 2, 3, H, W, C, 3)
    for n in range(2):
        b.put(n, *_features(3, H * W, C, 3, 100 + n))
    ws, nbytes = b.workspace()
    good = (2, [0, 1], 0, 3)
    desc = _desc_rows(2, {0: good, 1: good})
    before = b.sb.clone()
    wide = torch.zeros(2, 3, H * W, 96, dtype=torch.bfloat16)
    for what, code, args in (('C', -1, (wide, b.sb, ws, nbytes, desc, 2, 2, 2, 3, H, W, 96, 3, 3, 10, TEMP, None)),
                             ('topk', -1, (b.fb, b.sb, ws, nbytes, desc, 2, 2, 2, 3, H, W, C, 3, 3, 11, TEMP, None)),
                             ('nslots 0', -1, (b.fb, b.sb, ws, nbytes, desc, 0, 0, 2, 3, H, W, C, 3, 3, 10, TEMP, None)),
                             ('nslots 65', -1, (b.fb, b.sb, ws, nbytes, desc, 65, 2, 2, 3, H, W, C, 3, 3, 10, TEMP, None)),
                             ('max_nkeys', -1, (b.fb, b.sb, ws, nbytes, desc, 2, 2, 65, 3, H, W, C, 3, 3, 10, TEMP, None)),
                             ('workspace', -3, (b.fb, b.sb, ws, nbytes - 1, desc, 2, 2, 2, 3, H, W, C, 3, 3, 10, TEMP, None))):
        with pytest.raises(VfsError, match=rf'failed \({code}\)'):      # csrc/vfs_common.h: VFS_ERR_SHAPE -1, VFS_ERR_ARG -3
            lib.labelprop_batch(*args)
        assert np.array_equal(b.sb.numpy().view(np.uint32), before.numpy().view(np.uint32)), what
    nb = torch.zeros(1, dtype=torch.int64)
    for nslots in (0, 65):
        with pytest.raises(VfsError, match=r'failed \(-3\)'):
            lib.labelprop_batch_workspace_bytes(H, W, nslots, nb)
    want = b.single(0, 2, [0, 1], 3, 10, 0).numpy()
    for bad in ((3, [0, 1], 0, 3), (2, [0, 3], 0, 3)):      # qframe >= Tcap, a key frame >= Tcap
        b.rows(0, 2).fill_(float('nan'))
        lib.labelprop_batch(b.fb, b.sb, ws, nbytes, _desc_rows(2, {0: good, 1: bad}), 2, 2, 2, 3, H, W, C, 3, 3, 10, TEMP, None)
        assert np.array_equal(b.sb[1].numpy().view(np.uint32), before[1].numpy().view(np.uint32)), bad
        assert same_bits(b.rows(0, 2).numpy(), want), bad


# ---- tracker level: VanillaTracker.forward_test_batch(precision='bf16') == forward_test, video by video, on the batched kernels -------
class CountingLib:
    """the engine's library with every entry point counted by name"""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        attr = getattr(self._lib, name)
        if not callable(attr):
            return attr

        def call(*args):
            self.calls[name] += 1
            return attr(*args)
        return call


def batch_calls(backend, model, imgs_list, refs, metas, batch):
    """forward_test_batch with the engine's library counted -> (results, calls by entry point)"""
    eng = backend.eng
    lib = eng.lib
    eng.lib = counted = CountingLib(lib)
    try:
        got = model.forward_test_batch(imgs_list, refs, metas, batch=batch)
    finally:
        eng.lib = lib
    return got, counted.calls


def _assert_batched_bf16(calls, soft):
    assert calls['labelprop_batch'] >= 1 and calls['labelprop'] == 0, dict(calls)
    assert calls['labelprop_f32_batch'] == 0 and calls['labelprop_f32_2pass_batch'] == 0 and calls['labelprop_f32'] == 0, dict(calls)
    if soft:
        assert calls['bilinear_resize_f32_batch'] >= 1 and calls['seg_postprocess_batch'] == 0, dict(calls)
    else:
        assert calls['seg_postprocess_batch'] >= 1 and calls['seg_postprocess'] == 0 and calls['seg_postprocess_exact_batch'] == 0, dict(calls)


@pytest.mark.gpu
@pytest.mark.parametrize('soft', [False, True])
def test_forward_test_batch_bf16_equals_per_video(gpu_backend, soft):
    """five videos of two frame sizes through two slots: refills, a one-frame clip on its own path; class counts differ (3-D maps)"""
    model = _tracker(gpu_backend.dev, precision='bf16')
    lengths = [3, 1, 5, 2, 4]
    sizes = [(64, 96), (64, 96), (72, 88), (64, 96), (72, 88)]
    imgs_list, refs, metas = _videos(lengths, sizes, soft, gpu_backend.dev)
    want = _per_video(model, imgs_list, refs, metas)
    assert [w.shape[0] for w in want] == lengths
    assert all(len(np.unique(w[-1] if not soft else w[-1].argmax(0))) > 1 for w in want)      # not degenerate
    got, calls = batch_calls(gpu_backend, model, imgs_list, refs, metas, 2)
    _assert_same(got, want)
    _assert_batched_bf16(calls, soft)


@pytest.mark.parametrize('soft', [False, True])
def test_forward_test_batch_bf16_small_clips_on_the_emulator(emu_backend, tmp_path, monkeypatch, soft):
    """the CPU counterpart: 32 x 48 frames (4 x 6 features), two clips of two frames and a one-frame clip; the label maps once more
    with test_cfg.save_np, honoured as forward_test does"""
    monkeypatch.chdir(tmp_path)
    model = _tracker(emu_backend.dev, precision='bf16')
    imgs_list, refs, metas = _videos([2, 1, 2], [(32, 48)] * 3, soft, emu_backend.dev)
    want = _per_video(model, imgs_list, refs, metas)
    got, calls = batch_calls(emu_backend, model, imgs_list, refs, metas, 2)
    _assert_same(got, want)
    _assert_batched_bf16(calls, soft)
    if not soft:
        model.save_np = True
        got, calls = batch_calls(emu_backend, model, imgs_list, refs, metas, 1)
        assert all(isinstance(p, str) and p.endswith('.npy') for p in got)
        _assert_same([np.load(p) for p in got], want)
        _assert_batched_bf16(calls, soft)
