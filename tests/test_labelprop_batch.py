"""Label propagation of a batch of videos in lock-step: the batched kernels (csrc/labelprop2.hip, csrc/exact_f32.hip: a slot
dimension on the grids, per-slot arguments from a descriptor row) == the single-video calls == oracle/exact_oracle.c, BIT FOR BIT,
and VanillaTracker.forward_test_batch == forward_test per video.

The batched launches run the single-video kernel bodies, so what is at stake is the plumbing: slot strides of the banks, the rows of
the descriptor table, class counts packed per slot, grids sized for the slot with the most key frames, per-slot workspace and
overflow words, inactive slots."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import exact_oracle as X

DESC = 72      # include/vfs_hip.h VFS_LPB_DESC_INTS


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _features(T, HW, C, CO, seed, smooth=0.0):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(T, HW, C, generator=g)
    feats = feats + 2.0 * torch.randn(1, 1, C, generator=g) + torch.linspace(0, 3, HW)[None, :, None] * torch.randn(1, 1, C, generator=g)
    if smooth:
        feats = feats.abs() + smooth
    return feats, torch.rand(T, HW, CO, generator=g)


def _desc_rows(nslots, rows):
    """rows: {slot: (qframe, key frames, non_mask_len, CO[, map position: qframe])}; the other slots are inactive"""
    d = torch.zeros(nslots, DESC, dtype=torch.int32)
    for n, (qframe, keys, nml, CO, *mpos) in rows.items():
        d[n, 0], d[n, 1], d[n, 2], d[n, 3], d[n, 4], d[n, 5] = 1, qframe, len(keys), nml, CO, (mpos[0] if mpos else qframe)
        d[n, 8:8 + len(keys)] = torch.tensor(keys, dtype=torch.int32)
    return d


class Batch:
    """stacked banks of `nslots` slots in the layout of include/vfs_hip.h; label rows packed per slot with the slot's class count"""

    def __init__(self, lib, nslots, Tcap, H, W, C, COcap, two_pass):
        self.lib, self.N, self.Tcap, self.H, self.W, self.C, self.COcap = lib, nslots, Tcap, H, W, C, COcap
        HW = H * W
        self.fb = torch.zeros(nslots, Tcap, HW, C)
        self.hl = torch.zeros(nslots, Tcap, HW, 2 * C, dtype=torch.bfloat16) if two_pass else None
        self.sb = torch.full((nslots, Tcap * HW * COcap), float('nan'))
        self.videos = {}

    def put(self, n, feats, seg):
        T, HW, C = feats.shape
        self.lib.l2norm_rows_f32(feats.reshape(-1, C).contiguous(), self.fb[n, :T], T * HW, C, None)
        if self.hl is not None:
            self.lib.split_rows_bf16x2(self.fb[n, :T], self.hl[n, :T], T * HW, C, None)
        CO = seg.shape[-1]
        self.sb[n, :T * HW * CO] = seg.reshape(-1)
        self.videos[n] = (T, CO, seg.clone())

    def rows(self, n, frame):
        T, CO, _ = self.videos[n]
        HW = self.H * self.W
        return self.sb[n, frame * HW * CO:(frame + 1) * HW * CO].reshape(HW, CO)

    def single(self, n, qframe, keys, radius, topk, nml, dense=False):
        """the single-video call and the C oracle on slot n's own banks"""
        T, CO, seg = self.videos[n]
        lib, H, W = self.lib, self.H, self.W
        nb = torch.zeros(1, dtype=torch.int64)
        lib.labelprop_f32_2pass_workspace_bytes(H, W, nb)
        ws = torch.zeros((int(nb.item()) + 3) // 4)
        out = torch.full((H * W, CO), float('nan'))
        ks = (ctypes.c_int * len(keys))(*keys)
        fb = self.fb[n, :T].contiguous()
        if dense:
            lib.labelprop_f32(fb, seg, out, ws, ws.numel() * 4, qframe, ks, len(keys), H, W, self.C, CO, radius, nml, topk, 0.07, None)
        else:
            lib.labelprop_f32_2pass(fb, self.hl[n, :T].contiguous(), seg, out, ws, ws.numel() * 4, qframe, ks, len(keys), H, W, self.C, CO, radius,
                                    nml, topk, 0.07, 1, None)
        want = X.labelprop(fb.numpy(), seg.numpy(), qframe, keys, H, W, radius, topk, 0.07, non_mask_len=nml)
        flag = int(ws.view(torch.int32)[(int(nb.item()) - 16) // 4])
        return out, want, flag


def _four_slots(lib, H, W, C, two_pass, seed):
    """the slots of the issue: 0 = duplicated first frame (exact ties), 1 = five keys, 2 = inactive, 3 = one key"""
    b = Batch(lib, 4, 6, H, W, C, 5, two_pass)
    for n, T, CO in ((0, 4, 5), (1, 6, 3), (3, 2, 2)):
        b.put(n, *_features(T, H * W, C, CO, seed + n))
    plan = {0: (3, [0, 0, 1, 2]), 1: (5, [0, 1, 2, 3, 4]), 3: (1, [0])}
    return b, plan


def _check_four_slots(b, plan, radius, topk, nml_for, run, dense):
    cos = {n: b.videos[n][1] for n in plan}
    # (a single video refuses non_mask_len = nkeys under a spatial mask: the one-key slot keeps 0)
    rows = {n: (q, keys, nml_for(len(keys)), cos[n]) for n, (q, keys) in plan.items()}
    for n, (q, keys, nml, CO) in rows.items():
        b.rows(n, q).fill_(float('nan'))
    before = b.sb.clone()
    run(_desc_rows(4, rows))
    for n, (q, keys, nml, CO) in rows.items():
        out, want, _ = b.single(n, q, keys, radius, topk, nml, dense=dense)
        got = b.rows(n, q).numpy()
        assert same_bits(want, out.numpy()), n
        assert same_bits(got, out.numpy()) and same_bits(got, want), (n, float(np.nanmax(np.abs(got - want))))
        before[n, q * b.H * b.W * CO:(q + 1) * b.H * b.W * CO] = b.rows(n, q).reshape(-1)
    # nothing else was written: the inactive slot (all NaN), the other frames, the padding behind the packed rows
    assert np.array_equal(b.sb.numpy().view(np.uint32), before.numpy().view(np.uint32))
    assert torch.isnan(b.sb[2]).all()


@pytest.mark.parametrize('nml', [0, 1])
def test_batched_two_pass_equals_single_and_oracle(backend, nml):
    lib = backend.hostlib
    H, W, C = 9, 13, 256
    b, plan = _four_slots(lib, H, W, C, True, seed=20)
    nb = torch.zeros(1, dtype=torch.int64)
    lib.labelprop_f32_2pass_batch_workspace_bytes(H, W, 0, 4, nb)
    ws = torch.zeros((int(nb.item()) + 3) // 4)

    def run(desc):
        lib.labelprop_f32_2pass_batch(b.fb, b.hl, b.sb, ws, ws.numel() * 4, desc, 4, 3, 5, 6, H, W, C, 5, 3, 10, 0.07, 1, None)
    _check_four_slots(b, plan, 3, 10, lambda nk: nml if nk > 1 else 0, run, dense=False)
    assert ws.view(torch.int32)[:4].tolist() == [0, 0, 0, 0]      # no slot overflowed: the two-pass kernels produced these bits


@pytest.mark.parametrize('H,W,radius,topk', [(9, 13, 3, 10), (8, 8, 0, 5)])
@pytest.mark.parametrize('nml', [0, 1])
def test_batched_dense_kernel(backend, H, W, radius, topk, nml):
    """C = 64 is not two-pass eligible: the dense kernels, through their own entry point and through the two-pass entry point"""
    lib = backend.hostlib
    C = 64
    b, plan = _four_slots(lib, H, W, C, False, seed=30)
    nb = torch.zeros(1, dtype=torch.int64)
    lib.labelprop_f32_batch_workspace_bytes(H, W, 4, nb)
    ws = torch.zeros((int(nb.item()) + 3) // 4)
    nml_for = (lambda nk: nml if (nk > 1 or radius <= 0) else 0)

    def run(desc):
        lib.labelprop_f32_batch(b.fb, b.sb, ws, ws.numel() * 4, desc, 4, 3, 5, 6, H, W, C, 5, radius, topk, 0.07, None)
    _check_four_slots(b, plan, radius, topk, nml_for, run, dense=True)
    lib.labelprop_f32_2pass_batch_workspace_bytes(H, W, 16, 4, nb)
    ws2 = torch.zeros((int(nb.item()) + 3) // 4)

    def run2(desc):
        lib.labelprop_f32_2pass_batch(b.fb, None, b.sb, ws2, ws2.numel() * 4, desc, 4, 3, 5, 6, H, W, C, 5, radius, topk, 0.07, 1, None)
    _check_four_slots(b, plan, radius, topk, nml_for, run2, dense=True)


def test_overflow_and_dense_redo_are_per_slot(backend):
    """a list capacity of 16 entries per (split, query), as tests/test_labelprop2.py forces its fallback.  Slot 1 has the crowded scores
    that overflow it; slots 0 and 2 are video-like (eleven nearly identical key frames: the seeded threshold sits just under the
    query's own position in every key frame, a handful of candidates pass it).  Only slot 1 is redone by the dense kernels."""
    lib = backend.hostlib
    H, W, C = 12, 16, 256
    HW = H * W
    b = Batch(lib, 3, 12, H, W, C, 4, True)
    for n in (0, 2):
        g = torch.Generator().manual_seed(40 + n)
        base = torch.randn(1, HW, C, generator=g)
        b.put(n, base + 0.05 * torch.randn(12, HW, C, generator=g), torch.rand(12, HW, 2 + n, generator=g))
    b.put(1, *_features(4, HW, C, 3, 5, smooth=4.0))
    plan = {0: (11, list(range(11))), 1: (3, [0, 1, 2]), 2: (11, list(range(11)))}
    rows = {n: (q, keys, 0, b.videos[n][1]) for n, (q, keys) in plan.items()}
    nb = torch.zeros(1, dtype=torch.int64)
    lib.labelprop_f32_2pass_batch_workspace_bytes(H, W, 0, 3, nb)
    ws = torch.zeros((int(nb.item()) + 3) // 4)
    try:
        lib.set_option(b'lp2_cap', 16)
        singles = {n: b.single(n, q, keys, 5, 10, 0) for n, (q, keys) in plan.items()}
        assert [singles[n][2] for n in range(3)] == [0, 1, 0]      # the precondition, by the single-video call's own flag
        for n, (q, keys, nml, CO) in rows.items():
            b.rows(n, q).fill_(float('nan'))
        lib.labelprop_f32_2pass_batch(b.fb, b.hl, b.sb, ws, ws.numel() * 4, _desc_rows(3, rows), 3, 3, 11, 12, H, W, C, 4, 5, 10, 0.07, 1, None)
    finally:
        lib.set_option(b'lp2_cap', 0)
    assert ws.view(torch.int32)[:3].tolist() == [0, 1, 0]
    for n, (q, keys, nml, CO) in rows.items():
        assert same_bits(b.rows(n, q).numpy(), singles[n][1]), n
        assert same_bits(singles[n][0].numpy(), singles[n][1]), n


def test_batched_postprocessing(backend):
    """three slots with 2, 5 and 3 classes inside COcap = 5, 8 x 12 -> 31 x 45: label maps byte-equal to seg_postprocess_exact per slot
    (per-class min / max, normalised where max > 0 - class 1 of slot 1 is negative throughout -, argmax, up-sampling), soft maps
    bit-equal to bilinear_resize_f32 per slot; the frames that are not a slot's query frame stay as they were"""
    lib = backend.hostlib
    H, W, Ho, Wo, Tcap, COcap = 8, 12, 31, 45, 3, 5
    HW = H * W
    cos, qf = [2, 5, 3], [1, 2, 0]
    g = torch.Generator().manual_seed(50)
    sb = torch.full((3, Tcap * HW * COcap), float('nan'))
    segs = []
    for n in range(3):
        seg = torch.randn(HW, cos[n], generator=g)
        if n == 1:
            seg[:, 1] = -seg[:, 1].abs() - 0.1
        segs.append(seg)
        sb[n, qf[n] * HW * cos[n]:(qf[n] + 1) * HW * cos[n]] = seg.reshape(-1)
    desc = _desc_rows(3, {n: (qf[n], [0], 0, cos[n]) for n in range(3)})
    preds = torch.full((3, Tcap, Ho * Wo), 255, dtype=torch.uint8)
    partial = torch.zeros(3, 64, COcap, 2)
    lib.seg_postprocess_exact_batch(sb, partial, preds, desc, 3, Tcap, Tcap, H, W, COcap, Ho, Wo, None)
    soft = torch.full((3, Tcap * COcap * Ho * Wo), float('nan'))
    lib.bilinear_resize_f32_batch(sb, soft, desc, 3, Tcap, Tcap, H, W, COcap, Ho, Wo, None)
    for n in range(3):
        lab = torch.zeros(Ho * Wo, dtype=torch.uint8)
        lib.seg_postprocess_exact(segs[n], torch.zeros(64 * cos[n] * 2), lab, H, W, cos[n], Ho, Wo, None)
        assert len(set(lab.tolist())) > 1
        assert torch.equal(preds[n, qf[n]], lab), n
        others = [f for f in range(Tcap) if f != qf[n]]
        assert (preds[n, others] == 255).all()
        up = torch.zeros(cos[n], Ho, Wo)
        lib.bilinear_resize_f32(segs[n], up, cos[n], H, W, Ho, Wo, 1, 0, None)
        per = cos[n] * Ho * Wo
        assert same_bits(soft[n, qf[n] * per:(qf[n] + 1) * per].numpy(), up.reshape(-1).numpy()), n
        rest = torch.cat([soft[n, :qf[n] * per], soft[n, (qf[n] + 1) * per:]])
        assert torch.isnan(rest).all()


SENTINEL = 0xA5      # every byte of preds, the soft maps and partial before a call


def _sentinel(shape, dtype):
    t = torch.empty(shape, dtype=dtype)
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == SENTINEL).all())


def check_map_positions(lib, batch, single):
    """label maps with a map position of their own (descriptor column 5), for `batch` = seg_postprocess_exact_batch / seg_postprocess_batch
    against `single` = seg_postprocess_exact / seg_postprocess: 3 slots of 9 x 11 -> 37 x 45 (the bilinear clamp on both axes), 5, 2 and 3
    classes inside COcap = 5, Tcap = 4 positions of label rows and Tmaps = 7 of maps.  Slot 0 reads position 3 and writes map 6, slot 1
    is inactive, slot 2 reads position 1 and writes map 0 - bit for bit the single-video call, and no other byte of preds changes.
    Then map positions Tmaps and -1: nothing is written; Tmaps = 0: refused, nothing written.  -> (label rows, descriptor rows)"""
    from vfs_amd._lib import VfsError
    H, W, Ho, Wo, Tcap, Tmaps, COcap = 9, 11, 37, 45, 4, 7, 5
    HW = H * W
    plan = {0: (3, 6, 5), 2: (1, 0, 3)}      # slot: (position of the label rows, map position, classes)
    g = torch.Generator().manual_seed(51)
    sb = torch.full((3, Tcap * HW * COcap), float('nan'))
    sb[1, :HW * 2] = torch.randn(HW * 2, generator=g)      # slot 1 holds rows (2 classes) and sits the step out
    segs = {}
    for n, (q, m, CO) in plan.items():
        segs[n] = torch.randn(HW, CO, generator=g)
        sb[n, q * HW * CO:(q + 1) * HW * CO] = segs[n].reshape(-1)
    rows = {n: (q, [0], 0, CO, m) for n, (q, m, CO) in plan.items()}
    preds, partial = _sentinel((3, Tmaps, Ho * Wo), torch.uint8), _sentinel((3, 64, COcap, 2), torch.float32)
    batch(sb, partial, preds, _desc_rows(3, rows), 3, Tcap, Tmaps, H, W, COcap, Ho, Wo, None)
    for n, (q, m, CO) in plan.items():
        lab = torch.zeros(Ho * Wo, dtype=torch.uint8)
        single(segs[n], torch.zeros(64 * CO * 2), lab, H, W, CO, Ho, Wo, None)
        assert len(set(lab.tolist())) > 1
        assert torch.equal(preds[n, m], lab), n
        assert _untouched(preds[n, [p for p in range(Tmaps) if p != m]]), n
    assert _untouched(preds[1]) and _untouched(partial[1])
    for bad, Tm, refused in (({0: Tmaps, 2: -1}, Tmaps, False), ({}, 0, True)):
        preds, partial = _sentinel((3, Tmaps, Ho * Wo), torch.uint8), _sentinel((3, 64, COcap, 2), torch.float32)
        desc = _desc_rows(3, {n: r[:4] + (bad.get(n, r[4]),) for n, r in rows.items()})
        if refused:
            with pytest.raises(VfsError, match=r'failed \(-1\)'):      # csrc/vfs_common.h: VFS_ERR_SHAPE
                batch(sb, partial, preds, desc, 3, Tcap, Tm, H, W, COcap, Ho, Wo, None)
        else:
            batch(sb, partial, preds, desc, 3, Tcap, Tm, H, W, COcap, Ho, Wo, None)
        assert _untouched(preds) and _untouched(partial), (bad, Tm)
    return sb, segs, rows


def test_batched_postprocessing_map_positions(backend):
    """fp32 label maps (check_map_positions) and the soft maps of the same rows: slot n starts at n * Tmaps * COcap * Ho * Wo and holds
    [map position][CO_n][Ho][Wo] packed, so slot 0's map 6 (5 classes) and slot 2's map 0 (3 classes) lie at their own offsets"""
    from vfs_amd._lib import VfsError
    lib = backend.hostlib
    sb, segs, rows = check_map_positions(lib, lib.seg_postprocess_exact_batch, lib.seg_postprocess_exact)
    H, W, Ho, Wo, Tcap, Tmaps, COcap = 9, 11, 37, 45, 4, 7, 5
    soft = _sentinel((3, Tmaps * COcap * Ho * Wo), torch.float32)
    lib.bilinear_resize_f32_batch(sb, soft, _desc_rows(3, rows), 3, Tcap, Tmaps, H, W, COcap, Ho, Wo, None)
    for n, (q, _, _, CO, m) in rows.items():
        up = torch.zeros(CO, Ho, Wo)
        lib.bilinear_resize_f32(segs[n], up, CO, H, W, Ho, Wo, 1, 0, None)
        per = CO * Ho * Wo
        assert same_bits(soft[n, m * per:(m + 1) * per].numpy(), up.reshape(-1).numpy()), n
        assert _untouched(soft[n, :m * per]) and _untouched(soft[n, (m + 1) * per:]), n
    assert _untouched(soft[1])
    for bad, Tm, refused in (({0: Tmaps, 2: -1}, Tmaps, False), ({}, 0, True)):
        soft = _sentinel((3, Tmaps * COcap * Ho * Wo), torch.float32)
        desc = _desc_rows(3, {n: r[:4] + (bad.get(n, r[4]),) for n, r in rows.items()})
        if refused:
            with pytest.raises(VfsError, match=r'failed \(-1\)'):
                lib.bilinear_resize_f32_batch(sb, soft, desc, 3, Tcap, Tm, H, W, COcap, Ho, Wo, None)
        else:
            lib.bilinear_resize_f32_batch(sb, soft, desc, 3, Tcap, Tm, H, W, COcap, Ho, Wo, None)
        assert _untouched(soft), (bad, Tm)


def test_invalid_rows_and_arguments_are_refused(emu_backend):
    """a row outside the single-video ranges sits the step out (nothing of it is read or written); the host-side checks raise"""
    lib = emu_backend.hostlib
    H, W, C = 8, 8, 64
    b = Batch(lib, 2, 3, H, W, C, 3, False)
    for n in range(2):
        b.put(n, *_features(3, H * W, C, 3, 60 + n))
    nb = torch.zeros(1, dtype=torch.int64)
    lib.labelprop_f32_batch_workspace_bytes(H, W, 2, nb)
    ws = torch.zeros((int(nb.item()) + 3) // 4)
    before = b.sb.clone()
    for bad in ((3, [0, 1], 0, 3), (2, [0, 7], 0, 3), (2, [0, 1], 2, 3), (2, [0, 1], 0, 4)):      # qframe, key frame, non_mask_len, CO
        lib.labelprop_f32_batch(b.fb, b.sb, ws, ws.numel() * 4, _desc_rows(2, {1: bad}), 2, 1, 2, 3, H, W, C, 3, 3, 10, 0.07, None)
        assert np.array_equal(b.sb.numpy().view(np.uint32), before.numpy().view(np.uint32)), bad
    desc = _desc_rows(2, {0: (2, [0, 1], 0, 3)})
    for args in ((b.fb, b.sb, ws, ws.numel() * 4, desc, 65, 1, 2, 3, H, W, C, 3, 3, 10, 0.07, None),        # nslots
                 (b.fb, b.sb, ws, ws.numel() * 4, desc, 2, 1, 65, 3, H, W, C, 3, 3, 10, 0.07, None),        # max_nkeys
                 (b.fb, b.sb, ws, ws.numel() * 4, desc, 2, 1, 2, 3, H, W, C, 3, 3, 11, 0.07, None),         # topk
                 (b.fb, b.sb, ws, ws.numel() * 4 - 256, desc, 2, 1, 2, 3, H, W, C, 3, 3, 10, 0.07, None)):  # workspace
        with pytest.raises(Exception):
            lib.labelprop_f32_batch(*args)


# ---- tracker level: VanillaTracker.forward_test_batch == forward_test, video by video ---------------------------------------------
TEST_CFG = dict(precede_frames=2, topk=10, temperature=0.07, neighbor_range=6, strides=(1, 2, 1, 1), out_indices=(2,))


def _tracker(dev, **over):
    import vfs_amd
    tc = vfs_amd.ConfigDict(dict(TEST_CFG, **over))
    bb = dict(type='ResNet', depth=18, out_indices=tc['out_indices'], strides=tc['strides'], norm_eval=False, zero_init_residual=True)
    model = vfs_amd.build_model(dict(type='VanillaTracker', backbone=bb), train_cfg=None, test_cfg=tc)
    g = torch.Generator().manual_seed(1234)
    with torch.no_grad():      # BatchNorm running statistics away from (0, 1), scales away from 0: the features are not degenerate
        for name, buf in model.named_buffers():
            if name.endswith('running_mean'):
                buf.copy_(0.2 * torch.randn(buf.shape, generator=g))
            elif name.endswith('running_var'):
                buf.copy_(0.5 + torch.rand(buf.shape, generator=g))
        for name, p in model.named_parameters():
            if p.ndim == 1 and name.endswith('weight'):
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
            elif p.ndim == 1:
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / p[0].numel()) ** 0.5)
    return model.to(dev).eval()


def _videos(lengths, sizes, soft, dev, seed=7):
    g = torch.Generator().manual_seed(seed)
    imgs_list, refs, metas = [], [], []
    for i, (T, (H, W)) in enumerate(zip(lengths, sizes)):
        base = torch.randn(1, 1, 3, 1, H, W, generator=g)
        imgs_list.append((base + 0.3 * torch.randn(1, 1, 3, T, H, W, generator=g)).to(dev))      # a video: frames that resemble each other
        if soft:
            refs.append(torch.softmax(2.0 * torch.randn(1, 4, H, W, generator=g), dim=1))
        else:
            lab = torch.zeros(H, W, dtype=torch.uint8)
            for c in range(1, 2 + i % 4):      # 2 .. 5 classes, different from video to video
                y, x = 6 * c, 10 * c
                lab[y:y + 24, x:x + 30] = c
            refs.append(lab[None])
        metas.append([dict(original_shape=(H, W, 3))])
    return imgs_list, refs, metas


def _per_video(model, imgs_list, refs, metas):
    return [model(a, return_loss=False, ref_seg_map=b, img_meta=c)[0] for a, b, c in zip(imgs_list, refs, metas)]


def _assert_same(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, (i, a.shape, b.shape)
        assert np.array_equal(a, b), (i, float((a != b).mean()))


@pytest.mark.gpu
@pytest.mark.parametrize('soft', [False, True])
def test_forward_test_batch_equals_per_video(gpu_backend, soft):
    """six videos, two slots: refills, an idle slot at the tail, two frame sizes, a one-frame clip; class counts differ (3-D maps)"""
    model = _tracker(gpu_backend.dev)
    lengths = [3, 6, 1, 4, 6, 2]
    sizes = [(64, 96), (64, 96), (64, 96), (72, 88), (64, 96), (72, 88)]
    imgs_list, refs, metas = _videos(lengths, sizes, soft, gpu_backend.dev)
    want = _per_video(model, imgs_list, refs, metas)
    assert [w.shape[0] for w in want] == lengths
    assert all(len(np.unique(w[-1] if not soft else w[-1].argmax(0))) > 1 for w in want)      # not degenerate
    for batch in (2, 1, 64):
        _assert_same(model.forward_test_batch(imgs_list, refs, metas, batch=batch), want)


@pytest.mark.gpu
@pytest.mark.parametrize('over', [dict(precision='bf16'), dict(all_blocks=True)])
def test_forward_test_batch_fallback_configurations(gpu_backend, over):
    """no batched kernels for the bf16 precision and for all_blocks: forward_test per video inside, same results"""
    model = _tracker(gpu_backend.dev, **over)
    imgs_list, refs, metas = _videos([3, 2], [(64, 96), (64, 96)], False, gpu_backend.dev)
    _assert_same(model.forward_test_batch(imgs_list, refs, metas, batch=2), _per_video(model, imgs_list, refs, metas))


def test_forward_test_batch_small_clips_on_the_emulator(emu_backend, tmp_path, monkeypatch):
    """the CPU counterpart of the tracker-level test: 32 x 48 frames (4 x 6 features), lengths 2, 1, 2 through ONE slot (a refill and a
    one-frame clip); then the same with test_cfg.save_np, honoured as forward_test does"""
    monkeypatch.chdir(tmp_path)
    model = _tracker(emu_backend.dev)
    imgs_list, refs, metas = _videos([2, 1, 2], [(32, 48)] * 3, False, emu_backend.dev)
    want = _per_video(model, imgs_list, refs, metas)
    _assert_same(model.forward_test_batch(imgs_list, refs, metas, batch=1), want)
    model.save_np = True
    got = model.forward_test_batch(imgs_list, refs, metas, batch=2)
    assert all(isinstance(p, str) and p.endswith('.npy') for p in got)
    _assert_same([np.load(p) for p in got], want)


def test_forward_test_batch_argument_errors(emu_backend):
    model = _tracker(emu_backend.dev)
    imgs_list, refs, metas = _videos([2, 2], [(32, 48)] * 2, False, emu_backend.dev)
    assert model.forward_test_batch([], [], []) == []
    with pytest.raises(ValueError):
        model.forward_test_batch(imgs_list, refs[:1], metas)
    with pytest.raises(ValueError):
        model.forward_test_batch(imgs_list, refs, metas[:1])
    for batch in (0, 65, 2.5):
        with pytest.raises(ValueError):
            model.forward_test_batch(imgs_list, refs, metas, batch=batch)
    with pytest.raises(ValueError):
        model.forward_test_batch([imgs_list[0], imgs_list[1][:, :, :, :0]], refs, metas)
    big = _tracker(emu_backend.dev, topk=11)
    with pytest.raises(NotImplementedError) as single:
        big(imgs_list[0], return_loss=False, ref_seg_map=refs[0], img_meta=metas[0])
    with pytest.raises(NotImplementedError) as batched:
        big.forward_test_batch(imgs_list, refs, metas)
    assert str(single.value) == str(batched.value)
    with pytest.raises(NotImplementedError):
        _tracker(emu_backend.dev, precede_frames=64).forward_test_batch(imgs_list, refs, metas)
