"""VanillaTracker.forward_test on the HIP kernels (trackers/vanilla_tracker.py:80-206).

Differences from the reference's execution (not its results): the feature bank and the soft
label bank stay on the GPU for the whole clip (the reference keeps them on the CPU and re-uploads
<= 21 frames per step), features are L2-normalised once per frame, the backbone stops after the
evaluated stage (the reference also computes and discards layer4), and the dense [T*HW, HW]
affinity / boolean mask are never materialised.

Two precisions (test_cfg.precision, default 'fp32'; env VFS_EVAL_PRECISION overrides the default):
  'fp32'  fp32 storage and bit-defined fp32 arithmetic (csrc/exact_f32.hip, vfs_amd/exact.py) - what the
          reference computes in; label maps equal the C oracle's bit for bit;
  'bf16'  the training path's bf16 kernels and a bf16 bank (about 3x faster; labels differ where the exact
          10th / 11th affinities or the two best classes are nearly tied).
Limits of the kernels (checked, errors raised): topk <= 10, at most 64 key frames per step
(precede_frames + 1 <= 64), feature channels % 64 == 0 (bf16) / % 4 == 0 (fp32), <= 256 classes."""
import ctypes
import os
import tempfile

import numpy as np
import torch

from . import knobs, resnet
from .engine import BF16, shared_engine

F32 = torch.float32


def eval_precision(test_cfg):
    p = resnet.eval_precision(None if test_cfg is None else test_cfg.get('precision', None))
    if p not in ('fp32', 'bf16'):
        raise ValueError(f"test_cfg.precision must be 'fp32' or 'bf16', got {p!r}")
    return p


def pil_nearest_resize(label, out_h, out_w):
    """PIL NEAREST as used by mmcv.imresize(backend='pillow') in pil_nearest_interpolate
    (common/utils.py:25-42): src = floor((dst + 0.5) * in / out)."""
    in_h, in_w = label.shape
    ys = np.minimum(np.floor((np.arange(out_h) + 0.5) * (in_h / out_h)).astype(np.int64), in_h - 1)
    xs = np.minimum(np.floor((np.arange(out_w) + 0.5) * (in_w / out_w)).astype(np.int64), in_w - 1)
    return label[ys][:, xs]


def torch_nearest_resize(label, out_h, out_w):
    """F.interpolate(mode='nearest') index rule: src = floor(dst * in / out)."""
    in_h, in_w = label.shape
    ys = np.minimum(np.floor(np.arange(out_h) * np.float32(in_h / out_h)).astype(np.int64), in_h - 1)
    xs = np.minimum(np.floor(np.arange(out_w) * np.float32(in_w / out_w)).astype(np.int64), in_w - 1)
    return label[ys][:, xs]


def mask_pairs(h, w, radius):
    """number of (query, key) pairs of one key frame inside the circular mask (affinity_utils.py:144-156: distance < radius);
    radius <= 0: no mask -> (h*w)^2.  The ALGORITHMIC affinity work of a propagation step is 2 * C * pairs per key frame."""
    if radius <= 0:
        return float(h * w) ** 2
    n = 0
    for dy in range(-(radius - 1), radius):
        for dx in range(-(radius - 1), radius):
            if dy * dy + dx * dx < radius * radius:
                n += max(0, h - abs(dy)) * max(0, w - abs(dx))
    return float(n)


def _block_feats(bb, ctx_blocks, stages):
    """(block index range) of every residual block of the listed stages, in network order"""
    sel, bi = [], 0
    for si, lname in enumerate(bb.res_layers):
        nb = len(getattr(bb, lname))
        if si in stages:
            sel += list(range(bi, min(bi + nb, ctx_blocks)))
        bi += nb
        if bi >= ctx_blocks:
            break
    return sel


def two_pass_ok(precision, with_norm, C):
    """the two-pass exact label propagation (csrc/labelprop2.hip: bf16 hi/lo prefilter + exact rescoring, same bits as the dense
    kernel) needs the fp32 path, unit rows and a channel count its register-resident query tile covers; VFS_LP_TWO_PASS=0 keeps
    the dense kernel (A/B)"""
    return precision == 'fp32' and with_norm and C in (256, 512, 1024) and knobs.flag('VFS_LP_TWO_PASS')


def extract_features(tracker, eng, frames_ncthw, batch_step, all_blocks=False, precision='bf16', with_norm=True, split_banks=None, alloc=None):
    """imgs [1,3,T,H,W] fp32 -> feature bank [T, h*w, C] of the evaluated stage, L2-normalised over the
    channels unless with_norm=False (bf16 or fp32 by `precision`); with all_blocks (vanilla_tracker.py:32-45,
    README.md:76) a LIST of banks, one per residual block of every stage in test_cfg.out_indices.
    split_banks: a list that receives, per bank, its bf16 hi / lo split copy [T, h*w, 2C] (or None) for the two-pass kernels.
    alloc(T, rows, channels, dtype): where a bank lives (forward_test_batch: the slot's region of the stacked banks); default: its own tensor."""
    bb = tracker.backbone
    dev = frames_ncthw.device
    _, _, T, H, W = frames_ncthw.shape
    s = eng.stream(dev)
    stages = tuple(tracker.test_cfg.get('out_indices', bb.out_indices))
    stage = stages[0]
    exact = precision == 'fp32'
    if exact:
        from .exact import exact_state
        ex = exact_state(bb)
    else:
        bb.attach(eng)
        eng.pack_weights()
    Wp = W + (W & 1)
    banks, shapes = None, None
    for t0 in range(0, T, batch_step):
        n = min(batch_step, T - t0)
        chunk = frames_ncthw[:, :, t0:t0 + n].contiguous().float()
        if exact:
            x4 = eng.buf('exact.x4', (n, H, W, 4), F32, dev)
            eng.lib.imgs_to_nhwc4_f32(chunk, x4, 1, 1, n, H, W, s)
            outs, blocks = ex.forward(eng, x4, n, H, W, stop_after_out=True)
            block_feats = [b[:4] for b in blocks]
        else:
            x4 = eng.buf('backbone.x4', (n, H, Wp, 4), BF16, dev)
            eng.lib.imgs_to_nhwc4(chunk, x4, 1, 1, n, H, W, Wp, s)
            outs, ctx = bb.forward_nhwc(eng, x4, n, H, W, 1, False, stop_after_out=True)
            block_feats = [(b['out'], b['dims'][-1][2], b['dims'][-1][3], b['out'].shape[-1]) for b in ctx['blocks']]
        if all_blocks:          # every block output of the listed stages, in network order
            feats = [block_feats[i] for i in _block_feats(bb, len(block_feats), stages)]
        else:
            feats = [outs[stage]]
        if banks is None:
            if alloc is None:
                def alloc(T, rows, channels, dtype):
                    return torch.empty(T, rows, channels, dtype=dtype, device=dev)
            banks = [alloc(T, h * w, C, F32 if exact else BF16) for (_, h, w, C) in feats]
            shapes = [(h, w, C) for (_, h, w, C) in feats]
            hls = [alloc(T, h * w, 2 * C, BF16) if two_pass_ok(precision, with_norm, C) else None
                   for (_, h, w, C) in feats]
            if split_banks is not None:
                split_banks.extend(hls)
        for bank, hl, (feat, h, w, C) in zip(banks, hls, feats):
            if not with_norm:
                bank[t0:t0 + n].copy_(feat.reshape(n, h * w, C))
            elif exact:
                eng.lib.l2norm_rows_f32(feat, bank[t0:t0 + n], n * h * w, C, s)
                if hl is not None:      # x = hi + lo (bf16 each) of the unit rows: the operands of the two-pass kernel's matrix pass
                    eng.lib.split_rows_bf16x2(bank[t0:t0 + n], hl[t0:t0 + n], n * h * w, C, s)
            else:
                eng.lib.l2norm_rows(feat, bank[t0:t0 + n], n * h * w, C, s)
    if all_blocks:
        return banks, shapes
    return banks[0], shapes[0][0], shapes[0][1], shapes[0][2]


def _result(tracker, arr):
    """the label maps of one feature level as forward_test hands them over: the array, or with test_cfg.save_np its .npy path"""
    if not tracker.save_np:
        return arr
    os.makedirs('.eval', exist_ok=True)                             # vanilla_tracker.py:184-193
    tmp = tempfile.NamedTemporaryFile(dir='.eval', suffix='.npy', delete=False)
    tmp.close()
    np.save(tmp.name, arr)
    return tmp.name


def forward_test_hip(tracker, imgs, ref_seg_map, img_meta):
    tc = tracker.test_cfg
    eng = shared_engine()
    precision = eval_precision(tc)
    exact = precision == 'fp32'
    imgs = imgs.reshape((-1,) + tuple(imgs.shape[2:]))          # [1,3,T,H,W]
    assert imgs.shape[0] == 1
    dev = imgs.device
    clip_len = imgs.size(2)
    if tracker.training:
        raise RuntimeError('forward_test expects model.eval() (BatchNorm running statistics)')
    nr = tc.get('neighbor_range', None)
    radius = int(nr) // 2 if nr is not None else 0
    with_first = bool(tc.get('with_first', True))
    non_mask_len = 0 if tc.get('with_first_neighbor', True) else 1      # vanilla_tracker.py:158-159
    with_norm = bool(tc.get('with_norm', True))
    all_blocks = bool(tc.get('all_blocks', False))
    precede = int(tc['precede_frames'])
    topk, temp = int(tc['topk']), float(tc['temperature'])
    if topk > 10 or precede + (1 if with_first else 0) > 64:
        raise NotImplementedError(f'label propagation kernels: topk <= 10 (got {topk}), precede_frames + first frame <= 64 '
                                  f'(got {precede + (1 if with_first else 0)})')
    hls = []
    if all_blocks:
        banks, shapes = extract_features(tracker, eng, imgs, int(tc.get('batch_step', 10)), True, precision, with_norm, hls)
    else:
        bank, h, w, C = extract_features(tracker, eng, imgs, int(tc.get('batch_step', 10)), False, precision, with_norm, hls)
        banks, shapes = [bank], [(h, w, C)]
    s = eng.stream(dev)
    out_h, out_w = img_meta[0]['original_shape'][:2]
    input_onehot = ref_seg_map.ndim == 4                         # vanilla_tracker.py:94
    if input_onehot:
        ref = ref_seg_map[0].detach().to(dev, F32).contiguous()  # [CO, Hr, Wr] soft / one-hot map
    else:
        ref = ref_seg_map[0].detach().cpu().numpy().astype(np.uint8)
    lp = eng.lib.labelprop_f32 if exact else eng.lib.labelprop
    post = eng.lib.seg_postprocess_exact if exact else eng.lib.seg_postprocess
    all_preds = []
    for bank, hl, (h, w, C) in zip(banks, hls, shapes):
        if input_onehot:
            # bilinear to the feature size (values) and to the original size (frame 0 of the output); the soft maps of
            # the later frames are returned as they are, without min-max / argmax (vanilla_tracker.py:101-111,167)
            CO, hr, wr = ref.shape
            sbank = torch.zeros(clip_len, h * w, CO, dtype=F32, device=dev)
            eng.lib.bilinear_resize_f32(ref, sbank[0], CO, hr, wr, h, w, 0, 1, s)
            preds = torch.empty(clip_len, CO, out_h, out_w, dtype=F32, device=dev)
            eng.lib.bilinear_resize_f32(ref, preds[0], CO, hr, wr, out_h, out_w, 0, 0, s)
            ref = preds[0].clone()            # the reference keeps the resized map for the next feature level
        else:
            small = pil_nearest_resize(ref, h, w)
            CO = int(small.max()) + 1                                    # F.one_hot infers max+1 classes
            sbank = torch.zeros(clip_len, h * w, CO, dtype=F32, device=dev)
            eng.lib.onehot(torch.from_numpy(np.ascontiguousarray(small)).to(dev), sbank[0], h * w, CO, s)
            preds = torch.empty(clip_len, out_h, out_w, dtype=torch.uint8, device=dev)
            ref = np.ascontiguousarray(torch_nearest_resize(ref, out_h, out_w))    # vanilla_tracker.py:101-104 (kept, as there)
            preds[0] = torch.from_numpy(ref).to(dev)
        if CO > 256:
            raise NotImplementedError('label propagation kernels: at most 256 classes')
        pairs = mask_pairs(h, w, radius)
        partial = eng.ws('ws.segpost', 64 * CO * 2, F32, dev)
        nbytes = torch.zeros(1, dtype=torch.int64)
        entries = int(tc['lp2_entries']) if 'lp2_entries' in tc else knobs.integer('VFS_LP2_ENTRIES')      # list entries per query of the two-pass kernels
        if hl is None:
            eng.lib.labelprop_workspace_bytes(h, w, nbytes)
        elif entries > 0:
            eng.lib.labelprop_f32_2pass_workspace_bytes_for(h, w, entries, nbytes)
        else:
            eng.lib.labelprop_f32_2pass_workspace_bytes(h, w, nbytes)
        lpws = eng.ws('ws.labelprop', (int(nbytes.item()) + 3) // 4, F32, dev)
        for f in range(1, clip_len):
            key_start = max(0, f - precede)
            slots = list(range(key_start, f))
            if with_first:
                slots = [0] + slots                                 # frame 0 twice while f <= precede (as the reference)
            assert 0 <= non_mask_len < len(slots)                   # local_attention.py:272
            ks = (ctypes.c_int * len(slots))(*slots)
            nmask = len(slots) - non_mask_len
            work = (2.0 * C * (nmask * pairs + non_mask_len * float(h * w) ** 2),          # in-mask affinity FLOP
                    float(bank.element_size()) * (len(set(slots)) + 1) * h * w * C)         # every key / query row once
            if hl is not None:      # same label maps, bit for bit (csrc/labelprop2.hip); algorithmic work as SURVEY section 8(d) counts it:
                # ONE product per in-mask (query, key, channel) (the kernel EXECUTES three bf16 products for it - hi.hi + hi.lo + lo.hi:
                # bench.py reports that as executed_frac) and every key / query row once in both copies (fp32 + split)
                eng.timed('labelprop_2pass', (work[0], 2.0 * work[1]), dev, eng.lib.labelprop_f32_2pass, bank, hl, sbank, sbank[f], lpws, lpws.numel() * 4, f, ks,
                          len(slots), h, w, C, CO, radius, non_mask_len, topk, temp, 1, s)
            else:
                eng.timed('labelprop_f32' if exact else 'labelprop', work, dev, lp, bank, sbank, sbank[f], lpws, lpws.numel() * 4, f, ks, len(slots), h, w,
                          C, CO, radius, non_mask_len, topk, temp, s)
            if input_onehot:
                eng.lib.bilinear_resize_f32(sbank[f], preds[f], CO, h, w, out_h, out_w, 1, 0, s)
            else:
                eng.timed('seg_postprocess', (0.0, 4.0 * h * w * CO + float(out_h * out_w)), dev, post, sbank[f], partial, preds[f],
                          h, w, CO, out_h, out_w, s)
        all_preds.append(_result(tracker, preds.cpu().numpy()))
    if tracker.save_np:
        return [all_preds] if len(all_preds) > 1 else [all_preds[0]]
    if len(all_preds) > 1:      # vanilla_tracker.py:199-205: [1, num_feats, T, ...] unravelled over the batch dim
        return [np.stack(all_preds, axis=0)]
    return [all_preds[0]]


# ---------------------------------------------------------------------------------------------------------------------
# forward_test of a batch of videos in lock-step (csrc: vfs_labelprop_f32_batch / _2pass_batch and the batched post-processing).
#
# A JHMDB or VIP frame (30 x 40 features: 20 query tiles) does not fill the chip, and an evaluation is hundreds of such videos.  Here
# up to `batch` videos of one frame size occupy SLOTS of stacked banks and advance together: one launch set per step serves every slot,
# each at its own frame with its own key list and class count; a slot whose video ends is refilled with the next one.  All clip
# lengths are known, so the schedule of the whole group - per step and slot: active, query frame, key frames, non_mask_len, class
# count - is worked out on the host first and uploaded ONCE as the descriptor table the kernels read (include/vfs_hip.h); inside the
# step loop nothing is read back and nothing but a newly admitted video's frames and first label map goes to the device.
DESC_INTS = 72      # include/vfs_hip.h VFS_LPB_DESC_INTS


def _key_frames(f, precede, with_first):
    keys = list(range(max(0, f - precede), f))
    return [0] + keys if with_first else keys      # frame 0 twice while f <= precede (as the reference)


def batch_schedule(lengths, class_counts, nslots, precede, with_first, non_mask_len):
    """the lock-step schedule of videos of `lengths` frames (each >= 2, admitted in this order) over `nslots` slots.
    -> (table int32 [steps][nslots][DESC_INTS], steps) with steps[i] = (admitted [(slot, video)], retired [(slot, video)], active
    slots, most key frames of a slot)"""
    queue = list(range(len(lengths)))[::-1]
    slots = [None] * nslots      # [video, next frame]
    rows, steps = [], []
    while True:
        admitted = []
        for n in range(nslots):
            if slots[n] is None and queue:
                slots[n] = [queue.pop(), 1]
                admitted.append((n, slots[n][0]))
        if all(sl is None for sl in slots):
            break
        row = np.zeros((nslots, DESC_INTS), np.int32)
        retired, most = [], 0
        for n, sl in enumerate(slots):
            if sl is None:
                continue
            v, f = sl
            keys = _key_frames(f, precede, with_first)
            assert 0 <= non_mask_len < len(keys)                    # local_attention.py:272
            row[n, :5] = (1, f, len(keys), non_mask_len, class_counts[v])
            row[n, 8:8 + len(keys)] = keys
            most = max(most, len(keys))
            sl[1] += 1
            if sl[1] == lengths[v]:
                retired.append((n, v))
                slots[n] = None
        rows.append(row)
        steps.append((admitted, retired, sum(int(r[0]) for r in row), most))
    table = np.stack(rows) if rows else np.zeros((0, nslots, DESC_INTS), np.int32)
    return table, steps


def _first_maps(ref_seg_map, dev):
    """the reference label map of a video as forward_test reads it: (4-D) the soft map on the device, (3-D) uint8 on the host"""
    if ref_seg_map.ndim == 4:
        return ref_seg_map[0].detach().to(dev, F32).contiguous()
    return ref_seg_map[0].detach().cpu().numpy().astype(np.uint8)


def _run_group(tracker, eng, cfg, vids, batch, outs):
    """vids: [(index, imgs [1,3,T,H,W], ref_seg_map, out_h, out_w)] of ONE frame size, label-map kind and output size"""
    lib = eng.lib
    dev = vids[0][1].device
    s = eng.stream(dev)
    soft = vids[0][2].ndim == 4
    out_h, out_w = vids[0][3], vids[0][4]
    refs = [_first_maps(v[2], dev) for v in vids]
    if soft and max(r.shape[0] for r in refs) > 256:
        raise NotImplementedError('label propagation kernels: at most 256 classes')
    single = [i for i, v in enumerate(vids) if v[1].size(2) == 1]
    for i in single:      # a one-frame clip is its (resized) reference map
        if soft:
            first = torch.empty(1, refs[i].shape[0], out_h, out_w, dtype=F32, device=dev)
            lib.bilinear_resize_f32(refs[i], first[0], refs[i].shape[0], refs[i].shape[1], refs[i].shape[2], out_h, out_w, 0, 0, s)
            outs[vids[i][0]] = _result(tracker, first.cpu().numpy())
        else:
            outs[vids[i][0]] = _result(tracker, np.ascontiguousarray(torch_nearest_resize(refs[i], out_h, out_w))[None])
    run = [i for i in range(len(vids)) if i not in set(single)]
    if not run:
        return
    B = min(batch, len(run))
    lengths = [int(vids[i][1].size(2)) for i in run]
    Tcap = max(lengths)
    g = {}      # the group's banks: allocated when the first video's feature map is known
    cur = [0]   # the slot being admitted

    def alloc(T, rows, channels, dtype):
        key = 'hl' if dtype == BF16 else 'fb'
        if key not in g:
            g[key] = torch.empty(B, Tcap, rows, channels, dtype=dtype, device=dev)
        return g[key][cur[0], :T]

    def features(n, i):
        cur[0] = n
        return extract_features(tracker, eng, vids[i][1], cfg['batch_step'], False, 'fp32', cfg['with_norm'], [], alloc)[1:]

    def set_up(h, w, C):
        """everything that needs the feature-map size: class counts, label / prediction banks, workspace, the schedule"""
        hw = h * w
        g['small'] = [None if soft else pil_nearest_resize(refs[i], h, w) for i in run]
        cos = [refs[i].shape[0] if soft else int(sm.max()) + 1 for i, sm in zip(run, g['small'])]      # F.one_hot infers max+1 classes
        COcap = max(cos)
        g.update(h=h, w=w, C=C, cos=cos, COcap=COcap)
        g['sb'] = torch.empty(B, Tcap * hw * COcap, dtype=F32, device=dev)
        if soft:
            g['preds'] = torch.empty(B, Tcap * COcap * out_h * out_w, dtype=F32, device=dev)
        else:
            g['preds'] = torch.empty(B, Tcap, out_h * out_w, dtype=torch.uint8, device=dev)
            g['partial'] = eng.ws('ws.segpost_batch', B * 64 * COcap * 2, F32, dev)
        nbytes = torch.zeros(1, dtype=torch.int64)
        if 'hl' in g:
            lib.labelprop_f32_2pass_batch_workspace_bytes(h, w, max(0, cfg['entries']), B, nbytes)
        else:
            lib.labelprop_f32_batch_workspace_bytes(h, w, B, nbytes)
        g['ws'] = torch.empty((int(nbytes.item()) + 3) // 4, dtype=F32, device=dev)      # (per group: released with it)
        table, steps = batch_schedule(lengths, cos, B, cfg['precede'], cfg['with_first'], cfg['non_mask_len'])
        g['table'] = torch.from_numpy(table).to(dev)      # the ONE upload of the schedule
        return steps

    def first_frame(n, k):
        """the video's reference map -> frame 0 of the slot's label rows (feature size) and of its predictions (original size)"""
        i, h, w, CO = run[k], g['h'], g['w'], g['cos'][k]
        hw = h * w
        rows0 = g['sb'][n, :hw * CO]
        if soft:
            ref = refs[i]
            lib.bilinear_resize_f32(ref, rows0, CO, ref.shape[1], ref.shape[2], h, w, 0, 1, s)
            lib.bilinear_resize_f32(ref, g['preds'][n, :CO * out_h * out_w], CO, ref.shape[1], ref.shape[2], out_h, out_w, 0, 0, s)
        else:
            lib.onehot(torch.from_numpy(np.ascontiguousarray(g['small'][k])).to(dev), rows0, hw, CO, s)
            g['preds'][n, 0] = torch.from_numpy(np.ascontiguousarray(torch_nearest_resize(refs[i], out_h, out_w))).to(dev).reshape(-1)

    # the first video's features give the feature-map size; from there on the schedule is fixed
    h, w, C = features(0, run[0])
    steps = set_up(h, w, C)
    hl, ws, table = g.get('hl'), g['ws'], g['table']
    for step, (admitted, retired, nactive, most) in enumerate(steps):
        for n, k in admitted:
            if (step, n) != (0, 0):
                features(n, run[k])
            first_frame(n, k)
        if hl is not None:
            lib.labelprop_f32_2pass_batch(g['fb'], hl, g['sb'], ws, ws.numel() * 4, table[step], B, nactive, most, Tcap, h, w, C, g['COcap'],
                                          cfg['radius'], cfg['topk'], cfg['temp'], 1, s)
        else:
            lib.labelprop_f32_batch(g['fb'], g['sb'], ws, ws.numel() * 4, table[step], B, nactive, most, Tcap, h, w, C, g['COcap'], cfg['radius'],
                                    cfg['topk'], cfg['temp'], s)
        if soft:
            lib.bilinear_resize_f32_batch(g['sb'], g['preds'], table[step], B, Tcap, h, w, g['COcap'], out_h, out_w, s)
        else:
            lib.seg_postprocess_exact_batch(g['sb'], g['partial'], g['preds'], table[step], B, Tcap, h, w, g['COcap'], out_h, out_w, s)
        for n, k in retired:      # the video's maps leave the device now; its slot is refilled at the next step
            T, CO = lengths[k], g['cos'][k]
            if soft:
                arr = g['preds'][n, :T * CO * out_h * out_w].reshape(T, CO, out_h, out_w)
            else:
                arr = g['preds'][n, :T].reshape(T, out_h, out_w)
            arr = arr.cpu().numpy() if dev.type != 'cpu' else arr.numpy().copy()      # (the slot's maps are overwritten by the next video)
            outs[vids[run[k]][0]] = _result(tracker, arr)


def forward_test_batch_hip(tracker, imgs_list, ref_seg_maps, img_metas, batch=8):
    """out[i] == forward_test(imgs_list[i], ref_seg_maps[i], img_metas[i])[0] for every video, in input order.
    Videos are grouped by frame size, kind of label map (3-D labels / 4-D soft maps) and output size; a group runs in lock-step
    (above) with precision 'fp32' and one feature level.  precision='bf16' and all_blocks=True have no batched kernels: they are
    served by forward_test, video by video - same results."""
    n = len(imgs_list)
    if len(ref_seg_maps) != n or len(img_metas) != n:
        raise ValueError(f'forward_test_batch: {n} videos, {len(ref_seg_maps)} label maps, {len(img_metas)} img_metas')
    if isinstance(batch, bool) or not isinstance(batch, int) or not 1 <= batch <= 64:
        raise ValueError(f'forward_test_batch: 1 <= batch <= 64, got {batch!r}')
    if n == 0:
        return []
    for i, imgs in enumerate(imgs_list):
        if imgs is None or not hasattr(imgs, 'numel') or imgs.numel() == 0:
            raise ValueError(f'forward_test_batch: video {i} has no frames')
    tc = tracker.test_cfg
    precision = eval_precision(tc)
    if tracker.training:
        raise RuntimeError('forward_test expects model.eval() (BatchNorm running statistics)')
    nr = tc.get('neighbor_range', None)
    with_first = bool(tc.get('with_first', True))
    precede, topk = int(tc['precede_frames']), int(tc['topk'])
    if topk > 10 or precede + (1 if with_first else 0) > 64:
        raise NotImplementedError(f'label propagation kernels: topk <= 10 (got {topk}), precede_frames + first frame <= 64 '
                                  f'(got {precede + (1 if with_first else 0)})')
    if precision != 'fp32' or bool(tc.get('all_blocks', False)):
        return [forward_test_hip(tracker, a, b, c)[0] for a, b, c in zip(imgs_list, ref_seg_maps, img_metas)]
    cfg = dict(radius=int(nr) // 2 if nr is not None else 0, with_first=with_first, precede=precede, topk=topk, temp=float(tc['temperature']),
               non_mask_len=0 if tc.get('with_first_neighbor', True) else 1, with_norm=bool(tc.get('with_norm', True)),
               batch_step=int(tc.get('batch_step', 10)),
               entries=int(tc['lp2_entries']) if 'lp2_entries' in tc else knobs.integer('VFS_LP2_ENTRIES'))
    groups = {}
    for i, (imgs, ref, meta) in enumerate(zip(imgs_list, ref_seg_maps, img_metas)):
        imgs = imgs.reshape((-1,) + tuple(imgs.shape[2:]))          # [1,3,T,H,W]
        assert imgs.shape[0] == 1
        out_h, out_w = meta[0]['original_shape'][:2]
        key = (imgs.shape[3], imgs.shape[4], ref.ndim == 4, int(out_h), int(out_w), imgs.device)
        groups.setdefault(key, []).append((i, imgs, ref, int(out_h), int(out_w)))
    eng = shared_engine()
    outs = [None] * n
    for vids in groups.values():
        _run_group(tracker, eng, cfg, vids, batch, outs)
    return outs
