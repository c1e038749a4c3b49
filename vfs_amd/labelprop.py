"""VanillaTracker.forward_test on the HIP kernels (trackers/vanilla_tracker.py:80-206).

Differences from the reference's execution (not its results): the feature bank and the soft
label bank stay on the GPU for the whole clip (the reference keeps them on the CPU and re-uploads
<= 21 frames per step), features are L2-normalised once per frame, the backbone stops after the
evaluated stage (the reference also computes and discards layer4), and the dense [T*HW, HW]
affinity / boolean mask are never materialised.  forward_test and forward_test_batch hold every frame of a clip; a stream
(LabelPropStream) and forward_test_batch(..., ring=True) hold the precede_frames + 2 frames the algorithm reads (ring banks, below).

Feature levels: with test_cfg.all_blocks every residual block of the stages in test_cfg.out_indices; otherwise the output of EVERY
stage listed there (the backbone's own out_indices where the config has none), in stage order, from ONE backbone pass that stops after
the last listed stage - tools/test.py:130-131 sets the backbone's out_indices from the test-time config, ResNet.forward returns a tuple
and forward_test propagates once per entry (vanilla_tracker.py:86-93, 199-205).  Every level has its own (h, w, C), workspace and
kernel; the result is [num_feats, T, H, W] (soft: [num_feats, T, CO, H, W]), a single level [T, ...].  The two-pass exact kernels
(csrc/labelprop2.hip) cover C = 256 / 512 / 1024 and C = 64 / 128 (test_cfg.lp2_narrow=False: the dense kernel there); C = 2048 (ResNet-50 stage 3) stays on the
dense fp32 kernel: the two-pass query tile does not fit in registers.

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
from collections import namedtuple

import numpy as np
import torch

from . import knobs, resnet
from .engine import BF16, shared_engine

F32 = torch.float32


LabelPropConfig = namedtuple('LabelPropConfig', 'precision radius with_first non_mask_len with_norm all_blocks precede topk temp batch_step entries narrow')


def labelprop_config(tracker):
    """tracker.test_cfg as the label propagation reads it (vanilla_tracker.py:133-159), checked against the limits of the kernels"""
    tc = tracker.test_cfg
    precision = resnet.eval_precision(None if tc is None else tc.get('precision', None))
    if precision not in ('fp32', 'bf16'):
        raise ValueError(f"test_cfg.precision must be 'fp32' or 'bf16', got {precision!r}")
    if tracker.training:
        raise RuntimeError('forward_test expects model.eval() (BatchNorm running statistics)')
    nr = tc.get('neighbor_range', None)
    with_first = bool(tc.get('with_first', True))
    precede, topk = int(tc['precede_frames']), int(tc['topk'])
    if topk > 10 or precede + (1 if with_first else 0) > 64:
        raise NotImplementedError(f'label propagation kernels: topk <= 10 (got {topk}), precede_frames + first frame <= 64 '
                                  f'(got {precede + (1 if with_first else 0)})')
    return LabelPropConfig(
        precision=precision, radius=int(nr) // 2 if nr is not None else 0,      # radius 0: no spatial mask
        with_first=with_first, non_mask_len=0 if tc.get('with_first_neighbor', True) else 1,      # vanilla_tracker.py:158-159
        with_norm=bool(tc.get('with_norm', True)), all_blocks=bool(tc.get('all_blocks', False)), precede=precede, topk=topk,
        temp=float(tc['temperature']), batch_step=int(tc.get('batch_step', 10)),
        entries=int(tc['lp2_entries']) if 'lp2_entries' in tc else knobs.integer('VFS_LP2_ENTRIES'),      # list entries per query of the two-pass kernels
        narrow=two_pass_narrow(tracker))


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


def feature_stages(tracker):
    """the backbone stages behind the feature levels, in network order (as ResNet.forward returns them): test_cfg.out_indices, or the
    backbone's own where the config has none"""
    return tuple(sorted({int(s) for s in tracker.test_cfg.get('out_indices', tracker.backbone.out_indices)}))


LP2_NARROW_DEFAULT = True      # the two-pass kernels for C = 64 / 128 where test_cfg.lp2_narrow names nothing: measured faster than the dense kernel at both widths (MEASUREMENTS.md)


def two_pass_narrow(tracker):
    """test_cfg.lp2_narrow: the levels of 64 and 128 channels (ResNet-18 stages 0 and 1) on the two-pass kernels - same bits"""
    tc = tracker.test_cfg
    return bool(tc.get('lp2_narrow', LP2_NARROW_DEFAULT)) if tc is not None else LP2_NARROW_DEFAULT


def two_pass_ok(precision, with_norm, C, narrow=None):
    """the two-pass exact label propagation (csrc/labelprop2.hip: bf16 hi/lo prefilter + exact rescoring, same bits as the dense
    kernel) needs the fp32 path, unit rows and a channel count its register-resident query tile covers: 256, 512, 1024, and with
    `narrow` (None: LP2_NARROW_DEFAULT) 64 and 128.  C = 2048 (ResNet-50 stage 3) stays on the dense kernel: the query tile does not
    fit in registers.  VFS_LP_TWO_PASS=0 keeps the dense kernel everywhere (A/B)"""
    widths = (64, 128, 256, 512, 1024) if (LP2_NARROW_DEFAULT if narrow is None else narrow) else (256, 512, 1024)
    return precision == 'fp32' and with_norm and C in widths and knobs.flag('VFS_LP_TWO_PASS')


def _prepare_backbone(tracker, eng, precision):
    """the bf16 kernels read packed copies of the weights: packed once in front of the passes of a clip, a group or a stream"""
    if precision != 'fp32':
        tracker.backbone.attach(eng)
        eng.pack_weights()


def _backbone_levels(tracker, eng, frames_ncthw, all_blocks, precision):
    """ONE backbone pass over the n frames of imgs [1,3,n,H,W] (after _prepare_backbone) -> [(feature map [n,h,w,C] as the backbone
    leaves it, h, w, C)], one entry per feature level: the outputs of the listed stages (feature_stages), or with all_blocks the
    blocks of those stages.  The maps live in the engine's buffers until the next pass."""
    bb = tracker.backbone
    stages = feature_stages(tracker)
    own = bb.out_indices
    if not all_blocks and tuple(own) != stages:      # the pass returns the listed stages and stops after the last of them
        bb.out_indices = stages
    try:
        return _backbone_pass(tracker, eng, frames_ncthw, all_blocks, precision, stages)
    finally:
        bb.out_indices = own


def _backbone_pass(tracker, eng, frames_ncthw, all_blocks, precision, stages):
    bb = tracker.backbone
    dev = frames_ncthw.device
    _, _, n, H, W = frames_ncthw.shape
    s = eng.stream(dev)
    chunk = frames_ncthw.contiguous().float()
    if precision == 'fp32':
        from .exact import exact_state
        x4 = eng.buf('exact.x4', (n, H, W, 4), F32, dev)
        eng.lib.imgs_to_nhwc4_f32(chunk, x4, 1, 1, n, H, W, s)
        outs, blocks = exact_state(bb).forward(eng, x4, n, H, W, stop_after_out=True)
        block_feats = [b[:4] for b in blocks]
    else:
        Wp = W + (W & 1)
        x4 = eng.buf('backbone.x4', (n, H, Wp, 4), BF16, dev)
        eng.lib.imgs_to_nhwc4(chunk, x4, 1, 1, n, H, W, Wp, s)
        outs, ctx = bb.forward_nhwc(eng, x4, n, H, W, 1, False, stop_after_out=True)
        block_feats = [(b['out'], b['dims'][-1][2], b['dims'][-1][3], b['out'].shape[-1]) for b in ctx['blocks']]
    if all_blocks:          # every block output of the listed stages, in network order
        return [block_feats[i] for i in _block_feats(bb, len(block_feats), stages)]
    return [outs[si] for si in stages]      # the outputs of the listed stages: each its own h x w and channel count


def extract_feature_levels(tracker, eng, frames_ncthw, batch_step, all_blocks=False, precision='bf16', with_norm=True, banks=None, split_banks=None):
    """imgs [1,3,T,H,W] fp32 -> (banks, split_banks, shapes), one entry per feature level: the evaluated stage, or with all_blocks
    (vanilla_tracker.py:32-45, README.md:76) every residual block of every stage in test_cfg.out_indices.
    banks[l]        [T, h*w, C], L2-normalised over the channels unless with_norm=False (bf16 or fp32 by `precision`);
    split_banks[l]  its bf16 hi / lo split copy [T, h*w, 2C] for the two-pass kernels, or None where they do not apply;
    shapes[l]       (h, w, C).  banks / split_banks: the destinations, if given (forward_test_batch: a slot's views of its stacked banks)"""
    dev = frames_ncthw.device
    T = frames_ncthw.shape[2]
    s = eng.stream(dev)
    exact = precision == 'fp32'
    _prepare_backbone(tracker, eng, precision)
    shapes = None
    for t0 in range(0, T, batch_step):
        n = min(batch_step, T - t0)
        feats = _backbone_levels(tracker, eng, frames_ncthw[:, :, t0:t0 + n], all_blocks, precision)
        if shapes is None:
            shapes = [(h, w, C) for (_, h, w, C) in feats]
            if banks is None:
                banks = [torch.empty(T, h * w, C, dtype=F32 if exact else BF16, device=dev) for (h, w, C) in shapes]
                split_banks = [torch.empty(T, h * w, 2 * C, dtype=BF16, device=dev) if two_pass_ok(precision, with_norm, C, two_pass_narrow(tracker)) else None
                               for (h, w, C) in shapes]
            split_banks = split_banks or [None] * len(banks)      # destinations without split copies: the dense kernels
        for bank, hl, (feat, h, w, C) in zip(banks, split_banks, feats):
            if not with_norm:
                bank[t0:t0 + n].copy_(feat.reshape(n, h * w, C))
            elif exact:
                eng.lib.l2norm_rows_f32(feat, bank[t0:t0 + n], n * h * w, C, s)
                if hl is not None:      # x = hi + lo (bf16 each) of the unit rows: the operands of the two-pass kernel's matrix pass
                    eng.lib.split_rows_bf16x2(bank[t0:t0 + n], hl[t0:t0 + n], n * h * w, C, s)
            else:
                eng.lib.l2norm_rows(feat, bank[t0:t0 + n], n * h * w, C, s)
    return banks, split_banks, shapes


def extract_features(tracker, eng, frames_ncthw, batch_step, precision='bf16', with_norm=True):
    """the one feature level of the evaluated stage: -> (bank [T, h*w, C], h, w, C)"""
    (bank,), _, ((h, w, C),) = extract_feature_levels(tracker, eng, frames_ncthw, batch_step, False, precision, with_norm)
    return bank, h, w, C


def _key_frames(f, precede, with_first, non_mask_len=0):
    """the key frames of query frame f: the `precede` frames before it, after frame 0 if with_first"""
    keys = list(range(max(0, f - precede), f))
    keys = [0] + keys if with_first else keys      # frame 0 twice while f <= precede (as the reference)
    assert 0 <= non_mask_len < len(keys)           # local_attention.py:272
    return keys


def _first_maps(ref_seg_map, dev):
    """the reference label map of a video as forward_test reads it (vanilla_tracker.py:94): (4-D) the soft / one-hot map
    [CO, Hr, Wr] on the device, (3-D) the label map, uint8 on the host - either way of at most 256 classes"""
    if ref_seg_map.ndim != 4:
        return ref_seg_map[0].detach().cpu().numpy().astype(np.uint8)
    if ref_seg_map.shape[1] > 256:
        raise NotImplementedError('label propagation kernels: at most 256 classes')
    return ref_seg_map[0].detach().to(dev, F32).contiguous()


def _at_feature_size(ref, h, w):
    """a video's reference map (_first_maps) at feature size -> (h, w, class count, the label map PIL-nearest resized / None for a soft map)"""
    if torch.is_tensor(ref):
        return h, w, ref.shape[0], None
    small = pil_nearest_resize(ref, h, w)
    return h, w, int(small.max()) + 1, small       # F.one_hot infers max+1 classes


def _first_frame(eng, ref, feat, rows0, out_size, pred0):
    """a video's reference map (_first_maps) -> frame 0 of its label rows `rows0` (feat: _at_feature_size; both None: not wanted) and of
    its predictions `pred0` (original size `out_size`).  A soft map is resized bilinearly to both, and the soft maps of the later
    frames are returned as they are, without min-max / argmax; a label map goes one-hot into the rows and torch-nearest into the
    prediction (vanilla_tracker.py:101-111,167; pred0 None: only returned).  -> the map at the original size: pred0 (soft), on the host (labels)"""
    out_h, out_w = out_size
    if torch.is_tensor(ref):
        s = eng.stream(pred0.device)
        CO, hr, wr = ref.shape
        if rows0 is not None:
            eng.lib.bilinear_resize_f32(ref, rows0, CO, hr, wr, feat[0], feat[1], 0, 1, s)
        eng.lib.bilinear_resize_f32(ref, pred0, CO, hr, wr, out_h, out_w, 0, 0, s)
        return pred0
    if rows0 is not None:
        h, w, CO, small = feat
        eng.lib.onehot(torch.from_numpy(np.ascontiguousarray(small)).to(rows0.device), rows0, h * w, CO, eng.stream(rows0.device))
    big = np.ascontiguousarray(torch_nearest_resize(ref, out_h, out_w))
    if pred0 is not None:
        pred0.copy_(torch.from_numpy(big).to(pred0.device).reshape(pred0.shape))
    return big


def _workspace_bytes(lib, h, w, two_pass, entries, nslots=None, precision='fp32'):
    """workspace bytes of the dense or the two-pass kernels (`entries` list entries per query, <= 0: the library's own), one video or
    `nslots` slots (`precision`: which batched kernels; one video: the dense kernels of both precisions share a layout)"""
    nbytes = torch.zeros(1, dtype=torch.int64)
    if nslots is None:
        if not two_pass:
            lib.labelprop_workspace_bytes(h, w, nbytes)
        elif entries > 0:
            lib.labelprop_f32_2pass_workspace_bytes_for(h, w, entries, nbytes)
        else:
            lib.labelprop_f32_2pass_workspace_bytes(h, w, nbytes)
    elif precision == 'bf16':
        lib.labelprop_batch_workspace_bytes(h, w, nslots, nbytes)
    elif two_pass:
        lib.labelprop_f32_2pass_batch_workspace_bytes(h, w, max(0, entries), nslots, nbytes)
    else:
        lib.labelprop_f32_batch_workspace_bytes(h, w, nslots, nbytes)
    return int(nbytes.item())


def _result(tracker, arr):
    """the label maps of one feature level as forward_test hands them over: the array, or with test_cfg.save_np its .npy path"""
    if not tracker.save_np:
        return arr
    os.makedirs('.eval', exist_ok=True)                             # vanilla_tracker.py:184-193
    tmp = tempfile.NamedTemporaryFile(dir='.eval', suffix='.npy', delete=False)
    tmp.close()
    np.save(tmp.name, arr)
    return tmp.name


def _levels_result(tracker, levels):
    """forward_test(...)[0] from the label maps of every feature level (vanilla_tracker.py:199-205: several levels are stacked
    [num_feats, T, ...]; save_np: the list of their paths)"""
    res = [_result(tracker, arr) for arr in levels]
    if len(res) == 1:
        return res[0]
    return res if tracker.save_np else np.stack(res, axis=0)


def forward_test_hip(tracker, imgs, ref_seg_map, img_meta):
    return _forward_test(tracker, labelprop_config(tracker), imgs, ref_seg_map, img_meta)


def _forward_test(tracker, cfg, imgs, ref_seg_map, img_meta):
    eng = shared_engine()
    imgs = imgs.reshape((-1,) + tuple(imgs.shape[2:]))          # [1,3,T,H,W]
    assert imgs.shape[0] == 1
    dev = imgs.device
    clip_len = imgs.size(2)
    banks, hls, shapes = extract_feature_levels(tracker, eng, imgs, cfg.batch_step, cfg.all_blocks, cfg.precision, cfg.with_norm)
    out_h, out_w = img_meta[0]['original_shape'][:2]
    ref = _first_maps(ref_seg_map, dev)
    soft = torch.is_tensor(ref)
    all_preds = []
    for bank, hl, (h, w, C) in zip(banks, hls, shapes):
        _, _, CO, _ = feat = _at_feature_size(ref, h, w)
        sbank = torch.zeros(clip_len, h * w, CO, dtype=F32, device=dev)
        shape = (clip_len, CO, out_h, out_w) if soft else (clip_len, out_h, out_w)
        preds = torch.empty(shape, dtype=F32 if soft else torch.uint8, device=dev)
        first = _first_frame(eng, ref, feat, sbank[0], (out_h, out_w), preds[0])
        ref = first.clone() if soft else first          # the reference keeps the resized map for the next feature level
        step = _SingleStep(eng, cfg, bank, hl, sbank, (h, w, C), CO, (out_h, out_w))
        for f in range(1, clip_len):
            step(f, _key_frames(f, cfg.precede, cfg.with_first, cfg.non_mask_len), preds[f])
        all_preds.append(preds.cpu().numpy())
    return [_levels_result(tracker, all_preds)]


class _SingleStep:
    """one propagation step of ONE video at one feature level on the single-video kernels: the label rows of bank position `q` from the
    key positions `keys` (reference order, duplicates kept), post-processed into `pred`.  Positions index bank / hl / sbank: the frame
    numbers of a whole-clip bank (_forward_test), the ring positions of a stream"""

    def __init__(self, eng, cfg, bank, hl, sbank, shape, CO, out_size):
        self.eng, self.cfg, self.bank, self.hl, self.sbank, self.shape, self.CO, self.out_size = eng, cfg, bank, hl, sbank, shape, CO, out_size
        h, w, _ = shape
        dev = bank.device
        self.pairs = mask_pairs(h, w, cfg.radius)
        self.partial = eng.ws('ws.segpost', 64 * CO * 2, F32, dev)
        self.lpws = eng.ws('ws.labelprop', (_workspace_bytes(eng.lib, h, w, hl is not None, cfg.entries) + 3) // 4, F32, dev)

    def __call__(self, q, keys, pred):
        eng, cfg, bank, hl, sbank, lpws, CO = self.eng, self.cfg, self.bank, self.hl, self.sbank, self.lpws, self.CO
        (h, w, C), (out_h, out_w), pairs = self.shape, self.out_size, self.pairs
        radius, non_mask_len, topk, temp = cfg.radius, cfg.non_mask_len, cfg.topk, cfg.temp
        exact = cfg.precision == 'fp32'
        dev = bank.device
        s = eng.stream(dev)
        ks = (ctypes.c_int * len(keys))(*keys)
        nmask = len(keys) - non_mask_len
        work = (2.0 * C * (nmask * pairs + non_mask_len * float(h * w) ** 2),          # in-mask affinity FLOP
                float(bank.element_size()) * (len(set(keys)) + 1) * h * w * C)          # every key / query row once
        if hl is not None:      # same label maps, bit for bit (csrc/labelprop2.hip); algorithmic work as SURVEY section 8(d) counts it:
            # ONE product per in-mask (query, key, channel) (the kernel EXECUTES three bf16 products for it - hi.hi + hi.lo + lo.hi:
            # bench.py reports that as executed_frac) and every key / query row once in both copies (fp32 + split)
            eng.timed('labelprop_2pass', (work[0], 2.0 * work[1]), dev, eng.lib.labelprop_f32_2pass, bank, hl, sbank, sbank[q], lpws, lpws.numel() * 4, q, ks,
                      len(keys), h, w, C, CO, radius, non_mask_len, topk, temp, 1, s)
        else:
            eng.timed('labelprop_f32' if exact else 'labelprop', work, dev, eng.lib.labelprop_f32 if exact else eng.lib.labelprop, bank, sbank, sbank[q],
                      lpws, lpws.numel() * 4, q, ks, len(keys), h, w, C, CO, radius, non_mask_len, topk, temp, s)
        if torch.is_floating_point(pred):      # soft maps
            eng.lib.bilinear_resize_f32(sbank[q], pred, CO, h, w, out_h, out_w, 1, 0, s)
        else:
            eng.timed('seg_postprocess', (0.0, 4.0 * h * w * CO + float(out_h * out_w)), dev, eng.lib.seg_postprocess_exact if exact else eng.lib.seg_postprocess,
                      sbank[q], self.partial, pred, h, w, CO, out_h, out_w, s)


# ---------------------------------------------------------------------------------------------------------------------
# Ring banks and the streaming interface.
#
# For query frame f the reference reads frame 0 and frames max(0, f - precede_frames) .. f - 1 only (vanilla_tracker.py:132-149).  A bank
# of R = precede_frames + 2 positions therefore serves a clip of any length: position 0 keeps frame 0, frame f >= 1 lives at position
# 1 + (f - 1) % (precede_frames + 1) - the precede_frames key frames and the query frame never share a position.  The label rows use the
# same positions, and the kernels, which address their banks through qframe / kslot / descriptor rows, get positions instead of frame
# numbers: the key lists keep the reference's order and duplicates.  The label maps of a clip are not a ring: a descriptor row names
# the map position its post-processing writes on its own (column 5), and that stays the frame number.  A frame enters its position
# through the table-driven ingest (csrc/bank_ingest.hip): one launch per feature level for the new frames of every video of a step.
def ring_positions(precede):
    """bank positions per video of a ring bank"""
    return precede + 2


def ring_position(f, precede):
    """the bank position of frame f (an int or an integer array)"""
    return np.where(np.asarray(f) == 0, 0, 1 + (np.asarray(f) - 1) % (precede + 1))


def _ring_rows(table, precede):
    """the descriptor rows of batch_schedule with the frame numbers that address the banks - query frame (column 1), key frames
    (8..) - replaced by their ring positions; the map position (column 5) stays the frame number"""
    rows = table.copy()
    rows[..., 1] = ring_position(table[..., 1], precede)
    rows[..., 8:] = ring_position(table[..., 8:], precede)
    return rows


def _ingest(eng, cfg, feats, banks, hls, tables, n):
    """the maps `feats` (_backbone_levels) of n images enter the banks, level by level in one launch: image i of a level at row
    tables[level][i] (device int64 [n][2]: the first row in the bank, in its split copy) - unit rows and their hi / lo split with the bits
    of extract_feature_levels, plain copies with test_cfg.with_norm=False"""
    for (feat, h, w, C), bank, hl, table in zip(feats, banks, hls, tables):
        s = eng.stream(bank.device)
        if cfg.precision == 'fp32':
            eng.lib.bank_ingest_f32(feat, bank, hl, table, n, h * w, C, bank.numel() // C, int(cfg.with_norm), s)
        else:
            eng.lib.bank_ingest_bf16(feat, bank, table, n, h * w, C, bank.numel() // C, int(cfg.with_norm), s)


def _frames_ncthw(frames, what):
    """[1,3,H,W], [1,3,t,H,W] or forward_test's [1,1,3,t,H,W] -> [1,3,t,H,W]"""
    if not torch.is_tensor(frames) or frames.ndim not in (4, 5, 6) or frames.numel() == 0:
        raise ValueError(f'{what}: frames [1,3,H,W] or [1,3,t,H,W], got {tuple(getattr(frames, "shape", ()))}')
    if frames.ndim == 6:
        frames = frames.reshape((-1,) + tuple(frames.shape[2:]))
    elif frames.ndim == 4:
        frames = frames[:, :, None]
    if frames.shape[0] != 1 or frames.shape[1] != 3:
        raise ValueError(f'{what}: frames [1,3,H,W] or [1,3,t,H,W], got {tuple(frames.shape)}')
    return frames


class _StreamLevel:
    """one feature level of a stream: its ring banks, the rows of the ingest table (one per position) and its propagation step"""

    def __init__(self, eng, cfg, shape, CO, out_size, R, dev):
        h, w, C = shape
        exact = cfg.precision == 'fp32'
        self.bank = torch.empty(R, h * w, C, dtype=F32 if exact else BF16, device=dev)
        self.hl = torch.empty(R, h * w, 2 * C, dtype=BF16, device=dev) if two_pass_ok(cfg.precision, cfg.with_norm, C, cfg.narrow) else None
        self.sbank = torch.zeros(R, h * w, CO, dtype=F32, device=dev)
        self.table = (torch.arange(R, dtype=torch.int64) * (h * w))[:, None].repeat(1, 2).to(dev)
        self.step = _SingleStep(eng, cfg, self.bank, self.hl, self.sbank, shape, CO, out_size)


class LabelPropStream:
    """VanillaTracker.forward_test for frames that arrive one at a time (tracker.open_stream): `first` holds what forward_test returns
    for frame 0 and push(frames) what it returns for the pushed frames, bit for bit - [t, ...] per push (with several feature levels [levels, t,
    ...]; `first` with t = 1), so that the rows of `first` and of every push, joined along the frame axis, are forward_test(...)[0] of
    the whole clip.  Always arrays: test_cfg.save_np is forward_test's.  The device buffers are ring banks of `bank_positions` =
    precede_frames + 2 positions per feature level, whatever the number of frames pushed; the packed weights of the bf16 precision are
    those of the moment the stream was opened."""

    def __init__(self, tracker, first, ref_seg_map, img_meta):
        cfg = self.cfg = labelprop_config(tracker)
        self.tracker, self.eng = tracker, shared_engine()
        first = _frames_ncthw(first, 'open_stream')
        if first.size(2) != 1:
            raise ValueError(f'open_stream: one first frame, got {first.size(2)}')
        dev = first.device
        self.frame_size = tuple(first.shape[3:])
        self.bank_positions = R = ring_positions(cfg.precede)
        self.out_size = out_size = tuple(int(v) for v in img_meta[0]['original_shape'][:2])
        ref = _first_maps(ref_seg_map, dev)
        self.soft = torch.is_tensor(ref)
        _prepare_backbone(tracker, self.eng, cfg.precision)
        feats = _backbone_levels(tracker, self.eng, first, cfg.all_blocks, cfg.precision)
        self.levels, firsts = [], []
        for _, h, w, C in feats:
            _, _, CO, _ = feat = _at_feature_size(ref, h, w)
            lv = _StreamLevel(self.eng, cfg, (h, w, C), CO, out_size, R, dev)
            pred0 = self._preds(1, CO, dev)
            ref = _first_frame(self.eng, ref, feat, lv.sbank[0], out_size, pred0[0])
            ref = ref.clone() if self.soft else ref          # the next level starts from this level's map at the output size
            lv.CO = CO
            self.levels.append(lv)
            firsts.append(pred0.cpu().numpy())
        self._ingest(feats, 0, 0)
        self.frames = 1
        self.first = self._rows(firsts)

    def _preds(self, t, CO, dev):
        shape = (t, CO) + self.out_size if self.soft else (t,) + self.out_size
        return torch.empty(shape, dtype=F32 if self.soft else torch.uint8, device=dev)

    def _rows(self, levels):
        return levels[0] if len(levels) == 1 else np.stack(levels, axis=0)

    def _ingest(self, feats, j, pos):
        """image j of the maps `feats` enters position pos of every level's banks"""
        n = feats[0][0].numel() // (feats[0][1] * feats[0][2] * feats[0][3])
        _ingest(self.eng, self.cfg, [(feat.reshape(n, h * w, C)[j], h, w, C) for feat, h, w, C in feats], [lv.bank for lv in self.levels],
                [lv.hl for lv in self.levels], [lv.table[pos:pos + 1] for lv in self.levels], 1)

    @property
    def bank_bytes(self):
        """bytes of the stream's device buffers"""
        return sum(t.numel() * t.element_size() for lv in self.levels for t in (lv.bank, lv.hl, lv.sbank, lv.table) if t is not None)

    def push(self, frames):
        if self.levels is None:
            raise ValueError('push: the stream is closed')
        frames = _frames_ncthw(frames, 'push')
        if tuple(frames.shape[3:]) != self.frame_size:
            raise ValueError(f'push: frames of {tuple(frames.shape[3:])}, the stream was opened with {self.frame_size}')
        cfg, t = self.cfg, frames.size(2)
        preds = [self._preds(t, lv.CO, frames.device) for lv in self.levels]
        for t0 in range(0, t, cfg.batch_step):
            n = min(cfg.batch_step, t - t0)
            feats = _backbone_levels(self.tracker, self.eng, frames[:, :, t0:t0 + n], cfg.all_blocks, cfg.precision)
            for j in range(n):      # a ring holds one query frame: the frames of a chunk enter and propagate one after the other
                f = self.frames
                self._ingest(feats, j, int(ring_position(f, cfg.precede)))
                keys = [int(p) for p in ring_position(_key_frames(f, cfg.precede, cfg.with_first, cfg.non_mask_len), cfg.precede)]
                for lv, pred in zip(self.levels, preds):
                    lv.step(int(ring_position(f, cfg.precede)), keys, pred[t0 + j])
                self.frames += 1
        return self._rows([p.cpu().numpy() for p in preds])

    def close(self):
        self.levels = None


# ---------------------------------------------------------------------------------------------------------------------
# forward_test of a batch of videos in lock-step (csrc: vfs_labelprop_f32_batch / _2pass_batch, vfs_labelprop_batch for the bf16
# precision, and the batched post-processing).
#
# A JHMDB or VIP frame (30 x 40 features: 20 query tiles) does not fill the chip, and an evaluation is hundreds of such videos.  Here
# up to `batch` videos of one frame size occupy SLOTS of stacked banks and advance together: one launch set per step serves every slot,
# each at its own frame with its own key list and class count; a slot whose video ends is refilled with the next one.  All clip
# lengths are known, so the schedule of the whole group - per step and slot: active, query frame, key frames, non_mask_len, class
# count - is worked out on the host first and uploaded ONCE as the descriptor table the kernels read (include/vfs_hip.h); inside the
# step loop nothing is read back and nothing but a newly admitted video's frames and first label map goes to the device.
DESC_INTS = 72      # include/vfs_hip.h VFS_LPB_DESC_INTS: [0] active, [1] query frame (bank position), [2] key frames, [3] non_mask_len,
                    # [4] classes, [5] map position (the query frame's number), [6..7] 0, [8..] the key frames (bank positions)


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
            keys = _key_frames(f, precede, with_first, non_mask_len)
            row[n, :6] = (1, f, len(keys), non_mask_len, class_counts[v], f)
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


def _level_maps(ref, shapes, out_size):
    """a video's reference map at the size of every feature level (_at_feature_size).  Level l + 1 starts from the map level l resized
    to the output size, not from the caller's (as _forward_test chains them): class counts of a label map may differ between levels"""
    feats = []
    for h, w, _ in shapes:
        feats.append(_at_feature_size(ref, h, w))
        if not torch.is_tensor(ref):      # (a soft map keeps its channel count: nothing else of it is read here)
            ref = torch_nearest_resize(ref, *out_size)
    return feats


class _Level:
    """one feature level of a group: its stacked banks (layout: include/vfs_hip.h), maps and descriptor table on the device.  `ring`
    decides the positions per slot of the feature, split and label-row banks (and, in _Group, when frames are extracted) and nothing
    else: the maps hold every frame of the longest clip either way, and the kernels write them in place"""

    def __init__(self, eng, cfg, shape, split, feats, lengths, soft, out_size, B, Tcap, dev, ring=False):
        h, w, C = self.h, self.w, self.C = shape
        out_h, out_w = out_size
        exact = cfg.precision == 'fp32'
        # frame positions per slot of the banks: every frame of the longest clip, or a ring
        Tb = self.Tb = ring_positions(cfg.precede) if ring else Tcap
        self.fb = torch.empty(B, Tb, h * w, C, dtype=F32 if exact else BF16, device=dev)
        self.hl = torch.empty(B, Tb, h * w, 2 * C, dtype=BF16, device=dev) if split else None      # fp32, two-pass kernels only
        self.feats = feats
        self.cos = [feat[2] for feat in feats]
        COcap = self.COcap = max(self.cos)
        self.sb = torch.empty(B, Tb * h * w * COcap, dtype=F32, device=dev)      # label rows, packed per slot with the slot's class count
        if soft:
            self.preds = torch.empty(B, Tcap * COcap * out_h * out_w, dtype=F32, device=dev)
        else:
            self.preds = torch.empty(B, Tcap, out_h * out_w, dtype=torch.uint8, device=dev)
        self.ws_bytes = _workspace_bytes(eng.lib, h, w, split, cfg.entries, B, cfg.precision)
        # the levels share one schedule; only the class-count column of their tables may differ
        self.frames, self.steps = batch_schedule(lengths, self.cos, B, cfg.precede, cfg.with_first, cfg.non_mask_len)
        self.table = torch.from_numpy(_ring_rows(self.frames, cfg.precede) if ring else self.frames).to(dev)      # the ONE upload of the schedule


class _Group:
    """videos of ONE frame size, label-map kind and output size (each of >= 2 frames) in lock-step: per feature level (one, or with
    all_blocks every block of the evaluated stages) the stacked banks of B slots, and the workspace and the schedule they share"""

    def __init__(self, tracker, eng, cfg, videos, ref_seg_maps, out_size, batch, ring=False):
        """videos: [imgs [1,3,T,H,W]] in the order of admission.  ring: the banks of a slot are rings of precede_frames + 2 positions
        (above), and a video's frames are extracted as the lock-step reaches them, one backbone pass per step for every active slot"""
        self.tracker, self.eng, self.cfg, self.videos, self.out_size, self.ring = tracker, eng, cfg, videos, out_size, ring
        dev = videos[0].device
        self.refs = [_first_maps(r, dev) for r in ref_seg_maps]
        self.soft = torch.is_tensor(self.refs[0])
        self.lengths = [int(v.size(2)) for v in videos]
        B, Tcap = self.B, self.Tcap = min(batch, len(videos)), max(self.lengths)
        # the stacked banks can be sized only when a feature map is known
        if ring:      # one pass over frame 0 of video 0 for the shapes alone (admit() extracts it again with the frames it enters with)
            _prepare_backbone(tracker, eng, cfg.precision)
            self.first = None
            shapes = [(h, w, C) for _, h, w, C in _backbone_levels(tracker, eng, videos[0][:, :, :1], cfg.all_blocks, cfg.precision)]
            splits = [True if two_pass_ok(cfg.precision, cfg.with_norm, C, cfg.narrow) else None for _, _, C in shapes]
        else:         # video 0 is extracted into tensors of its own, which admit() copies into its slot - one device-to-device copy per
            # group, the same launches as extracting into the slot
            self.first = extract_feature_levels(tracker, eng, videos[0], cfg.batch_step, cfg.all_blocks, cfg.precision, cfg.with_norm)
            _, splits, shapes = self.first
        feats = [_level_maps(ref, shapes, out_size) for ref in self.refs]      # [video][level]
        self.levels = [_Level(eng, cfg, shape, split is not None, [f[l] for f in feats], self.lengths, self.soft, out_size, B, Tcap, dev, ring)
                       for l, (shape, split) in enumerate(zip(shapes, splits))]
        self.steps = self.levels[0].steps
        if not self.soft:
            self.partial = eng.ws('ws.segpost_batch', B * 64 * max(lv.COcap for lv in self.levels) * 2, F32, dev)
        self.ws = torch.empty((max(lv.ws_bytes for lv in self.levels) + 3) // 4, dtype=F32, device=dev)      # (per group: released with it)
        if ring:
            self._ring_tables(dev)

    def _ring_tables(self, dev):
        """what the schedule says about the frames a ring group extracts, worked out and uploaded once like the descriptor table:
        active[i] = [(slot, video, query frame)] of step i, and per level the rows of the ingest table, int64 [steps][2][B][2]:
        [i][0] the first frames of the videos admitted at step i, [i][1] the query frames of its active slots, in that order"""
        frames, R = self.levels[0].frames, self.levels[0].Tb
        videos, self.active = {}, []
        rows = np.full((len(self.steps), 2, self.B, 2), -1, np.int64)
        for i, (admitted, retired, _, _) in enumerate(self.steps):
            videos.update(admitted)
            self.active.append([(n, videos[n], int(frames[i, n, 1])) for n in sorted(videos)])
            for j, (n, _) in enumerate(admitted):
                rows[i, 0, j] = n * R
            for j, (n, _, f) in enumerate(self.active[i]):
                rows[i, 1, j] = n * R + int(ring_position(f, self.cfg.precede))
            for n, _ in retired:
                del videos[n]
        for lv in self.levels:
            lv.ingest = torch.from_numpy(np.where(rows < 0, rows, rows * (lv.h * lv.w))).to(dev)

    def _extract(self, frames, rows, n):
        """ring: ONE backbone pass over the n frames [(video, frame)], which enter the banks at the table rows `rows` of every level"""
        chunk = torch.stack([self.videos[k][0, :, f] for k, f in frames], dim=1)[None]
        feats = _backbone_levels(self.tracker, self.eng, chunk, self.cfg.all_blocks, self.cfg.precision)
        _ingest(self.eng, self.cfg, feats, [lv.fb for lv in self.levels], [lv.hl for lv in self.levels], [lv.ingest[rows] for lv in self.levels], n)

    def _extract_clip(self, n, k):
        """every frame of video k enters slot n"""
        T, cfg = self.lengths[k], self.cfg
        fbs, hls = [lv.fb[n, :T] for lv in self.levels], [None if lv.hl is None else lv.hl[n, :T] for lv in self.levels]
        if self.first is not None:      # video 0 (always the first admitted)
            for dst, src in zip(fbs + hls, self.first[0] + self.first[1]):
                if dst is not None:
                    dst.copy_(src)
            self.first = None
        else:
            extract_feature_levels(self.tracker, self.eng, self.videos[k], cfg.batch_step, cfg.all_blocks, cfg.precision, cfg.with_norm, fbs, hls)

    def admit(self, i):
        """the videos admitted at step i enter their slots: their features (ring: of their first frames), and frame 0 of their label rows
        and predictions, level by level"""
        admitted = self.steps[i][0]
        if self.ring and admitted:
            self._extract([(k, 0) for _, k in admitted], (i, 0), len(admitted))
        for n, k in admitted:
            if not self.ring:
                self._extract_clip(n, k)
            out_h, out_w = self.out_size
            ref = self.refs[k]
            for lv in self.levels:      # the next level starts from this level's map at the output size (a soft map: frame 0 of its predictions)
                CO = lv.cos[k]
                pred0 = lv.preds[n, :CO * out_h * out_w].reshape(CO, out_h, out_w) if self.soft else lv.preds[n, 0]
                ref = _first_frame(self.eng, ref, lv.feats[k], lv.sb[n, :lv.h * lv.w * CO], self.out_size, pred0)

    def step(self, i):
        """one launch set per level: every active slot propagates to and post-processes its frame of row i of the schedule"""
        lib, cfg, ws = self.eng.lib, self.cfg, self.ws
        _, _, nactive, most = self.steps[i]
        B, Tcap, (out_h, out_w) = self.B, self.Tcap, self.out_size
        s = self.eng.stream(ws.device)
        if self.ring:
            self._extract([(k, f) for _, k, f in self.active[i]], (i, 1), nactive)
        for lv in self.levels:
            row, h, w, C, COcap, Tb = lv.table[i], lv.h, lv.w, lv.C, lv.COcap, lv.Tb
            if cfg.precision == 'bf16':
                lib.labelprop_batch(lv.fb, lv.sb, ws, lv.ws_bytes, row, B, nactive, most, Tb, h, w, C, COcap, cfg.radius, cfg.topk, cfg.temp, s)
            elif lv.hl is not None:
                lib.labelprop_f32_2pass_batch(lv.fb, lv.hl, lv.sb, ws, lv.ws_bytes, row, B, nactive, most, Tb, h, w, C, COcap, cfg.radius,
                                              cfg.topk, cfg.temp, 1, s)
            else:
                lib.labelprop_f32_batch(lv.fb, lv.sb, ws, lv.ws_bytes, row, B, nactive, most, Tb, h, w, C, COcap, cfg.radius, cfg.topk,
                                        cfg.temp, s)
            if self.soft:
                lib.bilinear_resize_f32_batch(lv.sb, lv.preds, row, B, Tb, Tcap, h, w, COcap, out_h, out_w, s)
            elif cfg.precision == 'bf16':
                lib.seg_postprocess_batch(lv.sb, self.partial, lv.preds, row, B, Tb, Tcap, h, w, COcap, out_h, out_w, s)
            else:
                lib.seg_postprocess_exact_batch(lv.sb, self.partial, lv.preds, row, B, Tb, Tcap, h, w, COcap, out_h, out_w, s)

    def retire(self, n, k):
        """-> forward_test(...)[0] of video k, which ended in slot n: its maps leave the device now, the slot is refilled at the next step"""
        T, (out_h, out_w) = self.lengths[k], self.out_size
        levels = []
        for lv in self.levels:
            CO = lv.cos[k]
            if self.soft:
                arr = lv.preds[n, :T * CO * out_h * out_w].reshape(T, CO, out_h, out_w)
            else:
                arr = lv.preds[n, :T].reshape(T, out_h, out_w)
            levels.append(arr.cpu().numpy() if arr.device.type != 'cpu' else arr.numpy().copy())      # (the slot's maps are overwritten by the next video)
        return _levels_result(self.tracker, levels)


def forward_test_batch_hip(tracker, imgs_list, ref_seg_maps, img_metas, batch=8, ring=False):
    """out[i] == forward_test(imgs_list[i], ref_seg_maps[i], img_metas[i])[0] for every video, in input order.
    Videos are grouped by frame size, kind of label map (3-D labels / 4-D soft maps) and output size; a group runs in lock-step
    (above) on the batched kernels of test_cfg.precision ('fp32': vfs_labelprop_f32_2pass_batch / vfs_labelprop_f32_batch, 'bf16':
    vfs_labelprop_batch), with all_blocks=True one launch set per feature level and step.  There is no per-video path inside.
    ring=True: a slot's feature and label-row banks hold precede_frames + 2 positions instead of every frame of the longest clip, and
    the frames are extracted step by step, one backbone pass for the next frame of every active slot (above: ring banks); the maps
    are the whole-clip batch's, written in place."""
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
    cfg = labelprop_config(tracker)
    eng = shared_engine()
    bb = tracker.backbone
    nlevels = len(_block_feats(bb, 1 << 30, feature_stages(tracker))) if cfg.all_blocks else len(feature_stages(tracker))
    outs = [None] * n
    groups = {}
    for i, (imgs, ref_seg_map, meta) in enumerate(zip(imgs_list, ref_seg_maps, img_metas)):
        imgs = imgs.reshape((-1,) + tuple(imgs.shape[2:]))          # [1,3,T,H,W]
        assert imgs.shape[0] == 1
        soft, dev = ref_seg_map.ndim == 4, imgs.device
        out_h, out_w = (int(v) for v in meta[0]['original_shape'][:2])
        if imgs.size(2) > 1:
            groups.setdefault((imgs.shape[3], imgs.shape[4], soft, out_h, out_w, dev), []).append((i, imgs, ref_seg_map))
            continue
        ref = _first_maps(ref_seg_map, dev)      # a one-frame clip is its (resized) reference map, level after level
        levels = []
        for _ in range(nlevels):
            pred0 = torch.empty(ref.shape[0], out_h, out_w, dtype=F32, device=dev) if soft else None
            ref = _first_frame(eng, ref, None, None, (out_h, out_w), pred0)
            levels.append((ref.cpu().numpy() if soft else ref)[None])
        outs[i] = _levels_result(tracker, levels)
    for (_, _, _, out_h, out_w, _), vids in groups.items():
        group = _Group(tracker, eng, cfg, [v[1] for v in vids], [v[2] for v in vids], (out_h, out_w), batch, ring)
        for step, (_, retired, _, _) in enumerate(group.steps):
            group.admit(step)
            group.step(step)
            for slot, k in retired:
                outs[vids[k][0]] = group.retire(slot, k)
    return outs
