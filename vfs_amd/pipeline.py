"""GPU-side training input pipeline: the reference's
RandomResizedCrop -> Resize -> Flip -> Normalize -> FormatShape('NCTHW') chain (configs/r*_*.py:48-91,
mmaction/datasets/pipelines/augmentations.py, formating.py:222-309) applied to decoded uint8 frames that
are already on the device, by ONE kernel (`vfs_crop_resize_flip_norm`, csrc/pipeline.hip).  Decoding
(DecordInit / SampleFrames / DecordDecode) stays outside.

The object-level configs (r18_sgd_cos_100e_r2_1xNx8_k400.py, r50_sgd_cos_100e_r5_1xNx2_k400.py) add ColorJitter,
RandomGrayScale and RandomGaussianBlur between Flip and Normalize (augmentations.py:1224-1320); with any of
them present the chain runs as two launches (`vfs_crop_resize_flip_photo_norm`) that apply them to the uint8
resized frame, where the reference's PIL / cv2 calls act.  A blur whose box radius reaches 1 (sigma above ~0.9) needs a
wider tile in the second launch: `GpuTrainPipeline(..., max_blur_radius=R)` and `vfs_crop_resize_flip_photo_norm_blur`.

DecordDecode returns every video at its own size (Kinetics-400: 340x256, 454x256, 256x340, ...) and the reference crops
and resizes sample by sample; a batch of such samples is packed into one byte buffer (`pack_frames`) and goes through
the same one or two launches (`vfs_crop_resize_flip_norm_ragged`, `vfs_crop_resize_flip_photo_norm_ragged`), which
read a per-sample descriptor table {offset, Hs, Ws}.

The random decisions are drawn on the host with the reference's own rules and RNG streams
(`np.random` for the candidates / flips, `random.randint` for the offsets): seeding both reproduces the
reference's boxes and flips (tests/golden/pipeline_decisions.npz)."""
import collections
import math
import random

import numpy as np
import torch

from ._lib import get_lib
from .engine import BF16


def get_crop_bbox(img_shape, area_range, aspect_ratio_range=(3 / 4, 4 / 3), max_attempts=10):
    """RandomResizedCrop.get_crop_bbox (augmentations.py:213-262)"""
    assert 0 < area_range[0] <= area_range[1] <= 1
    assert 0 < aspect_ratio_range[0] <= aspect_ratio_range[1]
    img_h, img_w = img_shape
    log_lo, log_hi = np.log(aspect_ratio_range[0]), np.log(aspect_ratio_range[1])
    aspect = np.exp(np.random.uniform(log_lo, log_hi, size=max_attempts))
    target = np.random.uniform(*area_range, size=max_attempts) * (img_h * img_w)
    cand_w = np.round(np.sqrt(target * aspect)).astype(np.int32)
    cand_h = np.round(np.sqrt(target / aspect)).astype(np.int32)
    for w, h in zip(cand_w, cand_h):
        if h <= img_h and w <= img_w:
            x0 = random.randint(0, img_w - w)
            y0 = random.randint(0, img_h - h)
            return x0, y0, x0 + w, y0 + h
    side = min(img_h, img_w)
    x0, y0 = (img_w - side) // 2, (img_h - side) // 2
    return x0, y0, x0 + side, y0 + side


def _new_for_frame(i, clip_len, same_on_clip, same_across_clip):
    return (not same_on_clip) or ((not same_across_clip) and i % clip_len == 0 and i > 0)


def clips_from_pipeline(pipeline_cfg):
    """(num_clips, clip_len) of the frames that reach the augmentations: SampleFrames' values, regrouped by
    Clip2Frame when present (r18 config: 8 clips of 1 frame -> 2 clips of 4 frames, pipelines/loading.py:226-232)"""
    num_clips = clip_len = None
    for step in pipeline_cfg:
        if step['type'] == 'SampleFrames':
            num_clips, clip_len = int(step.get('num_clips', 1)), int(step['clip_len'])
        elif step['type'] == 'Clip2Frame' and num_clips is not None:
            total = num_clips * clip_len
            clip_len = int(step['clip_len'])
            assert total % clip_len == 0
            num_clips = total // clip_len
    if num_clips is None:
        raise ValueError('the pipeline has no SampleFrames step: pass num_clips / clip_len')
    return num_clips, clip_len


PHOTOMETRIC = ('ColorJitter', 'RandomGrayScale', 'RandomGaussianBlur')


def _jitter_range(value, center=1, bound=(0, float('inf')), clip_first_on_zero=True):
    """torchvision 0.7 ColorJitter._check_input; None = component disabled"""
    if isinstance(value, (int, float)):
        if value < 0:
            raise ValueError('ColorJitter: a single value must be non-negative')
        value = [center - value, center + value]
        if clip_first_on_zero:
            value[0] = max(value[0], 0.0)
        if not bound[0] <= value[0] <= value[1] <= bound[1]:
            raise ValueError(f'ColorJitter: {value} out of {bound}')
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        if not bound[0] <= value[0] <= value[1] <= bound[1]:
            raise ValueError(f'ColorJitter: {value} out of {bound}')
        value = list(value)
    else:
        raise TypeError('ColorJitter: a number or a (min, max) pair')
    return None if value[0] == value[1] == center else value


def _jitter_params(ranges):
    """torchvision 0.7 ColorJitter.get_params: random.uniform per enabled component, then random.shuffle of the ops"""
    factors, ops = [math.nan] * 4, []
    for k, r in enumerate(ranges):
        if r is not None:
            factors[k] = random.uniform(r[0], r[1])
            ops.append(k + 1)
    random.shuffle(ops)
    return factors, ops


MAX_BLUR_RADIUS = 3      # the largest max_blur_radius the _blur entry points take (csrc/pipeline.hip PHOTO_MAX_RADIUS)


def _box_radius(sigma):
    """PIL GaussianBlur(radius=sigma): _gaussian_blur_radius (3 passes, fp32 as Pillow computes it)"""
    f32 = np.float32
    s2 = f32(f32(f32(sigma) * f32(sigma)) / f32(3))
    L = f32(math.sqrt(12.0 * float(s2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * s2)))
    a = f32(a / f32(f32(6) * f32(s2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    return f32(l + a)


def blur_weights_wide(sigma):
    """PIL GaussianBlur(radius=sigma) at any box radius -> (r, ww, fw) of ImagingLineBoxBlur8: r the integer part of the
    fp32 box radius, ww the weight of the 2r + 1 inner taps, fw of the two outer ones (row words [4] bits 8..15, [6], [7])"""
    f32 = np.float32
    rad = _box_radius(sigma)
    if not rad >= 0:
        raise ValueError(f'RandomGaussianBlur: sigma {sigma} gives a box radius of {float(rad)}')
    r = int(rad)
    ww = int(f32(f32(1 << 24) / f32(rad * f32(2) + f32(1))))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def blur_weights(sigma):
    """the box weights (ww, fw) of a box radius below 1 (sigma_range (0.1, 0.2) gives ~0.1), all that runs without
    max_blur_radius; blur_weights_wide takes any radius"""
    rad = _box_radius(sigma)
    if not 0 <= rad < 1:
        hint = f'; GpuTrainPipeline(..., max_blur_radius={int(rad)}) admits it' if 1 <= rad < MAX_BLUR_RADIUS + 1 else ''
        raise NotImplementedError(f'RandomGaussianBlur: sigma {sigma} gives a box radius of {float(rad)} '
                                  f'(only < 1 runs on the GPU by default{hint})')
    return blur_weights_wide(sigma)[1:]


def pack_photometric(photo, max_blur_radius=0):
    """per-frame photometric decisions (GpuTrainPipeline.sample) -> int32 [F][8] parameter rows of
    vfs_crop_resize_flip_photo_norm (layout in include/vfs_hip.h).  max_blur_radius: the largest integer box radius a row
    may carry (0: blurs of box radius >= 1 are refused, as blur_weights does)"""
    F = len(photo['jitter'])
    rows = np.zeros((F, 8), np.int32)
    for i in range(F):
        if photo['jitter'][i]:
            rows[i, 0] = sum(int(op) << (4 * k) for k, op in enumerate(photo['order'][i]))
            for k in range(3):
                if not math.isnan(photo['factors'][i][k]):
                    rows[i, 1 + k] = np.float32(photo['factors'][i][k]).view(np.int32)
            if not math.isnan(photo['factors'][i][3]):
                rows[i, 4] = int(math.trunc(photo['factors'][i][3] * 255)) % 256    # np.uint8(h * 255) of numpy 1.x: wraps
        rows[i, 5] = int(photo['gray'][i])
        if photo['blur'][i]:
            sigma = float(photo['sigma'][i])
            if max_blur_radius == 0:
                rows[i, 6], rows[i, 7] = blur_weights(sigma)
            else:
                r, rows[i, 6], rows[i, 7] = blur_weights_wide(sigma)
                if r > max_blur_radius:
                    raise NotImplementedError(f'frame {i}: sigma {sigma} gives a box radius of {r}, above max_blur_radius={max_blur_radius}')
                rows[i, 4] |= r << 8
    return rows


class PackedFrames(collections.namedtuple('PackedFrames', 'buffer offsets shapes')):
    """A batch whose samples were decoded at different sizes, as the ragged kernels read it: `buffer` 1-D uint8 on the
    device, sample i's frames uint8 [F][Hs_i][Ws_i][3] at byte `offsets[i]` of it (python ints, no alignment needed),
    `shapes[i]` = (Hs_i, Ws_i).  Made by pack_frames, or by a loader that decodes straight into one buffer."""
    __slots__ = ()


def _sample_info(i, s):
    """(device, shape) of sample i of a mixed-size batch; ValueError for anything but uint8 [F][Hs][Ws][3]"""
    if not isinstance(s, (np.ndarray, torch.Tensor)):
        raise ValueError(f'sample {i}: a numpy array or a tensor is expected, got {type(s).__name__}')
    if s.dtype != (torch.uint8 if isinstance(s, torch.Tensor) else np.uint8):
        raise ValueError(f'sample {i}: dtype {s.dtype}, decoded frames are uint8')
    shape = tuple(int(v) for v in s.shape)
    if len(shape) != 4 or shape[3] != 3 or min(shape) <= 0:
        raise ValueError(f'sample {i}: shape {shape}, expected [F][Hs][Ws][3]')
    return (s.device if isinstance(s, torch.Tensor) else torch.device('cpu')), shape


def pack_frames(samples, device=None, pinned=None):
    """B decoded samples, each uint8 [F][Hs_i][Ws_i][3] at its own size (numpy arrays, host tensors or device tensors, all on
    one device) -> PackedFrames on `device` (None: where the samples are).  Host samples are written back to back into one
    staging tensor - `pinned` when the caller passes a 1-D uint8 tensor that is large enough, so that a loader can reuse
    its pinned buffer (and must not refill it before the copy has run), else a fresh one, pinned when there is a GPU -
    and uploaded with ONE non-blocking copy; device samples are concatenated with one torch.cat."""
    if len(samples) == 0:
        raise ValueError('pack_frames: no samples')
    infos = [_sample_info(i, s) for i, s in enumerate(samples)]
    src = infos[0][0]
    for i, (d, _) in enumerate(infos):
        if d != src:
            raise ValueError(f'sample {i}: on {d}, sample 0 is on {src} (one device per batch)')
    device = src if device is None else torch.device(device)
    sizes = [int(np.prod(shape)) for _, shape in infos]
    offsets = [int(v) for v in np.cumsum([0] + sizes[:-1])]
    shapes = [shape[1:3] for _, shape in infos]
    total = sum(sizes)
    if src.type != 'cpu':
        buffer = torch.cat([s.reshape(-1) for s in samples]).to(device)
        return PackedFrames(buffer, offsets, shapes)
    if (pinned is None or pinned.dtype != torch.uint8 or pinned.dim() != 1 or pinned.device.type != 'cpu'
            or not pinned.is_contiguous() or pinned.numel() < total):
        pinned = torch.empty(total, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    stage = pinned.numpy()
    for s, off, n in zip(samples, offsets, sizes):
        stage[off:off + n] = (s.numpy() if isinstance(s, torch.Tensor) else s).reshape(-1)
    return PackedFrames(pinned[:total].to(device, non_blocking=True), offsets, shapes)


class GpuTrainPipeline:
    """Built from the reference's `train_pipeline` list; `__call__(frames)` with frames uint8
    [B][num_clips*clip_len][Hs][Ws][3] on the GPU returns dict(imgs=fp32 [B][num_clips][3][clip_len][H][W])
    (and x4, the bf16 NHWC4 frames, when asked).  A batch of samples decoded at different sizes (DecordDecode on
    Kinetics: 340x256, 454x256, 256x340, ...) goes in as a list of per-sample [num_clips*clip_len][Hs_i][Ws_i][3]
    arrays / tensors or as a PackedFrames, through the same number of launches (`vfs_crop_resize_flip_norm_ragged`).

    max_blur_radius (0..3): the largest integer box radius a RandomGaussianBlur of this pipeline may reach.  With the
    default 0 only sigma ranges whose box radius stays below 1 are taken (the reference's default (0.1, 0.2)); with R >= 1
    a sigma_range whose ends give int(radius) <= R is admitted ((0.1, 2.0) of the SimSiam / BYOL recipes needs 1) and every
    call runs `vfs_crop_resize_flip_photo_norm_blur` with that R: the bound belongs to the pipeline, so its launches do
    not depend on the sigmas a batch drew."""

    def __init__(self, pipeline_cfg, num_clips=None, clip_len=None, max_blur_radius=0):
        if not (isinstance(max_blur_radius, int) and 0 <= max_blur_radius <= MAX_BLUR_RADIUS):
            raise ValueError(f'max_blur_radius {max_blur_radius!r}: an integer in 0..{MAX_BLUR_RADIUS}')
        self.max_blur_radius = max_blur_radius
        if num_clips is None or clip_len is None:
            num_clips, clip_len = clips_from_pipeline(pipeline_cfg)
        self.num_clips, self.clip_len = int(num_clips), int(clip_len)
        self.crop = self.flip = None
        self.out_hw, self.mean, self.std = None, None, None
        self.jitter = self.gray = self.blur = None
        self._ws = None
        types = [step['type'] for step in pipeline_cfg]
        photo_at = [i for i, t in enumerate(types) if t in PHOTOMETRIC]
        if photo_at:     # only on the uint8 resized frame: after Resize, before Normalize, each once, in this order
            resize = types.index('Resize') if 'Resize' in types else len(types)
            norm = types.index('Normalize') if 'Normalize' in types else -1
            names = [types[i] for i in photo_at]
            if (not all(resize < i < norm for i in photo_at) or len(set(names)) != len(names)
                    or names != sorted(names, key=PHOTOMETRIC.index)):
                raise NotImplementedError(f'{", ".join(names)}: the GPU pipeline runs ColorJitter, RandomGrayScale, '
                                          'RandomGaussianBlur only between Resize and Normalize, each once, in that order')
        for step in pipeline_cfg:
            t = step['type']
            if t == 'RandomResizedCrop':
                self.crop = dict(area_range=tuple(step.get('area_range', (0.08, 1.0))),
                                 aspect_ratio_range=tuple(step.get('aspect_ratio_range', (3 / 4, 4 / 3))),
                                 same_on_clip=step.get('same_on_clip', True), same_across_clip=step.get('same_across_clip', True))
            elif t == 'Resize':
                if step.get('keep_ratio', True):
                    raise NotImplementedError('Resize(keep_ratio=True) is not on the GPU pipeline')
                w, h = step['scale']
                self.out_hw = (int(h), int(w))
            elif t == 'Flip':
                if step.get('direction', 'horizontal') != 'horizontal':
                    raise NotImplementedError('vertical Flip')
                self.flip = dict(flip_ratio=float(step.get('flip_ratio', 0.5)), same_on_clip=step.get('same_on_clip', True),
                                 same_across_clip=step.get('same_across_clip', True))
            elif t == 'Normalize':
                if step.get('to_bgr', False):
                    raise NotImplementedError('Normalize(to_bgr=True)')
                self.mean, self.std = [float(v) for v in step['mean']], [float(v) for v in step['std']]
            elif t == 'FormatShape':
                if step.get('input_format') != 'NCTHW':
                    raise NotImplementedError(f"FormatShape {step.get('input_format')}")
            elif t == 'ColorJitter':      # augmentations.py:1290-1320 (p default 0.5) over torchvision 0.7 ColorJitter
                ranges = [_jitter_range(step.get('brightness', 0)), _jitter_range(step.get('contrast', 0)),
                          _jitter_range(step.get('saturation', 0)),
                          _jitter_range(step.get('hue', 0), center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)]
                self.jitter = dict(ranges=ranges, p=float(step.get('p', 0.5)), same_on_clip=step.get('same_on_clip', True),
                                   same_across_clip=step.get('same_across_clip', True))
            elif t == 'RandomGrayScale':    # augmentations.py:1258-1281
                self.gray = dict(p=float(step.get('p', 0.5)), same_on_clip=step.get('same_on_clip', True),
                                 same_across_clip=step.get('same_across_clip', True))
            elif t == 'RandomGaussianBlur':   # augmentations.py:1224-1255
                sr = tuple(float(v) for v in step.get('sigma_range', (0.1, 0.2)))
                for sg in sr:      # the box radius grows with sigma: the ends bound every draw
                    if max_blur_radius == 0:
                        blur_weights(sg)      # NotImplementedError for a box radius >= 1
                    elif blur_weights_wide(sg)[0] > max_blur_radius:
                        raise NotImplementedError(f'RandomGaussianBlur: sigma {sg} gives a box radius of {blur_weights_wide(sg)[0]}, '
                                                  f'above max_blur_radius={max_blur_radius} (at most {MAX_BLUR_RADIUS} runs on the GPU)')
                self.blur = dict(sigma_range=sr, p=float(step.get('p', 0.5)), same_on_clip=step.get('same_on_clip', True),
                                 same_across_clip=step.get('same_across_clip', True))
        if self.out_hw is None or self.mean is None:
            raise ValueError('pipeline needs Resize(scale=..., keep_ratio=False) and Normalize')

    @property
    def photometric(self):
        return self.jitter is not None or self.gray is not None or self.blur is not None

    def sample(self, num_frames, img_shape):
        """boxes int32 [F][4], flips uint8 [F] for ONE sample, consuming the RNGs like the reference; with photometric
        steps in the pipeline a third item, their per-frame decisions (sample_photometric)"""
        Hs, Ws = img_shape
        if self.crop is None:
            boxes = np.tile(np.asarray([[0, 0, Ws, Hs]], np.int32), (num_frames, 1))
        else:
            c = self.crop
            box = get_crop_bbox(img_shape, c['area_range'], c['aspect_ratio_range'])
            rows = []
            for i in range(num_frames):
                if _new_for_frame(i, self.clip_len, c['same_on_clip'], c['same_across_clip']):
                    box = get_crop_bbox(img_shape, c['area_range'], c['aspect_ratio_range'])
                rows.append(box)
            boxes = np.asarray(rows, np.int32)
        if self.flip is None:
            flips = np.zeros(num_frames, np.uint8)
        else:
            f = self.flip
            flip = np.random.rand() < f['flip_ratio']
            vals = []
            for i in range(num_frames):
                if _new_for_frame(i, self.clip_len, f['same_on_clip'], f['same_across_clip']):
                    flip = np.random.rand() < f['flip_ratio']
                vals.append(flip)
            flips = np.asarray(vals, np.uint8)
        if not self.photometric:
            return boxes, flips
        return boxes, flips, self.sample_photometric(num_frames)

    def sample_photometric(self, num_frames):
        """ColorJitter, RandomGrayScale, RandomGaussianBlur decisions of ONE sample's frames, drawn as their __call__s
        do (augmentations.py:1224-1320): apply flag (np.random) and parameters (random) once before the frame loop, again
        for every frame that does not share.  -> dict jitter uint8 [F], factors float64 [F][4] (brightness, contrast,
        saturation, hue; nan = disabled), order int8 [F][4] (op codes in application order, 0 = none), gray uint8 [F],
        blur uint8 [F], sigma float64 [F]"""
        F = num_frames
        out = dict(jitter=np.zeros(F, np.uint8), factors=np.full((F, 4), np.nan), order=np.zeros((F, 4), np.int8),
                   gray=np.zeros(F, np.uint8), blur=np.zeros(F, np.uint8), sigma=np.zeros(F))
        if self.jitter is not None:
            j = self.jitter
            apply = np.random.rand() < j['p']
            factors, ops = _jitter_params(j['ranges'])
            for i in range(F):
                if _new_for_frame(i, self.clip_len, j['same_on_clip'], j['same_across_clip']):
                    apply = np.random.rand() < j['p']
                    factors, ops = _jitter_params(j['ranges'])
                out['jitter'][i], out['factors'][i] = apply, factors
                out['order'][i, :len(ops)] = ops
        if self.gray is not None:
            g = self.gray
            apply = np.random.rand() < g['p']
            for i in range(F):
                if _new_for_frame(i, self.clip_len, g['same_on_clip'], g['same_across_clip']):
                    apply = np.random.rand() < g['p']
                out['gray'][i] = apply
        if self.blur is not None:
            b = self.blur
            apply = np.random.rand() < b['p']
            sigma = random.uniform(*b['sigma_range'])
            for i in range(F):
                if _new_for_frame(i, self.clip_len, b['same_on_clip'], b['same_across_clip']):
                    apply = np.random.rand() < b['p']
                    sigma = random.uniform(*b['sigma_range'])
                out['blur'][i], out['sigma'][i] = apply, sigma
        return out

    def _workspace(self, frames, H, W, dev):
        """the photometric launches' workspace (luma sums + uint8 frames), kept and grown across calls"""
        nbytes = torch.zeros(1, dtype=torch.int64)
        get_lib().crop_resize_flip_photo_norm_workspace_bytes(frames, H, W, nbytes)
        if self._ws is None or self._ws.device != dev or self._ws.numel() < int(nbytes.item()):
            self._ws = torch.empty(int(nbytes.item()), dtype=torch.uint8, device=dev)
        return self._ws

    def _ragged_input(self, frames, device):
        """a list of per-sample frames or a PackedFrames -> (PackedFrames, int32 [B][4] descriptor table of the ragged
        entry points: offset low, offset high, Hs, Ws per sample), checked here: the kernels zero a sample whose row is
        bad, the host names it"""
        F = self.num_clips * self.clip_len
        if not isinstance(frames, PackedFrames):
            for i, s in enumerate(frames):
                if _sample_info(i, s)[1][0] != F:
                    raise ValueError(f'sample {i}: {s.shape[0]} frames, the pipeline takes num_clips * clip_len = {F}')
            frames = pack_frames(frames, device)
        buf = frames.buffer
        if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous():
            raise ValueError('PackedFrames.buffer: a contiguous 1-D uint8 tensor is expected')
        if len(frames.offsets) != len(frames.shapes) or len(frames.shapes) == 0:
            raise ValueError(f'PackedFrames: {len(frames.offsets)} offsets, {len(frames.shapes)} shapes')
        desc = np.empty((len(frames.shapes), 4), np.uint32)
        for i, (off, (Hs, Ws)) in enumerate(zip(frames.offsets, frames.shapes)):
            off, Hs, Ws = int(off), int(Hs), int(Ws)
            if Hs <= 0 or Ws <= 0 or max(Hs, Ws) >= 1 << 31:
                raise ValueError(f'sample {i}: frame size {Hs} x {Ws}')
            if off < 0 or off + F * Hs * Ws * 3 > buf.numel():
                raise ValueError(f'sample {i}: {F} frames of {Hs} x {Ws} at offset {off} do not fit the buffer of {buf.numel()} bytes')
            desc[i] = off & 0xFFFFFFFF, off >> 32, Hs, Ws
        return frames, desc.view(np.int32)

    def __call__(self, frames, boxes=None, flips=None, want_x4=False, want_imgs=True, photo=None, device=None):
        """boxes / flips / photo: decisions to use instead of sampling them (tests); photo = sample_photometric's dict
        (concatenated over the samples) or packed int32 [B*F][8] rows; with explicit boxes and no photo, no frame gets a
        photometric step.  frames: the dense uint8 tensor, or a mixed-size batch: a list / tuple of per-sample frames, packed
        with pack_frames onto `device` (None: where they are), or a PackedFrames, read in place.  Decisions are drawn sample
        by sample at the sample's own size: the reference's RNG consumption for the batch"""
        F = self.num_clips * self.clip_len
        desc = None
        if isinstance(frames, (list, tuple)):      # PackedFrames is a tuple
            frames, desc = self._ragged_input(frames, device)
            B, dev, shapes = len(frames.shapes), frames.buffer.device, [(int(h), int(w)) for h, w in frames.shapes]
        else:
            assert frames.dtype == torch.uint8 and frames.dim() == 5 and frames.shape[-1] == 3, frames.shape
            B, nf, Hs, Ws, _ = frames.shape
            assert nf == F
            dev, shapes = frames.device, [(Hs, Ws)] * B
        if boxes is None:      # sample by sample: crop boxes of all its frames, then its flips, then the photometric steps (pipeline order)
            draws = [self.sample(F, shape) for shape in shapes]
            boxes, flips = np.concatenate([d[0] for d in draws]), np.concatenate([d[1] for d in draws])
            if self.photometric:
                photo = {k: np.concatenate([d[2][k] for d in draws]) for k in draws[0][2]}
        H, W = self.out_hw
        Wp = W + (W & 1)
        imgs = torch.empty(B, self.num_clips, 3, self.clip_len, H, W, device=dev) if want_imgs else None
        x4 = torch.empty(self.num_clips * B * self.clip_len, H, Wp, 4, dtype=BF16, device=dev) if want_x4 else None
        boxes_i32 = np.ascontiguousarray(boxes, dtype=np.int32)
        flips_u8 = np.ascontiguousarray(flips, dtype=np.uint8)
        if boxes_i32.shape != (B * F, 4) or flips_u8.shape != (B * F,):
            raise ValueError(f'boxes {boxes_i32.shape} / flips {flips_u8.shape}: one row per frame, {B * F} frames')
        if desc is None:
            bt = torch.as_tensor(boxes_i32).to(dev)
            src, size, entry = (frames.contiguous(),), shapes[0], ''
        else:      # the descriptor table travels with the boxes: one upload
            tab = torch.as_tensor(np.concatenate([desc.reshape(-1), boxes_i32.reshape(-1)])).to(dev)
            bt = tab[desc.size:]
            src, size, entry = (frames.buffer, frames.buffer.numel(), tab[:desc.size]), (), '_ragged'
        ft = torch.as_tensor(flips_u8).to(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == 'cuda' else None
        out = dict(boxes=boxes, flips=flips, shapes=shapes)
        tail = (imgs, x4, B, self.num_clips, self.clip_len, *size, H, W, Wp, *self.mean, *self.std, stream)
        if self.photometric:
            if photo is None:
                rows = np.zeros((B * F, 8), np.int32)
            elif isinstance(photo, dict):
                rows = pack_photometric(photo, self.max_blur_radius)
                out['photo'] = photo
            else:
                rows = np.ascontiguousarray(photo, dtype=np.int32)
            assert rows.shape == (B * F, 8), rows.shape
            R = self.max_blur_radius
            if R:      # the kernel clamps a radius above the bound; the host names the frame
                over = np.flatnonzero(((rows[:, 4] >> 8) & 255) > R)
                if over.size:
                    raise ValueError(f'frame {int(over[0])}: photo row carries a box radius of {int((rows[over[0], 4] >> 8) & 255)}, '
                                     f'above max_blur_radius={R}')
            out['photo_rows'] = rows
            pt = torch.as_tensor(rows).to(dev)
            ws = self._workspace(B * F, H, W, dev)
            if R:
                getattr(get_lib(), 'crop_resize_flip_photo_norm_blur' + entry)(*src, bt, ft, pt, ws, ws.numel(), *tail[:-1], R, stream)
            else:
                getattr(get_lib(), 'crop_resize_flip_photo_norm' + entry)(*src, bt, ft, pt, ws, ws.numel(), *tail)
        else:
            getattr(get_lib(), 'crop_resize_flip_norm' + entry)(*src, bt, ft, *tail)
        if want_imgs:
            out['imgs'] = imgs
        if want_x4:
            out['x4'] = x4
        return out
