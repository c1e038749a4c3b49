"""CPU restatement (numpy) of the reference's photometric train-time augmentations.  TEST INFRASTRUCTURE ONLY.

ColorJitter / RandomGrayScale / RandomGaussianBlur (mmaction/datasets/pipelines/augmentations.py:1224-1320)
act on the uint8 frames after Resize and Flip, one frame at a time, through torchvision 0.7's ColorJitter
(PIL ImageEnhance / HSV conversion), mmcv.rgb2gray (cv2.cvtColor) and PIL's GaussianBlur.

* Decisions (`sample_photometric`): `np.random` for the apply flags, `random` for the jitter factors, the
  jitter order (`random.shuffle`) and the blur sigma - PINNED against the reference's own `__call__`
  (tests/golden/photometric.npz, gen_photometric_golden.py).
* PIL arithmetic (blend, HSV round trip, L conversion, contrast mean, extended box blur): restated from
  Pillow's C code and PINNED against the installed Pillow (tests/test_photometric_oracle.py).
* Grey = cv2.cvtColor(RGB2GRAY) fixed point: cv2 is absent, **parity unpinned** (restated from OpenCV's
  published coefficients, like the resize in oracle/pipeline_oracle.py).
"""
import math
import random

import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 1, 2, 3, 4      # jitter op codes (vfs_hip.h vfs_crop_resize_flip_photo_norm)
PHOTO_WORDS = 8


def check_jitter_input(value, center=1, bound=(0, float('inf')), clip_first_on_zero=True):
    """torchvision 0.7 ColorJitter._check_input: a number v -> [center - v, center + v] (first clipped at 0 for
    brightness / contrast / saturation); a range equal to [center, center] disables the component (None)"""
    if isinstance(value, (int, float)):
        if value < 0:
            raise ValueError('jitter value must be non-negative')
        value = [center - value, center + value]
        if clip_first_on_zero:
            value[0] = max(value[0], 0.0)
        if not bound[0] <= value[0] <= value[1] <= bound[1]:      # hue: adjust_hue refuses |factor| > 0.5
            raise ValueError(f'jitter range {value} out of {bound}')
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        if not bound[0] <= value[0] <= value[1] <= bound[1]:
            raise ValueError(f'jitter range {value} out of {bound}')
        value = list(value)
    else:
        raise TypeError('jitter value must be a number or a pair')
    if value[0] == value[1] == center:
        return None
    return value


def jitter_ranges(brightness=0, contrast=0, saturation=0, hue=0):
    return [check_jitter_input(brightness), check_jitter_input(contrast), check_jitter_input(saturation),
            check_jitter_input(hue, center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)]


def jitter_get_params(ranges):
    """torchvision 0.7 ColorJitter.get_params: one `random.uniform` per enabled component (brightness, contrast,
    saturation, hue), then `random.shuffle` of the enabled ops -> (factors[4] (nan = disabled), order list of codes)"""
    factors, ops = [math.nan] * 4, []
    for k, r in enumerate(ranges):
        if r is not None:
            factors[k] = random.uniform(r[0], r[1])
            ops.append(k + 1)
    random.shuffle(ops)
    return factors, ops


def new_for_frame(i, clip_len, same_on_clip, same_across_clip):
    return (not same_on_clip) or ((not same_across_clip) and i % clip_len == 0 and i > 0)


def sample_photometric(num_frames, clip_len, jitter=None, gray=None, blur=None):
    """decisions of ONE sample for the steps present (dicts of the step's arguments or None), consuming the
    RNGs like the reference's __call__s in pipeline order -> dict of per-frame arrays"""
    out = dict(jitter=np.zeros(num_frames, np.uint8), factors=np.full((num_frames, 4), np.nan),
               order=np.zeros((num_frames, 4), np.int8), gray=np.zeros(num_frames, np.uint8),
               blur=np.zeros(num_frames, np.uint8), sigma=np.zeros(num_frames))
    if jitter is not None:
        apply = np.random.rand() < jitter['p']
        factors, ops = jitter_get_params(jitter['ranges'])
        for i in range(num_frames):
            if new_for_frame(i, clip_len, jitter['same_on_clip'], jitter['same_across_clip']):
                apply = np.random.rand() < jitter['p']
                factors, ops = jitter_get_params(jitter['ranges'])
            out['jitter'][i] = apply
            out['factors'][i] = factors
            out['order'][i, :len(ops)] = ops
    if gray is not None:
        apply = np.random.rand() < gray['p']
        for i in range(num_frames):
            if new_for_frame(i, clip_len, gray['same_on_clip'], gray['same_across_clip']):
                apply = np.random.rand() < gray['p']
            out['gray'][i] = apply
    if blur is not None:
        apply = np.random.rand() < blur['p']
        sigma = random.uniform(*blur['sigma_range'])
        for i in range(num_frames):
            if new_for_frame(i, clip_len, blur['same_on_clip'], blur['same_across_clip']):
                apply = np.random.rand() < blur['p']
                sigma = random.uniform(*blur['sigma_range'])
            out['blur'][i] = apply
            out['sigma'][i] = sigma
    return out


# ---------------------------------------------------------------- pixel arithmetic (uint8 HxWx3 in, uint8 out)

def blend(x, d, alpha):
    """PIL ImagingBlend(degenerate, image, alpha): out = clip(trunc(d + alpha*(x - d))), fp32, no contraction;
    alpha == 0 / 1 return a copy of the degenerate / the image"""
    if alpha == 0.0:
        return np.broadcast_to(np.asarray(d, np.uint8), x.shape).copy()
    if alpha == 1.0:
        return x.copy()
    a = np.float32(alpha)
    xi, di = x.astype(np.int32), np.asarray(d, np.int32)
    t = di.astype(np.float32) + (a * (xi - di).astype(np.float32)).astype(np.float32)
    return np.clip(np.trunc(np.nan_to_num(t, nan=0.0)), 0, 255).astype(np.uint8)


def luma(x):
    """PIL RGB -> L: (R*19595 + G*38470 + B*7471 + 0x8000) >> 16"""
    x = x.astype(np.int64)
    return ((x[..., 0] * 19595 + x[..., 1] * 38470 + x[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def adjust_brightness(x, factor):
    return blend(x, 0, factor)


def adjust_saturation(x, factor):
    return blend(x, luma(x)[..., None], factor)


def contrast_mean(x):
    """ImageEnhance.Contrast: int(ImageStat.Stat(image.convert('L')).mean[0] + 0.5)"""
    lum = luma(x)
    return int(float(lum.astype(np.int64).sum()) / lum.size + 0.5)


def adjust_contrast(x, factor):
    return blend(x, contrast_mean(x), factor)


def rgb2hsv(x):
    """Pillow Convert.c rgb2hsv_row"""
    r, g, b = (x[..., c].astype(np.int32) for c in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = maxc == minc
    with np.errstate(divide='ignore', invalid='ignore'):
        cr = (maxc - minc).astype(np.float32)
        s = cr / maxc.astype(np.float32)
        rc, gc, bc = ((maxc - c).astype(np.float32) / cr for c in (r, g, b))
        h = np.where(r == maxc, bc - gc,
                     np.where(g == maxc, ((2.0 + rc.astype(np.float64)) - bc.astype(np.float64)).astype(np.float32),
                              ((4.0 + gc.astype(np.float64)) - rc.astype(np.float64)).astype(np.float32)))
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
        uh = np.clip(np.trunc(h.astype(np.float64) * 255.0), 0, 255)
        us = np.clip(np.trunc(s.astype(np.float64) * 255.0), 0, 255)
    uh = np.where(grey, 0, np.nan_to_num(uh)).astype(np.uint8)
    us = np.where(grey, 0, np.nan_to_num(us)).astype(np.uint8)
    return np.stack([uh, us, maxc.astype(np.uint8)], -1)


def _round_half_away(v):
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def hsv2rgb(x):
    """Pillow Convert.c hsv2rgb"""
    h, s, v = (x[..., c].astype(np.float64) for c in range(3))
    hf = h * 6.0 / 255.0
    i = np.floor(hf)
    f = (hf - i).astype(np.float32)
    fs = (s.astype(np.float32) / 255.0).astype(np.float32)
    p = np.clip(_round_half_away(v * (1.0 - fs.astype(np.float64))), 0, 255).astype(np.uint8)
    q = np.clip(_round_half_away(v * (1.0 - (fs * f).astype(np.float64))), 0, 255).astype(np.uint8)
    t = np.clip(_round_half_away(v * (1.0 - fs.astype(np.float64) * (1.0 - f.astype(np.float64)))), 0, 255).astype(np.uint8)
    vv = x[..., 2]
    sel = i.astype(np.int64) % 6
    r = np.choose(sel, [vv, q, p, p, t, vv])
    g = np.choose(sel, [t, vv, vv, q, p, p])
    b = np.choose(sel, [p, p, t, vv, vv, q])
    out = np.stack([r, g, b], -1)
    return np.where((x[..., 1] == 0)[..., None], vv[..., None], out).astype(np.uint8)


def hue_shift(hue_factor):
    """torchvision 0.7 adjust_hue: np.uint8(hue_factor * 255) (numpy 1.x: truncate, wrap mod 256)"""
    return int(math.trunc(hue_factor * 255)) % 256


def adjust_hue(x, factor):
    hsv = rgb2hsv(x)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + hue_shift(factor)) & 255).astype(np.uint8)
    return hsv2rgb(hsv)


def rgb2gray(x):
    """mmcv.rgb2gray = cv2.cvtColor(RGB2GRAY) on 8-bit data (fixed point, 14 bits) repeated to 3 channels.
    cv2 is absent: parity with the reference UNPINNED."""
    x = x.astype(np.int64)
    gy = ((x[..., 0] * 4899 + x[..., 1] * 9617 + x[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)
    return np.repeat(gy[..., None], 3, -1)


def blur_weights(sigma):
    """PIL GaussianBlur(radius=sigma) -> extended box radius (_gaussian_blur_radius, 3 passes) -> (ww, fw) of
    ImagingHorizontalBoxBlur.  Only box radii below 1 (int part 0) are supported."""
    f32 = np.float32
    r = f32(sigma)
    s2 = f32(f32(r * r) / f32(3))
    L = f32(math.sqrt(12.0 * float(s2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * s2)))
    a = f32(a / f32(f32(6) * f32(s2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    rad = f32(l + a)
    if int(rad) != 0:
        raise NotImplementedError(f'GaussianBlur sigma {sigma}: box radius {float(rad)} >= 1')
    ww = int(f32(f32(1 << 24) / f32(rad * f32(2) + f32(1))))
    fw = ((1 << 24) - ww) // 2
    return ww, fw


def _box_pass(x, ww, fw, axis):
    x = x.astype(np.int64)
    n = x.shape[axis]
    lo = np.take(x, np.clip(np.arange(n) - 1, 0, n - 1), axis=axis)
    hi = np.take(x, np.clip(np.arange(n) + 1, 0, n - 1), axis=axis)
    return ((x * ww + (lo + hi) * fw + (1 << 23)) >> 24).astype(np.uint8)


def gaussian_blur(x, sigma=None, weights=None):
    """PIL GaussianBlur: three horizontal box passes, then three vertical, uint8 after every pass"""
    ww, fw = weights if weights is not None else blur_weights(sigma)
    for _ in range(3):
        x = _box_pass(x, ww, fw, 1)
    for _ in range(3):
        x = _box_pass(x, ww, fw, 0)
    return x


_JITTER_FN = {BRIGHTNESS: adjust_brightness, CONTRAST: adjust_contrast, SATURATION: adjust_saturation, HUE: adjust_hue}


def apply_frame(x, jitter, factors, order, gray, blur, sigma):
    """the three steps on one uint8 HxWx3 frame, in pipeline order"""
    if jitter:
        for op in order:
            if op:
                x = _JITTER_FN[int(op)](x, float(factors[int(op) - 1]))
    if gray:
        x = rgb2gray(x)
    if blur:
        x = gaussian_blur(x, float(sigma))
    return x


def pack_photometric(photo):
    """per-frame decisions -> the int32 [F][8] parameter rows of vfs_crop_resize_flip_photo_norm"""
    F = len(photo['jitter'])
    rows = np.zeros((F, PHOTO_WORDS), np.int32)
    for i in range(F):
        if photo['jitter'][i]:
            code = 0
            for k, op in enumerate(photo['order'][i]):
                code |= int(op) << (4 * k)
            rows[i, 0] = code
            for k in range(3):
                if not math.isnan(photo['factors'][i][k]):
                    rows[i, 1 + k] = np.float32(photo['factors'][i][k]).view(np.int32)
            if not math.isnan(photo['factors'][i][3]):
                rows[i, 4] = hue_shift(float(photo['factors'][i][3]))
        rows[i, 5] = int(photo['gray'][i])
        if photo['blur'][i]:
            rows[i, 6], rows[i, 7] = blur_weights(float(photo['sigma'][i]))
    return rows


def apply_packed(x, row):
    """apply_frame driven by one packed parameter row (what the kernel reads)"""
    code = int(row[0]) & 0xFFFF
    for k in range(4):
        op = (code >> (4 * k)) & 15
        if op in (BRIGHTNESS, CONTRAST, SATURATION):
            x = _JITTER_FN[op](x, float(np.int32(row[op]).view(np.float32)))
        elif op == HUE:
            hsv = rgb2hsv(x)
            hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + (int(row[4]) & 255)) & 255).astype(np.uint8)
            x = hsv2rgb(hsv)
    if row[5]:
        x = rgb2gray(x)
    if row[6]:
        x = gaussian_blur(x, weights=(int(row[6]), int(row[7])))
    return x
