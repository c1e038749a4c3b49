#!/usr/bin/env python3
"""Golden photometric decisions and frames from the REAL reference pipeline classes
(/root/reference/mmaction/datasets/pipelines/augmentations.py: ColorJitter, RandomGrayScale, RandomGaussianBlur),
run in the build container only, with the real Pillow.  Stand-ins for what is absent here:

* torchvision (0.7) ColorJitter: `_check_input` / `get_params` restated (random.uniform per enabled component, in the
  order brightness, contrast, saturation, hue, then random.shuffle of the ops); the ops are PIL ImageEnhance
  Brightness / Contrast / Color and 0.7's adjust_hue recipe (HSV split, H += np.uint8(factor * 255) with numpy 1.x's
  wrap, merge).  Every transform records its factors and order when it is applied.
* mmcv.rgb2gray: cv2.cvtColor(RGB2GRAY)'s 8-bit fixed point (cv2 absent: parity of THIS step unpinned).
* PIL.ImageFilter.GaussianBlur is wrapped to record the sigma it is built with.

Which frames a step changed is read from the result list (a step replaces results['imgs'][i] only when it applies).

Usage: python tests/golden/gen_photometric_golden.py  (writes tests/golden/photometric.npz)"""
import math
import os
import random
import sys

import numpy as np
from PIL import Image, ImageEnhance, ImageFilter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_pipeline_golden import import_reference_augmentations  # noqa: E402

LOG = []


def check_input(value, center=1, bound=(0, float('inf')), clip_first_on_zero=True):
    if isinstance(value, (int, float)):
        value = [center - value, center + value]
        if clip_first_on_zero:
            value[0] = max(value[0], 0)
    else:
        value = list(value)
    if value[0] == value[1] == center:
        value = None
    return value


def adjust_hue(img, hue_factor):
    h, s, v = img.convert('HSV').split()
    shift = int(math.trunc(hue_factor * 255)) % 256       # np.uint8(hue_factor * 255) of numpy 1.x
    nh = ((np.asarray(h).astype(np.int32) + shift) & 255).astype(np.uint8)
    return Image.merge('HSV', (Image.fromarray(nh, 'L'), s, v)).convert(img.mode)


class ColorJitterStandin:
    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        self.brightness = check_input(brightness)
        self.contrast = check_input(contrast)
        self.saturation = check_input(saturation)
        self.hue = check_input(hue, center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)

    @staticmethod
    def get_params(brightness, contrast, saturation, hue):
        factors, ops = [math.nan] * 4, []
        for k, r in enumerate((brightness, contrast, saturation, hue)):
            if r is not None:
                factors[k] = random.uniform(r[0], r[1])
                ops.append(k + 1)
        random.shuffle(ops)
        fns = {1: lambda im: ImageEnhance.Brightness(im).enhance(factors[0]),
               2: lambda im: ImageEnhance.Contrast(im).enhance(factors[1]),
               3: lambda im: ImageEnhance.Color(im).enhance(factors[2]),
               4: lambda im: adjust_hue(im, factors[3])}

        def transform(img):
            LOG.append(('jitter', list(factors), list(ops)))
            for op in ops:
                img = fns[op](img)
            return img
        return transform


class RecordingBlur(ImageFilter.GaussianBlur):
    def __init__(self, radius=2):
        LOG.append(('blur', radius))
        super().__init__(radius)


def rgb2gray(img, keepdim=False):
    x = img.astype(np.int64)
    g = ((x[..., 0] * 4899 + x[..., 1] * 9617 + x[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)
    return g[..., None] if keepdim else g


def main():
    aug = import_reference_augmentations()
    aug._ColorJitter = ColorJitterStandin
    aug.mmcv.rgb2gray = rgb2gray
    ImageFilter.GaussianBlur = RecordingBlur
    out = {}
    cases = [   # name, (H, W), num_clips, clip_len, same_on_clip, same_across_clip, samples, seed, jitter args, p gray, p blur
        ('cfg_r18', (10, 12), 2, 4, False, False, 4, 7, (0.4, 0.4, 0.4, 0.1, 0.8), 0.2, 0.5),
        ('cfg_r50', (9, 14), 2, 1, False, False, 8, 8, (0.4, 0.4, 0.4, 0.1, 0.8), 0.2, 0.5),
        ('per_clip', (8, 11), 2, 4, True, False, 6, 9, (0.4, 0.4, 0.4, 0.1, 0.8), 0.5, 0.5),
        ('shared', (7, 9), 2, 4, True, True, 6, 10, (0.4, 0.4, 0.4, 0.1, 0.8), 0.5, 0.5),
        ('no_hue', (8, 8), 2, 1, False, True, 8, 11, (0.3, 0.5, 0.0, 0.0, 0.9), 0.3, 0.7),
    ]
    g = np.random.default_rng(0)
    for name, (h, w), nclips, clip_len, soc, sac, nsamp, seed, (jb, jc, js, jh, jp), gp, bp in cases:
        np.random.seed(seed)
        random.seed(seed)
        kw = dict(same_on_clip=soc, same_across_clip=sac)
        steps = [aug.ColorJitter(brightness=jb, contrast=jc, saturation=js, hue=jh, p=jp, **kw), aug.RandomGrayScale(p=gp, **kw),
                 aug.RandomGaussianBlur(p=bp, **kw)]
        nf = nclips * clip_len
        rec = {k: [] for k in ('src', 'out', 'jitter', 'gray', 'blur', 'factors', 'order', 'sigma', 'factors_all', 'order_all',
                               'sigma_all')}
        for _ in range(nsamp):
            src = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(nf)]
            res = dict(imgs=list(src), clip_len=clip_len, num_clips=nclips, modality='RGB')
            flags = []
            for step in steps:
                before = list(res['imgs'])
                del LOG[:]
                res = step(res)
                applied = [res['imgs'][i] is not before[i] for i in range(nf)]
                flags.append(applied)
                log = iter(list(LOG))
                for i in range(nf):
                    if step is steps[0]:
                        fac, order = [math.nan] * 4, [0] * 4
                        if applied[i]:
                            _, fac, ops = next(log)
                            order = ops + [0] * (4 - len(ops))
                            rec['factors'].append(fac)
                            rec['order'].append(order)
                        rec['factors_all'].append(fac)
                        rec['order_all'].append(order)
                    elif step is steps[2]:
                        sg = 0.0
                        if applied[i]:
                            sg = next(log)[1]
                            rec['sigma'].append(sg)
                        rec['sigma_all'].append(sg)
            rec['jitter'] += flags[0]
            rec['gray'] += flags[1]
            rec['blur'] += flags[2]
            rec['src'] += src
            rec['out'] += [np.asarray(im, np.uint8) for im in res['imgs']]
        for k in ('src', 'out'):
            out[f'{name}/{k}'] = np.stack(rec[k])
        for k in ('jitter', 'gray', 'blur'):
            out[f'{name}/{k}'] = np.asarray(rec[k], np.uint8)
        out[f'{name}/factors'] = np.asarray(rec['factors'], np.float64).reshape(-1, 4)
        out[f'{name}/order'] = np.asarray(rec['order'], np.int8).reshape(-1, 4)
        out[f'{name}/sigma'] = np.asarray(rec['sigma'], np.float64)
        out[f'{name}/factors_all'] = np.asarray(rec['factors_all'], np.float64)
        out[f'{name}/order_all'] = np.asarray(rec['order_all'], np.int8)
        out[f'{name}/sigma_all'] = np.asarray(rec['sigma_all'], np.float64)
        out[f'{name}/meta'] = np.asarray([h, w, nclips, clip_len, nsamp, seed], np.int64)
        out[f'{name}/same'] = np.asarray([soc, sac], np.uint8)
        out[f'{name}/jitter_args'] = np.asarray([jb, jc, js, jh], np.float64)
        out[f'{name}/probs'] = np.asarray([jp, gp, bp], np.float64)
        out[f'{name}/sigma_range'] = np.asarray([0.1, 0.2], np.float64)
        print(name, 'jitter', out[f'{name}/jitter'].sum(), 'gray', out[f'{name}/gray'].sum(), 'blur', out[f'{name}/blur'].sum(),
              'of', nf * nsamp)
    path = os.environ.get('VFS_GOLDEN_OUT', HERE)
    np.savez_compressed(os.path.join(path, 'photometric.npz'), **out)


if __name__ == '__main__':
    main()
