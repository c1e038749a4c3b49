#!/usr/bin/env python3
"""Golden data for blurs of box radius 1 and above (tests/test_photometric_wide_blur.py), run in the build container only,
with the real Pillow:

* `draw/...`: the REAL reference RandomGaussianBlur (mmaction/datasets/pipelines/augmentations.py) with
  sigma_range=(0.1, 2.0) on small random frames: which frames it blurred, the sigma PIL's GaussianBlur was built with,
  and the frames it returned.
* `pil/<k>/...`: (input, sigma, PIL.ImageFilter.GaussianBlur(sigma) output) triples at fixed sigmas whose box radii have
  the integer parts 0, 1, 2, 3 and 4, on sizes smaller than the window too.

Usage: python tests/golden/gen_wide_blur_golden.py  (writes tests/golden/wide_blur.npz)"""
import os
import random
import sys

import numpy as np
from PIL import Image, ImageFilter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_pipeline_golden import import_reference_augmentations  # noqa: E402

LOG = []
PlainBlur = ImageFilter.GaussianBlur


class RecordingBlur(PlainBlur):
    def __init__(self, radius=2):
        LOG.append(radius)
        super().__init__(radius)


def main():
    aug = import_reference_augmentations()
    out = {}
    g = np.random.default_rng(1)
    cases = [   # name, (H, W), num_clips, clip_len, same_on_clip, same_across_clip, samples, seed, p
        ('per_frame', (7, 9), 2, 4, False, False, 3, 21, 0.5),
        ('per_clip', (6, 7), 2, 4, True, False, 4, 22, 0.7),
        ('shared', (5, 6), 2, 2, True, True, 4, 23, 0.6),
    ]
    ImageFilter.GaussianBlur = RecordingBlur
    for name, (h, w), nclips, clip_len, soc, sac, nsamp, seed, p in cases:
        np.random.seed(seed)
        random.seed(seed)
        step = aug.RandomGaussianBlur(sigma_range=(0.1, 2.0), p=p, same_on_clip=soc, same_across_clip=sac)
        nf = nclips * clip_len
        srcs, outs, blur, sigma = [], [], [], []
        for _ in range(nsamp):
            src = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(nf)]
            del LOG[:]
            res = step(dict(imgs=list(src), clip_len=clip_len, num_clips=nclips, modality='RGB'))
            applied = [res['imgs'][i] is not src[i] for i in range(nf)]
            log = iter(list(LOG))
            sigma += [next(log) if a else 0.0 for a in applied]
            blur += applied
            srcs += src
            outs += [np.asarray(im, np.uint8) for im in res['imgs']]
        out[f'draw/{name}/src'], out[f'draw/{name}/out'] = np.stack(srcs), np.stack(outs)
        out[f'draw/{name}/blur'] = np.asarray(blur, np.uint8)
        out[f'draw/{name}/sigma'] = np.asarray(sigma, np.float64)
        out[f'draw/{name}/meta'] = np.asarray([h, w, nclips, clip_len, nsamp, seed], np.int64)
        out[f'draw/{name}/same'] = np.asarray([soc, sac], np.uint8)
        out[f'draw/{name}/p'] = np.asarray(p, np.float64)
        print(name, 'blur', int(np.sum(blur)), 'of', nf * nsamp, 'max sigma', max(sigma))
    ImageFilter.GaussianBlur = PlainBlur
    k = 0
    for sigma in (0.2, 0.9, 1.0, 1.5, 2.0, 3.0, 3.9, 5.0):
        for h, w in ((8, 11), (5, 3), (2, 9), (1, 1)):
            x = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
            out[f'pil/{k}/in'], out[f'pil/{k}/sigma'] = x, np.asarray(sigma, np.float64)
            out[f'pil/{k}/out'] = np.asarray(Image.fromarray(x).filter(PlainBlur(radius=sigma)), np.uint8)
            k += 1
    path = os.environ.get('VFS_GOLDEN_OUT', HERE)
    np.savez_compressed(os.path.join(path, 'wide_blur.npz'), **out)


if __name__ == '__main__':
    main()
