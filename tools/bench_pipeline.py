#!/usr/bin/env python3
"""Time the fused crop/resize/flip/normalise kernel on the reference's training shapes
(340x256 decoded frames -> 224x224, 2 frames per sample) and print its HBM roofline fraction.

--color: the plain pipeline against the colour pipeline of the object-level configs (ColorJitter p=0.8,
RandomGrayScale p=0.2, RandomGaussianBlur p=0.5 between Flip and Normalize, decisions sampled), fp32 imgs out."""
import json
import random
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit('/tools/', 1)[0])
from vfs_amd.pipeline import GpuTrainPipeline  # noqa: E402

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


COLOR_STEPS = [dict(type='ColorJitter', brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p=0.8, same_across_clip=False,
                    same_on_clip=False),
               dict(type='RandomGrayScale', p=0.2, same_across_clip=False, same_on_clip=False),
               dict(type='RandomGaussianBlur', p=0.5, same_across_clip=False, same_on_clip=False)]


def _time(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def color(B):
    dev = torch.device('cuda:0')
    head = [dict(type='RandomResizedCrop', area_range=(0.2, 1.), same_across_clip=False, same_on_clip=False),
            dict(type='Resize', scale=(224, 224), keep_ratio=False),
            dict(type='Flip', flip_ratio=0.5, same_across_clip=False, same_on_clip=False)]
    tail = [dict(type='Normalize', mean=MEAN, std=STD, to_bgr=False), dict(type='FormatShape', input_format='NCTHW')]
    plain, colour = GpuTrainPipeline(head + tail, 2, 1), GpuTrainPipeline(head + COLOR_STEPS + tail, 2, 1)
    np.random.seed(0)
    random.seed(0)
    frames = torch.randint(0, 256, (B, 2, 256, 340, 3), dtype=torch.uint8, device=dev)
    draws = [colour.sample(2, (256, 340)) for _ in range(B)]
    boxes, flips = np.concatenate([d[0] for d in draws]), np.concatenate([d[1] for d in draws])
    photo = {k: np.concatenate([d[2][k] for d in draws]) for k in draws[0][2]}
    from vfs_amd.pipeline import pack_photometric
    rows = pack_photometric(photo)
    res = dict(B=B, frames=2 * B, jitter=int(photo['jitter'].sum()), gray=int(photo['gray'].sum()), blur=int(photo['blur'].sum()))
    for name, fn in [('plain', lambda: plain(frames, boxes=boxes, flips=flips)),
                     ('color', lambda: colour(frames, boxes=boxes, flips=flips, photo=rows))]:
        ms = _time(fn)
        res[name] = dict(ms=round(ms, 4), frames_per_s=round(2 * B / ms * 1e3))
    print(json.dumps(res))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    B = int(args[0]) if args else 128
    if '--color' in sys.argv:
        return color(B)
    dev = torch.device('cuda:0')
    pipe = GpuTrainPipeline([dict(type='RandomResizedCrop', area_range=(0.2, 1.), same_across_clip=False, same_on_clip=False),
                             dict(type='Resize', scale=(224, 224), keep_ratio=False),
                             dict(type='Flip', flip_ratio=0.5, same_across_clip=False, same_on_clip=False),
                             dict(type='Normalize', mean=MEAN, std=STD, to_bgr=False),
                             dict(type='FormatShape', input_format='NCTHW')], 2, 1)
    np.random.seed(0)
    random.seed(0)
    frames = torch.randint(0, 256, (B, 2, 256, 340, 3), dtype=torch.uint8, device=dev)
    bs, fs = zip(*[pipe.sample(2, (256, 340)) for _ in range(B)])
    boxes, flips = np.concatenate(bs), np.concatenate(fs)
    res = {}
    for name, kw in [('imgs', dict(want_imgs=True, want_x4=False)), ('x4', dict(want_imgs=False, want_x4=True))]:
        for _ in range(3):
            pipe(frames, boxes=boxes, flips=flips, **kw)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20
        e0.record()
        for _ in range(n):
            pipe(frames, boxes=boxes, flips=flips, **kw)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / n
        crop_bytes = float(((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])).sum()) * 3
        out_bytes = 2 * B * 224 * 224 * (12 if name == 'imgs' else 8)
        res[name] = dict(ms=round(ms, 4), frames_per_s=round(2 * B / ms * 1e3), GBps=round((crop_bytes + out_bytes) / ms / 1e6, 1),
                         alg_MB=round((crop_bytes + out_bytes) / 1e6, 1))
    print(json.dumps(dict(B=B, **res)))


if __name__ == '__main__':
    main()
