#!/usr/bin/env python3
"""Time the fused crop/resize/flip/normalise kernel on the reference's training shapes
(340x256 decoded frames -> 224x224, 2 frames per sample) and print its HBM roofline fraction.

--color [--arms plain,color,wide] [--out FILE]: the plain pipeline against the colour pipeline of the object-level configs
(ColorJitter p=0.8, RandomGrayScale p=0.2, RandomGaussianBlur p=0.5 between Flip and Normalize, decisions sampled) and
against the same steps with sigma_range=(0.1, 2.0) at max_blur_radius=1 (wide), fp32 imgs out; arms interleaved.

--ragged [--out FILE]: batches of mixed frame sizes.  B samples of 2 frames at the four sizes DecordDecode returns for
Kinetics-400, repeated, -> 224x224, through ONE ragged call (plain and colour) against what the uniform entry points offer
for the same frames: one call per size group and a torch.cat of the outputs.  Second comparison: a uniform 340x256 batch
through the uniform and through the ragged entry points.  Arms are interleaved, ROUNDS rounds; per arm the median and
the min / max over the rounds of (call) the whole GpuTrainPipeline call and (launch) the C entries alone, replayed on
prebuilt device arguments."""
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


def color(B, arms=('plain', 'color', 'wide'), out_path=None):
    """arms: plain; color = the object-level configs' steps (sigma_range (0.1, 0.2)); wide = the same steps with the blur of
    the SimSiam / BYOL recipes, sigma_range (0.1, 2.0), at max_blur_radius=1.  Same frames, boxes, flips and the same
    jitter / grey / blur flags for color and wide (one draw of the RNGs each, from the same seed); the arms are interleaved,
    ROUNDS rounds of 20 calls, `ms` = the median round, with the min / max over the rounds beside it."""
    from vfs_amd.pipeline import pack_photometric
    dev = torch.device('cuda:0')
    head = [dict(type='RandomResizedCrop', area_range=(0.2, 1.), same_across_clip=False, same_on_clip=False),
            dict(type='Resize', scale=(224, 224), keep_ratio=False),
            dict(type='Flip', flip_ratio=0.5, same_across_clip=False, same_on_clip=False)]
    tail = [dict(type='Normalize', mean=MEAN, std=STD, to_bgr=False), dict(type='FormatShape', input_format='NCTHW')]
    wide_steps = COLOR_STEPS[:2] + [dict(COLOR_STEPS[2], sigma_range=(0.1, 2.0))]
    plain, colour = GpuTrainPipeline(head + tail, 2, 1), GpuTrainPipeline(head + COLOR_STEPS + tail, 2, 1)
    frames = torch.randint(0, 256, (B, 2, 256, 340, 3), dtype=torch.uint8, device=dev)

    def decisions(pipe):
        np.random.seed(0)
        random.seed(0)
        draws = [pipe.sample(2, (256, 340)) for _ in range(B)]
        photo = {k: np.concatenate([d[2][k] for d in draws]) for k in draws[0][2]}
        return np.concatenate([d[0] for d in draws]), np.concatenate([d[1] for d in draws]), photo
    boxes, flips, photo = decisions(colour)
    rows = pack_photometric(photo)
    res = dict(B=B, frames=2 * B, rounds=ROUNDS, jitter=int(photo['jitter'].sum()), gray=int(photo['gray'].sum()),
               blur=int(photo['blur'].sum()))
    fns = dict(plain=lambda: plain(frames, boxes=boxes, flips=flips), color=lambda: colour(frames, boxes=boxes, flips=flips, photo=rows))
    if 'wide' in arms:
        wide = GpuTrainPipeline(head + wide_steps + tail, 2, 1, max_blur_radius=1)
        wboxes, wflips, wphoto = decisions(wide)
        assert np.array_equal(wboxes, boxes) and np.array_equal(wflips, flips) and np.array_equal(wphoto['blur'], photo['blur'])
        wrows = pack_photometric(wphoto, max_blur_radius=1)
        res['wide_radius_1_frames'] = int((((wrows[:, 4] >> 8) & 255) == 1).sum())
        fns['wide'] = lambda: wide(frames, boxes=boxes, flips=flips, photo=wrows)
    fns = {k: fns[k] for k in arms}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            times[k].append(_window(fn, 20))
    for k, t in times.items():
        sp = _spread(t)
        res[k] = dict(ms=sp['median_ms'], min_ms=sp['min_ms'], max_ms=sp['max_ms'], frames_per_s=round(2 * B / sp['median_ms'] * 1e3))
    print(json.dumps(res))
    if out_path:
        with open(out_path, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


K400 = [(256, 340), (256, 454), (340, 256), (256, 342)]      # (Hs, Ws)
ROUNDS = 9


class _Capture:
    """stands in for the library during one call: keeps the C entries and their (device) arguments for replay"""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*args):
            if 'workspace_bytes' not in name:
                self.calls.append((fn, args))
            return fn(*args)
        return call


def _window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _spread(v):
    v = sorted(v)
    return dict(median_ms=round(v[len(v) // 2], 4), min_ms=round(v[0], 4), max_ms=round(v[-1], 4))


def ragged(B, out_path=None):
    from vfs_amd import _lib
    from vfs_amd.pipeline import pack_frames, pack_photometric
    dev = torch.device('cuda:0')
    head = [dict(type='RandomResizedCrop', area_range=(0.2, 1.), same_across_clip=False, same_on_clip=False),
            dict(type='Resize', scale=(224, 224), keep_ratio=False),
            dict(type='Flip', flip_ratio=0.5, same_across_clip=False, same_on_clip=False)]
    tail = [dict(type='Normalize', mean=MEAN, std=STD, to_bgr=False), dict(type='FormatShape', input_format='NCTHW')]
    np.random.seed(0)
    random.seed(0)
    g = torch.Generator(device='cpu').manual_seed(0)
    arms, res = {}, dict(B=B, frames=2 * B, out='224x224 fp32 imgs', rounds=ROUNDS)

    def add(name, pipe, call):
        """call(pipe) runs the arm through GpuTrainPipeline; its C entries are captured once for the launch-only replay"""
        lib = _lib.get_lib()
        cap = _Capture(lib)
        _lib.set_lib(cap)
        try:
            call(pipe)
        finally:
            _lib.set_lib(lib)
        torch.cuda.synchronize()
        arms[name] = (lambda: call(pipe), lambda: [fn(*a) for fn, a in cap.calls], len(cap.calls))

    for kind, steps in (('plain', []), ('color', COLOR_STEPS)):
        pipe = GpuTrainPipeline(head + steps + tail, 2, 1)
        # ---- mixed sizes: sample b has size K400[b % 4]
        shapes = [K400[b % 4] for b in range(B)]
        samples = [torch.randint(0, 256, (2, h, w, 3), dtype=torch.uint8, generator=g).to(dev) for h, w in shapes]
        draws = [pipe.sample(2, s) for s in shapes]
        boxes, flips = np.concatenate([d[0] for d in draws]), np.concatenate([d[1] for d in draws])
        rows = pack_photometric({k: np.concatenate([d[2][k] for d in draws]) for k in draws[0][2]}) if steps else None
        packed = pack_frames(samples)
        groups = []      # what the uniform entry points offer: one dense tensor, and the decisions, per size
        for k in range(4):
            idx = [b for b in range(B) if b % 4 == k]
            fr = np.concatenate([[2 * b, 2 * b + 1] for b in idx])
            groups.append((torch.stack([samples[b] for b in idx]), boxes[fr], flips[fr], None if rows is None else rows[fr]))
        add(f'mixed_{kind}_ragged', pipe, lambda p, a=(packed, boxes, flips, rows): p(a[0], boxes=a[1], flips=a[2], photo=a[3]))
        add(f'mixed_{kind}_per_size_group', pipe,
            lambda p, gs=groups: torch.cat([p(f, boxes=b, flips=fl, photo=r)['imgs'] for f, b, fl, r in gs]))
        # ---- one size: the same decisions' sampler at 340x256 through both entry families
        dense = torch.randint(0, 256, (B, 2, 256, 340, 3), dtype=torch.uint8, generator=g).to(dev)
        draws = [pipe.sample(2, (256, 340)) for _ in range(B)]
        ub, uf = np.concatenate([d[0] for d in draws]), np.concatenate([d[1] for d in draws])
        ur = pack_photometric({k: np.concatenate([d[2][k] for d in draws]) for k in draws[0][2]}) if steps else None
        same = pack_frames(list(dense))
        add(f'uniform_{kind}_uniform_entry', pipe, lambda p, a=(dense, ub, uf, ur): p(a[0], boxes=a[1], flips=a[2], photo=a[3]))
        add(f'uniform_{kind}_ragged_entry', pipe, lambda p, a=(same, ub, uf, ur): p(a[0], boxes=a[1], flips=a[2], photo=a[3]))
    for call, launch, _ in arms.values():      # warm every shape of the timed windows
        for _ in range(3):
            call()
            launch()
    torch.cuda.synchronize()
    times = {name: dict(call=[], launch=[]) for name in arms}
    for _ in range(ROUNDS):                     # interleaved: every arm once per round
        for name, (call, launch, _) in arms.items():
            times[name]['call'].append(_window(call, 20))
            times[name]['launch'].append(_window(launch, 100))
    for name, t in times.items():
        res[name] = dict(c_entries=arms[name][2], call=_spread(t['call']), launch=_spread(t['launch']))
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    out_path = None
    if '--out' in sys.argv:
        out_path = sys.argv[sys.argv.index('--out') + 1]
        args.remove(out_path)
    arms = ('plain', 'color', 'wide')
    if '--arms' in sys.argv:
        text = sys.argv[sys.argv.index('--arms') + 1]
        args.remove(text)
        arms = tuple(text.split(','))
    B = int(args[0]) if args else 128
    if '--color' in sys.argv:
        return color(B, arms, out_path)
    if '--ragged' in sys.argv:
        return ragged(int(args[0]) if args else 32, out_path)
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
