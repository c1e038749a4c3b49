#!/usr/bin/env python3
"""Frames per second of SiamFCProbe.track() with the host loop (device_loop=False: numpy crops, two synchronous copies, numpy
up-sampling and peak search around the device's feature pass) and with the device loop (device_loop=True:
csrc/siamfc_track.hip, one frame upload and one 16-byte read-back per frame), and where the host loop's time goes.

Protocol: one synthetic textured sequence (a textured target moving over a textured background), the same probe weights in
both arms; each arm is warmed up on the whole sequence once, then the arms alternate, `--repeats` timed passes each, on the same
box in the same process.  A pass is timed by the host clock around track() with a device synchronise before each reading
(the device loop's only per-frame synchronisation is its read-back; the host loop ends every frame on the host anyway).
The per-stage split re-runs the host loop's own statements with a clock between them (device work closed by a synchronise):
crops (numpy) / upload + features + head + download / cubic up-sampling (numpy) / penalties, normalisation, Hann blend, argmax,
state update (numpy).  The weights are seeded stand-ins (the backbone filled as the test-suite fills it, an untrained head): the arithmetic per
frame does not depend on them, where the boxes go does.

Usage: python tools/bench_siamfc_track.py [--depth 50] [--frames 60] [--size 480x640] [--repeats 5] [--out FILE.json]"""
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit('/tools/', 1)[0])
import vfs_amd  # noqa: E402
from vfs_amd import siamfc as SF  # noqa: E402


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def sequence(frames, H, W, seed=0):
    rng = np.random.default_rng(seed)
    bg = np.kron(rng.integers(30, 140, (H // 8, W // 8, 3)).astype(np.float64), np.ones((8, 8, 1))) + rng.integers(-12, 13, (H, W, 3))
    side = max(8, min(64, H // 32 * 8))
    target = np.kron(rng.integers(150, 255, (side // 8, side // 8, 3)).astype(np.float64), np.ones((8, 8, 1))) + rng.integers(-10, 11, (side, side, 3))
    y0, x0, out = H // 3, W // 3, []
    for t in range(frames):
        img = bg.copy()
        y, x = y0 + (2 * t) % (H - y0 - side), x0 + (3 * t) % (W - x0 - side)
        img[y:y + side, x:x + side] = target
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out, [x0 + 1, y0 + 1, side, side]


def probes(depth, dev):
    from oracle import vfs_oracle as O      # the seeded fill of the test-suite: activations stay in range through 50 layers
    cfg = dict(out_channels=512 if depth < 50 else 2048)      # the head's 1x1 convs take the backbone's last stage
    host = vfs_amd.SiamFCProbe(cfg, depth=depth, device=dev)
    ref = O.ResNet(depth, strides=(1, 2, 1, 1), dilations=(1, 1, 2, 4), out_indices=(3,), zero_init_residual=False)
    O.fill_state_dict_(ref, seed=118)
    host.backbone.load_state_dict(ref.state_dict())
    device = vfs_amd.SiamFCProbe(cfg, depth=depth, device=dev, backbone=host.backbone, device_loop=True)
    device.head.load_state_dict(host.head.state_dict())
    return host, device


def timed_track(probe, frames, box):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    boxes = probe.track(frames, box)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, boxes


@torch.no_grad()
def host_update_staged(p, img, acc):
    """the statements of SiamFCProbe.update (host loop), a clock between the stages"""
    c = p.cfg
    t0 = time.perf_counter()
    x = np.stack([SF.crop_and_resize(img, p.center, p.x_sz * f, c['instance_sz'], p.avg_color) for f in p.scale_factors])
    t1 = time.perf_counter()
    x = torch.from_numpy(x).to(p.device).permute(0, 3, 1, 2).float()
    responses = p.head(p.kernel, p.features(x)).squeeze(1).cpu().numpy()
    t2 = time.perf_counter()
    responses = np.stack([SF.resize_cubic(u, p.upscale_sz, p.upscale_sz) for u in responses])
    t3 = time.perf_counter()
    responses[:c['scale_num'] // 2] *= c['scale_penalty']
    responses[c['scale_num'] // 2 + 1:] *= c['scale_penalty']
    scale_id = np.argmax(np.amax(responses, axis=(1, 2)))
    response = responses[scale_id]
    response -= response.min()
    response /= response.sum() + 1e-16
    response = (1 - c['window_influence']) * response + c['window_influence'] * p.hann_window
    loc = np.unravel_index(response.argmax(), response.shape)
    box = p._apply_peak(scale_id, loc)
    t4 = time.perf_counter()
    for k, d in zip(('crops_numpy', 'upload_features_head_download', 'upsample_numpy', 'peak_and_state_numpy'), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
        acc[k] = acc.get(k, 0.0) + d
    return box


def main():
    depth, nframes, repeats = int(_arg('--depth', 50)), int(_arg('--frames', 60)), int(_arg('--repeats', 5))
    H, W = (int(v) for v in _arg('--size', '480x640').split('x'))
    out = _arg('--out', None)
    if not torch.cuda.is_available():
        raise SystemExit('bench_siamfc_track: needs the GPU (a CPU timing says nothing about it)')
    dev = torch.device('cuda:0')
    frames, box = sequence(nframes, H, W)
    host, device = probes(depth, dev)
    _, hb = timed_track(host, frames, box)          # warm-up of both arms: code objects, workspaces, the allocator's pools
    _, db = timed_track(device, frames, box)
    fps = dict(host_loop=[], device_loop=[])
    for _ in range(repeats):                        # alternating arms
        for name, probe in (('host_loop', host), ('device_loop', device)):
            dt, _ = timed_track(probe, frames, box)
            fps[name].append((nframes - 1) / dt)    # frame 0 is init()
    acc = {}
    for _ in range(repeats):
        host.init(frames[0], box)
        torch.cuda.synchronize()
        for img in frames[1:]:
            host_update_staged(host, img, acc)
    n = repeats * (nframes - 1)
    med = {k: statistics.median(v) for k, v in fps.items()}
    res = dict(device=torch.cuda.get_device_name(0), depth=depth, frame=[H, W], frames=nframes, repeats=repeats,
               timing='host clock around track() (init + frames - 1 updates) between device synchronises, arms alternating after one warm-up pass each; (frames - 1) / time',
               fps_host_loop=[round(v, 2) for v in fps['host_loop']], fps_device_loop=[round(v, 2) for v in fps['device_loop']],
               fps_host_loop_median=round(med['host_loop'], 2), fps_device_loop_median=round(med['device_loop'], 2),
               ms_per_frame_host_loop=round(1e3 / med['host_loop'], 3), ms_per_frame_device_loop=round(1e3 / med['device_loop'], 3),
               device_over_host=round(med['device_loop'] / med['host_loop'], 3),
               host_loop_stage_ms_per_frame={k: round(1e3 * v / n, 3) for k, v in acc.items()},
               boxes_identical=bool(np.array_equal(hb, db)), largest_box_difference=float(np.abs(hb - db).max()))
    print(json.dumps(res))
    if out:
        with open(out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
