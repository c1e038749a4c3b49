#!/usr/bin/env python3
"""Updates per second of the SiamFC probe over K sequences: SiamFCProbe(device_loop=True).track() one sequence after another
(state on the host, one 16-byte read-back per frame) against SiamFCProbe.track_batch (state on the device, `batch` slots in
lock-step, nothing read back before the end) with batch in 1, 4, 16, 32.

Protocol: K synthetic textured 60-frame 480 x 640 sequences (bench_siamfc_track.sequence; 8 distinct ones, repeated), the same
seeded weights in every arm; one warm-up pass per arm, then `--repeats` timed passes per arm, the arms alternating, in one
process.  A pass is timed by the host clock between device synchronises; updates = K * (frames - 1) (frame 0 is the init).
The boxes of every track_batch arm are compared with the first arm's (largest difference over all frames).

Usage: python tools/bench_siamfc_batch.py [--depth 18] [--sequences 32] [--frames 60] [--size 480x640] [--repeats 5] [--out FILE.json]
On a shared box run each depth as its own step under a time limit, chained:
  timeout -k 10 600 python tools/bench_siamfc_batch.py --depth 18 --out profiles/siamfc_batch_bench_r18.json && \\
  timeout -k 10 900 python tools/bench_siamfc_batch.py --depth 50 --out profiles/siamfc_batch_bench_r50.json"""
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit('/tools/', 1)[0] + '/tools')
sys.path.insert(0, __file__.rsplit('/tools/', 1)[0])
from bench_siamfc_track import _arg, probes, sequence  # noqa: E402

BATCHES = (1, 4, 16, 32)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    depth, K, nframes, repeats = int(_arg('--depth', 18)), int(_arg('--sequences', 32)), int(_arg('--frames', 60)), int(_arg('--repeats', 5))
    H, W = (int(v) for v in _arg('--size', '480x640').split('x'))
    out = _arg('--out', None)
    if not torch.cuda.is_available():
        raise SystemExit('bench_siamfc_batch: needs the GPU (a CPU timing says nothing about it)')
    distinct = [sequence(nframes, H, W, seed=s) for s in range(min(K, 8))]
    seqs, boxes = [distinct[k % len(distinct)][0] for k in range(K)], [distinct[k % len(distinct)][1] for k in range(K)]
    _, probe = probes(depth, torch.device('cuda:0'))
    arms = {'track_one_by_one': lambda: [probe.track(q, b) for q, b in zip(seqs, boxes)]}
    for n in BATCHES:
        arms[f'track_batch_{n}'] = lambda n=n: probe.track_batch(seqs, boxes, batch=n)
    first = {name: timed(fn)[1] for name, fn in arms.items()}      # warm-up: code objects, workspaces, the allocator's pools
    updates = K * (nframes - 1)
    ups = {name: [] for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            ups[name].append(updates / timed(fn)[0])
    ref = first['track_one_by_one']
    diff = {name: max(float(np.abs(a - b).max()) for a, b in zip(res, ref)) for name, res in first.items() if name != 'track_one_by_one'}
    med = {name: statistics.median(v) for name, v in ups.items()}
    res = dict(device=torch.cuda.get_device_name(0), depth=depth, frame=[H, W], sequences=K, frames=nframes, repeats=repeats,
               timing='host clock around a pass over all sequences between device synchronises, arms alternating after one warm-up pass each; sequences * (frames - 1) / time',
               updates_per_s={name: [round(v, 1) for v in vals] for name, vals in ups.items()},
               updates_per_s_median={name: round(v, 1) for name, v in med.items()},
               over_one_by_one={name: round(v / med['track_one_by_one'], 3) for name, v in med.items()},
               largest_box_difference_to_one_by_one=diff, boxes_identical=all(v == 0.0 for v in diff.values()))
    print(json.dumps(res))
    if out:
        with open(out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
