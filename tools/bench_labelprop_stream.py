"""Label propagation from ring banks: the streaming interface and forward_test_batch(..., ring=True) against the whole-clip paths.

Synthetic clips (tools/bench_labelprop_batch.py), the shipped test-time test_cfg of configs/vfs_r18.py / vfs_r50.py:
  davis   480 x 854, 30 frames, 3-D label maps        jhmdb   240 x 320, 40 frames, 16-channel soft maps
Arms, alternating inside every repeat on one box:
  forward_test      one video after another, every frame of a clip extracted first (unchanged code: the baseline)
  stream            open_stream + push, ONE frame per push: a backbone pass and an ingest launch per frame
  batch=B           forward_test_batch, whole-clip banks (unchanged code: the baseline)
  batch=B ring      forward_test_batch(..., ring=True): banks of precede_frames + 2 positions, one backbone pass per step
Per arm: ms per frame (median over the repeats, min .. max), torch.cuda.max_memory_allocated of one run, and whether its maps equal
forward_test's.  --arms forward_test batch runs on a checkout without the ring (the baseline on the parent commit).

  python tools/bench_labelprop_stream.py [--case davis jhmdb] [--depth 18 50] [--precision fp32 bf16] [--videos 8] [--repeats 3]
                                         [--batches 4 8] [--arms forward_test stream batch ring] [--out FILE.json]"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.bench_labelprop_batch import CASES, make_videos      # noqa: E402


def build_tracker(depth, precision, dev):
    import vfs_amd
    cfg = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', f'vfs_r{depth}.py'))
    tc = vfs_amd.ConfigDict(cfg.test_cfg)
    tc['precision'] = precision
    bb = dict(cfg.model['backbone'])
    bb['out_indices'], bb['strides'] = tc['out_indices'], tc['strides']
    torch.manual_seed(0)
    model = vfs_amd.build_model(dict(type='VanillaTracker', backbone=bb), train_cfg=None, test_cfg=tc)
    with torch.no_grad():
        for name, buf in model.named_buffers():
            if name.endswith('running_var'):
                buf.uniform_(0.5, 1.5)
            elif name.endswith('running_mean'):
                buf.normal_(0.0, 0.2)
    return model.to(dev).eval()


def stream_clip(model, imgs, ref, meta):
    frames = imgs[0]
    s = model.open_stream(frames[:, :, 0], ref, meta)
    rows = [s.first] + [s.push(frames[:, :, f]) for f in range(1, frames.size(2))]
    s.close()
    return np.concatenate(rows, axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', nargs='+', default=['davis', 'jhmdb'], choices=sorted(CASES))
    ap.add_argument('--depth', nargs='+', type=int, default=[18, 50], choices=[18, 50])
    ap.add_argument('--precision', nargs='+', default=['fp32', 'bf16'], choices=['fp32', 'bf16'])
    ap.add_argument('--videos', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batches', type=int, nargs='+', default=[4, 8])
    ap.add_argument('--arms', nargs='+', default=['forward_test', 'stream', 'batch', 'ring'], choices=['forward_test', 'stream', 'batch', 'ring'])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = torch.device('cuda:0')
    results = []
    for depth in args.depth:
        for precision in args.precision:
            model = build_tracker(depth, precision, dev)
            for name in args.case:
                case = CASES[name]
                imgs_list, refs, metas = make_videos(case, args.videos, dev)
                clips = list(zip(imgs_list, refs, metas))
                frames = args.videos * case['frames']
                arms = []
                if 'forward_test' in args.arms:
                    arms.append(('forward_test', lambda: [model(a, return_loss=False, ref_seg_map=b, img_meta=c)[0] for a, b, c in clips]))
                if 'stream' in args.arms:
                    arms.append(('stream', lambda: [stream_clip(model, a, b, c) for a, b, c in clips]))
                for b in args.batches:
                    if 'batch' in args.arms:
                        arms.append((f'batch={b}', lambda b=b: model.forward_test_batch(imgs_list, refs, metas, batch=b)))
                    if 'ring' in args.arms:
                        arms.append((f'batch={b} ring', lambda b=b: model.forward_test_batch(imgs_list, refs, metas, batch=b, ring=True)))
                want, equal, peak = None, {}, {}
                for arm, fn in arms:      # warm-up of every arm, its peak memory and its maps against the first arm's
                    torch.cuda.synchronize()
                    gc.collect()      # the banks of the arm before must be gone before this arm's peak is read
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    got = fn()
                    torch.cuda.synchronize()
                    peak[arm] = torch.cuda.max_memory_allocated() - base
                    if want is None:
                        want = got
                    else:
                        equal[arm] = all(np.array_equal(a, b) for a, b in zip(got, want))
                    del got
                times = {arm: [] for arm, _ in arms}
                for _ in range(args.repeats):
                    for arm, fn in arms:      # alternating: clock and thermal drift hit every arm alike
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        times[arm].append(time.perf_counter() - t0)
                for arm, _ in arms:
                    ts = sorted(times[arm])
                    med = ts[len(ts) // 2]
                    row = dict(case=name, depth=depth, precision=precision, arm=arm, videos=args.videos, frames_per_video=case['frames'],
                               size=list(case['size']), ms_per_frame=round(1e3 * med / frames, 4), ms_per_frame_min=round(1e3 * ts[0] / frames, 4),
                               ms_per_frame_max=round(1e3 * ts[-1] / frames, 4), repeats=args.repeats,
                               peak_mb_above_inputs=round(peak[arm] / 2 ** 20, 1), equals_first_arm=equal.get(arm))
                    results.append(row)
                    print(json.dumps(row), flush=True)
                del imgs_list, refs, metas, clips, want
                torch.cuda.empty_cache()
            del model
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
