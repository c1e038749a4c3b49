"""Label propagation over several backbone stages: one multi-stage run against one run per stage, and the two-pass kernels of the
narrow levels (C = 64 / 128) against the dense kernel.

Synthetic DAVIS-size clips (480 x 854, 3-D label maps), ResNet-18 and ResNet-50, the shipped test-time test_cfg of the depth, fp32:
  stages   out_indices = (0, 1, 2, 3) in ONE forward_test (one backbone pass per chunk of frames) against the SUM of four
           forward_test runs with out_indices = (s,) - what the single-level code path needs for the same label maps (four passes);
  narrow   ResNet-18 only: out_indices = (0,) (64 channels, 120 x 214 features) and (1,) (128 channels, 60 x 107) with
           test_cfg.lp2_narrow on (two-pass kernels) and off (dense kernel), and whether the label maps are equal.
Arms alternate inside every repeat on one box; the median over the repeats and the spread (min .. max) are reported per frame.

  python tools/bench_labelprop_stages.py [--depth 18 50] [--part stages narrow] [--frames 10] [--repeats 5] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZE = (480, 854)


def make_clip(T, dev, seed=0):
    H, W = SIZE
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(1, 1, 3, 1, H, W, generator=g)
    imgs = (base + 0.3 * torch.randn(1, 1, 3, T, H, W, generator=g)).to(dev)
    lab = torch.zeros(H, W, dtype=torch.uint8)
    for c in range(1, 4):
        lab[40 * c:40 * c + 160, 90 * c:90 * c + 220] = c
    return imgs, lab[None], [dict(original_shape=(H, W, 3))]


def make_model(depth, dev):
    import vfs_amd
    cfg = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', f'vfs_r{depth}.py'))
    tc = vfs_amd.ConfigDict(cfg.test_cfg)
    tc['precision'] = 'fp32'
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


def run(model, clip, stages, narrow=None):
    """forward_test with the listed stages (as tools/test.py of the reference sets them: config and backbone)"""
    model.test_cfg['out_indices'] = model.backbone.out_indices = tuple(stages)
    if narrow is None:
        model.test_cfg.pop('lp2_narrow', None)
    else:
        model.test_cfg['lp2_narrow'] = narrow
    imgs, ref, meta = clip
    return model(imgs, return_loss=False, ref_seg_map=ref, img_meta=meta)[0]


def measure(arms, repeats, frames):
    """arms: [(name, fn)] -> {name: (median, min, max) ms per frame}; the arms alternate inside every repeat"""
    for _, fn in arms:
        fn()      # warm-up: buffers, workspaces
    times = {name: [] for name, _ in arms}
    for _ in range(repeats):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    out = {}
    for name, ts in times.items():
        ts = sorted(ts)
        out[name] = tuple(round(1e3 * v / frames, 4) for v in (ts[len(ts) // 2], ts[0], ts[-1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, nargs='+', default=[18, 50], choices=[18, 50])
    ap.add_argument('--part', nargs='+', default=['stages', 'narrow'], choices=['stages', 'narrow'])
    ap.add_argument('--frames', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = torch.device('cuda:0')
    clip = make_clip(args.frames, dev)
    results = []

    def report(**row):
        results.append(row)
        print(json.dumps(row), flush=True)
    for depth in args.depth:
        model = make_model(depth, dev)
        if 'stages' in args.part:
            multi = run(model, clip, (0, 1, 2, 3))
            equal = all(np.array_equal(multi[s], run(model, clip, (s,))) for s in range(4))
            res = measure([('one run, out_indices=(0,1,2,3)', lambda: run(model, clip, (0, 1, 2, 3))),
                           ('four runs, out_indices=(s,)', lambda: [run(model, clip, (s,)) for s in range(4)])], args.repeats, args.frames)
            for arm, (med, lo, hi) in res.items():
                report(part='stages', depth=depth, arm=arm, frames=args.frames, size=list(SIZE), ms_per_frame=med, ms_per_frame_min=lo,
                       ms_per_frame_max=hi, repeats=args.repeats, levels_equal_single_stage_runs=equal)
        if 'narrow' in args.part and depth == 18:
            for stage, C in ((0, 64), (1, 128)):
                equal = np.array_equal(run(model, clip, (stage,), True), run(model, clip, (stage,), False))
                res = measure([('two-pass', lambda: run(model, clip, (stage,), True)), ('dense', lambda: run(model, clip, (stage,), False))],
                              args.repeats, args.frames)
                for arm, (med, lo, hi) in res.items():
                    report(part='narrow', depth=depth, stage=stage, channels=C, arm=arm, frames=args.frames, size=list(SIZE), ms_per_frame=med,
                           ms_per_frame_min=lo, ms_per_frame_max=hi, repeats=args.repeats, two_pass_equals_dense=equal)
        del model
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
