"""Times of the dilated-convolution backward (csrc/conv_dilated.hip) at the SiamFC probe's layer shapes, next to the same
shapes with dilation 1 through the tuned undilated kernels - same FLOP, same bytes: the yardstick - and the probe's train step
with the backbone frozen against frozen_stages=2.  Prints a table and one JSON line; asserts no time.

    python tools/bench_dilated_bwd.py [--batch 8] [--repeats 20] [--no-step] [--out FILE.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vfs_amd._lib import get_lib                                    # noqa: E402
from vfs_amd.packing import wgrad_halo_eligible, wgrad_splits       # noqa: E402

BF16 = torch.bfloat16
# (name, channels of the 3x3 conv - or (Cin, Cout) -, dilation): the dilated 3x3 convs of the probe's backbone (dilations=(1, 1, 2, 4); the first
# block of a dilated stage runs at dilation / 2), ResNet-18 BasicBlock conv1 and ResNet-50 Bottleneck conv2
LAYERS = [('r18.layer3.1.conv1', 256, 2), ('r18.layer4.0.conv1', (256, 512), 2), ('r18.layer4.1.conv1', 512, 4),
          ('r50.layer3.1.conv2', 256, 2), ('r50.layer4.0.conv2', 512, 2), ('r50.layer4.1.conv2', 512, 4)]
MAPS = [32, 15]      # 255 / 120 pixel crops at stride 8


def timed(fn, repeats, flush):
    """median time of fn in microseconds, the L2 flushed before every launch"""
    e0 = [torch.cuda.Event(enable_timing=True) for _ in range(repeats)]
    e1 = [torch.cuda.Event(enable_timing=True) for _ in range(repeats)]
    for _ in range(3):
        fn()
    for i in range(repeats):
        flush.add_(1.0)
        e0[i].record()
        fn()
        e1[i].record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in zip(e0, e1))
    return ts[len(ts) // 2]


def bench_layer(lib, name, ch, dil, N, hw, repeats, flush):
    cin, cout = ch if isinstance(ch, tuple) else (ch, ch)
    dev = torch.device('cuda:0')
    H = W = hw
    M = N * H * W
    g = torch.Generator(device='cpu').manual_seed(hw + dil)
    x = torch.randn(N, H, W, cin, generator=g).to(dev, BF16)
    dy = torch.randn(N, H, W, cout, generator=g).to(dev, BF16)
    wd = (torch.randn(cin, 3, 3, cout, generator=g) * 0.02).to(dev, BF16)
    dx = torch.empty(N, H, W, cin, dtype=BF16, device=dev)
    add = torch.randn(N, H, W, cin, generator=g).to(dev, BF16)
    grad = torch.zeros(cout, cin, 3, 3, device=dev)
    ktot = 9 * cin
    halo = (N, H, W, cin) if wgrad_halo_eligible(N, H, W, cin, cout, 3, 1, 1, lib=lib) else None
    ns1, pps1 = wgrad_splits(M, cout, ktot, halo_geom=halo, lib=lib)
    nsd, ppsd = wgrad_splits(M, cout, ktot, lib=lib)
    partial = torch.empty(max(ns1, nsd) * cout * ktot, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    row = dict(layer=name, map=hw, N=N, cin=cin, cout=cout, dilation=dil, gflop=2e-9 * M * cout * ktot)
    row['dgrad_dilated_us'] = timed(lambda: lib.conv_dgrad_dilated(dy, wd, dx, add, None, N, H, W, cin, H, W, cout, 3, 3, 1, dil, dil, s), repeats, flush)
    row['dgrad_undilated_us'] = timed(lambda: lib.conv_dgrad(dy, wd, dx, add, N, H, W, cin, H, W, cout, 3, 3, 1, 1, s), repeats, flush)
    row['wgrad_dilated_us'] = timed(lambda: lib.conv_wgrad_dilated(dy, x, partial, grad, N, H, W, cin, H, W, cout, 3, 3, 1, dil, dil, nsd, ppsd, s), repeats, flush)
    row['wgrad_undilated_us'] = timed(lambda: lib.conv_wgrad(dy, x, partial, grad, N, H, W, cin, H, W, cout, 3, 3, 1, 1, ns1, pps1, s), repeats, flush)
    row['dgrad_ratio'] = row['dgrad_dilated_us'] / row['dgrad_undilated_us']
    row['wgrad_ratio'] = row['wgrad_dilated_us'] / row['wgrad_undilated_us']
    return row


def bench_step(depth, frozen_stages, batch, repeats):
    """median milliseconds of SiamFCProbe.train_step (host + device, synchronised)"""
    import time
    import vfs_amd
    from vfs_amd.siamfc import DEFAULT_CFG
    cfg = dict(out_channels=512 if depth == 18 else 2048, batch_size=batch, backbone=dict(DEFAULT_CFG['backbone'], frozen_stages=frozen_stages))
    probe = vfs_amd.SiamFCProbe(cfg, depth=depth, device='cuda:0')
    g = torch.Generator().manual_seed(0)
    z = (torch.rand(batch, 3, 120, 120, generator=g) * 255).cuda()
    x = (torch.rand(batch, 3, 255, 255, generator=g) * 255).cuda()
    ts = []
    for i in range(repeats + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        probe.train_step((z, x))
        torch.cuda.synchronize()
        if i >= 3:
            ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out')
    a = ap.parse_args()
    lib = get_lib()
    flush = torch.zeros(96 << 20, device='cuda:0')      # 384 MB: larger than the L2 + MALL
    rows = [bench_layer(lib, n, ch, d, a.batch, hw, a.repeats, flush) for hw in MAPS for n, ch, d in LAYERS]
    print(f'{"layer":22s} {"map":>4s} {"dil":>3s} {"GFLOP":>7s} | {"dgrad dil":>9s} {"dgrad d=1":>9s} {"ratio":>5s} | {"wgrad dil":>9s} {"wgrad d=1":>9s} {"ratio":>5s}   (us)')
    for r in rows:
        print(f'{r["layer"]:22s} {r["map"]:4d} {r["dilation"]:3d} {r["gflop"]:7.2f} | {r["dgrad_dilated_us"]:9.1f} {r["dgrad_undilated_us"]:9.1f} '
              f'{r["dgrad_ratio"]:5.2f} | {r["wgrad_dilated_us"]:9.1f} {r["wgrad_undilated_us"]:9.1f} {r["wgrad_ratio"]:5.2f}')
    res = dict(layers=rows)
    if not a.no_step:
        del flush
        res['step_ms'] = {f'r18_frozen{fs}': bench_step(18, fs, a.batch, max(5, a.repeats // 2)) for fs in (4, 2)}
        print('train step (ms):', res['step_ms'])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
