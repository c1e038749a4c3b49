#!/usr/bin/env python3
"""What param groups cost in the optimizer step: the update over the ResNet-50 arena of configs/vfs_r50.py.
  (a) sgd          the shipped config's single group: vfs_sgd_step over the trainable range;
  (b) table1       vfs_opt_step_table with ONE param group (every parameter a segment of group 0);
  (c) tableN       vfs_opt_step_table with one param group per parameter (the groups of build_optimizer with paramwise_cfg);
  (d) adamwN       AdamW, one param group per parameter;
  (e) tableN_step  (c) through SGD.step(): the same launch behind step()'s host work (one row per group, every step).
(a) - (d) call the C entry point directly with arguments prepared once, and (a), (b), (c), (e) work on the SAME momentum arena, so
that they differ in the launch alone; (e) shows what the host side of step() adds.  Only the optimizer step is timed (no forward, no backward; the gradients are a resident random
arena).  All arms work on the same arena in one process; a round takes `--steps` steps of each arm in turn, each step's C call
between two events on the launch stream (the median over the steps is the round's value), so drift of a shared machine hits all
arms alike.  Reported per arm: the median over the rounds, every round, and the spread (max - min over the rounds), and the host
time of one step() of (e).  SGD moves 20 bytes per parameter and Adam 28, so (d) is expected near 1.4 x (a), and (b), (c) are
accepted when they are no slower than (a) by more than (a)'s own spread.

Usage: python tools/bench_optim.py [--steps 20] [--warmup 5] [--repeats 9] [--out FILE.json]"""
import json
import os
import statistics
import sys

import torch

REPO = __file__.rsplit('/tools/', 1)[0]
sys.path.insert(0, REPO)
import vfs_amd  # noqa: E402
from vfs_amd.engine import shared_engine  # noqa: E402


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    steps, warmup, repeats = _arg('--steps', 20), _arg('--warmup', 5), _arg('--repeats', 9)
    dev = torch.device('cuda:0')
    cfg = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', 'vfs_r50.py'))
    torch.manual_seed(0)
    model = vfs_amd.build_model(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(dev).train()
    f = model.flatten_parameters()
    f['grads'].copy_(torch.randn(f['grads'].shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 1e-3)
    base = dict(cfg.optimizer, lr=1e-6)      # the values do not matter to the time; small steps keep the arena finite
    paramwise = dict(norm_decay_mult=0., bias_decay_mult=0., bias_lr_mult=2., custom_keys={'img_head': dict(lr_mult=10.)})
    sgd = vfs_amd.build_optimizer(model, base)
    tableN = vfs_amd.build_optimizer(model, dict(base, paramwise_cfg=paramwise))
    adamwN = vfs_amd.build_optimizer(model, dict(type='AdamW', lr=1e-6, weight_decay=1e-2, paramwise_cfg=paramwise))
    eng = shared_engine()
    n, st = f['params'].numel(), eng.stream(dev)

    # the SGD arms (a), (b), (c) and (e) all update tableN's momentum arena: where an arena lies in memory moves an arm by more
    # than the arms differ (two arenas of the same size and content, the same kernel: 137 against 154 us was measured)
    tableN._arena()
    shared = tableN._buf

    def direct(opt, kind, nbytes):
        """the table launch as opt.step() issues it, with everything prepared once"""
        opt._arena()
        nseg, dev_map, table, hyper, ntrain = opt._device_table(eng, f)
        rows, _ = opt._group_rows()
        hyper.numpy()[:, :len(rows[0])] = rows
        s1 = opt._arenas[opt._state_names[0]] if kind else shared
        s2 = opt._arenas[opt._state_names[1]] if len(opt._state_names) > 1 else None
        return lambda: eng.timed('sgd', (0.0, nbytes * ntrain), dev, eng.lib.opt_step_table, kind, f['params'], f['grads'], s1, s2, n,
                                 dev_map, nseg, hyper.data_ptr(), len(rows), table, 0, 1, None, None, st), nseg, ntrain
    sgd._arena()
    (lo, hi), = sgd._segments[1]
    lr, wd, momentum = sgd._group_values(sgd.param_groups[0])

    p_a, g_a, b_a = f['params'][lo:hi], f['grads'][lo:hi], shared[lo:hi]

    def sgd_direct():
        eng.timed('sgd', (0.0, 20.0 * (hi - lo)), dev, eng.lib.sgd_step, p_a, g_a, b_a, hi - lo, lr, momentum, wd, None, st)
    one = vfs_amd.build_optimizer(model, base)      # (b): one group, so step() itself would take the single-group launch
    table1, nseg, ntrain = direct(one, 0, 20.0)
    arms = dict(sgd=sgd_direct, table1=table1, tableN=direct(tableN, 0, 20.0)[0], adamwN=direct(adamwN, 2, 28.0)[0], tableN_step=tableN.step)

    def timed(fn):
        """median over `steps` steps of the device time of the step's launches: the engine brackets each C call (for the table
        arms whatever the call launches) with two events on the launch stream"""
        torch.cuda.synchronize()
        eng.prof = []
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        rec, eng.prof = eng.prof, None
        assert len(rec) == steps and all(r[0] == 'sgd' for r in rec), 'one update launch per step in every arm'
        return statistics.median(r[2].elapsed_time(r[3]) for r in rec) * 1e3      # us per step

    for fn in arms.values():
        for _ in range(warmup):
            fn()
    runs = {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            runs[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in runs.items()}
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(100):
        tableN.step()
    host_us = (time.perf_counter() - t0) / 100 * 1e6      # issue time of step(): above the kernel's time the device idles between steps
    torch.cuda.synchronize()
    res = dict(device=torch.cuda.get_device_name(0), steps=steps, warmup=warmup, repeats=repeats, arena_words=f['params'].numel(),
               trainable_words=ntrain, parameters=nseg, groups=dict(sgd=1, table1=1, tableN=len(tableN.param_groups), adamwN=len(adamwN.param_groups)), tableN_step_host_us=host_us,
               step_us=med, rounds_us=runs, spread_us={k: max(v) - min(v) for k, v in runs.items()},
               table1_minus_sgd_us=med['table1'] - med['sgd'], tableN_minus_sgd_us=med['tableN'] - med['sgd'], adamwN_over_sgd=med['adamwN'] / med['sgd'],
               sgd_gbytes_per_s=20.0 * ntrain / med['sgd'] / 1e3, adamwN_gbytes_per_s=28.0 * ntrain / med['adamwN'] / 1e3)
    print(json.dumps(res), flush=True)
    if '--out' in sys.argv:
        out = _arg('--out', '')
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
