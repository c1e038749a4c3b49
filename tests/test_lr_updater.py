"""vfs_amd.build_lr_updater: the config's lr_config (configs/r*_*.py:135 -> mmcv's LrUpdaterHook) on the param groups of an
optimizer.  Host code only: closed-form values, no kernel."""
import math
import os

import pytest
import torch

import vfs_amd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX = 200


class _Opt:
    """what the updater needs of an optimizer: its param groups"""

    def __init__(self, *lrs):
        self.param_groups = [dict(lr=lr) for lr in lrs]


def _cos(base, target, progress, total):
    return target + 0.5 * (base - target) * (math.cos(math.pi * progress / total) + 1)


def _lrs(opt):
    return [g['lr'] for g in opt.param_groups]


@pytest.mark.parametrize('warmup', [None, 'linear', 'constant', 'exp'])
@pytest.mark.parametrize('target', [dict(min_lr=0), dict(min_lr=0.001), dict(min_lr_ratio=0.1)])
def test_cosine_closed_form(warmup, target):
    """iterations 0, inside the warmup, mid and last, for two groups (the second the x 10 head group): each from its own initial_lr"""
    opt = _Opt(0.05, 0.5)
    cfg = dict(policy='CosineAnnealing', by_epoch=False, **target)
    if warmup:
        cfg.update(warmup=warmup, warmup_iters=20, warmup_ratio=0.25)
    up = vfs_amd.build_lr_updater(opt, cfg, MAX)
    assert [g['initial_lr'] for g in opt.param_groups] == [0.05, 0.5]
    for it in (0, 7, 19, 20, MAX // 2, MAX - 1):
        up.before_iter(it)
        for lr, base in zip(_lrs(opt), (0.05, 0.5)):
            tgt = target['min_lr'] if 'min_lr' in target else base * target['min_lr_ratio']
            want = _cos(base, tgt, it, MAX)
            if warmup and it < 20:
                want *= {'linear': 1 - (1 - it / 20) * (1 - 0.25), 'constant': 0.25, 'exp': 0.25 ** (1 - it / 20)}[warmup]
            assert lr == pytest.approx(want, rel=1e-12, abs=1e-15), (it, warmup)
    up.before_iter(0)
    assert _lrs(opt) == ([0.05, 0.5] if warmup is None else pytest.approx([0.0125, 0.125]))
    up.before_iter(MAX // 2)
    if target == dict(min_lr=0):
        assert _lrs(opt) == pytest.approx([0.025, 0.25])


def test_fixed_policy_and_warmup():
    opt = _Opt(0.05, 0.5)
    up = vfs_amd.build_lr_updater(opt, dict(policy='fixed', warmup='linear', warmup_iters=10, warmup_ratio=0.5), MAX)
    up.before_iter(0)
    assert _lrs(opt) == pytest.approx([0.025, 0.25])
    up.before_iter(5)
    assert _lrs(opt) == pytest.approx([0.0375, 0.375])
    for it in (10, 150):
        up.before_iter(it)
        assert _lrs(opt) == [0.05, 0.5]


def test_by_epoch_steps_once_per_epoch():
    opt = _Opt(0.05)
    up = vfs_amd.build_lr_updater(opt, dict(policy='CosineAnnealing', min_lr=0, by_epoch=True), max_iters=100, iters_per_epoch=10)
    seen = []
    for it in range(100):
        up.before_iter(it)
        seen.append(opt.param_groups[0]['lr'])
    for epoch in range(10):
        assert set(seen[10 * epoch:10 * epoch + 10]) == {seen[10 * epoch]}
        assert seen[10 * epoch] == pytest.approx(_cos(0.05, 0.0, epoch, 10))
    assert len(set(seen)) == 10
    with pytest.raises(ValueError, match='iters_per_epoch'):
        vfs_amd.build_lr_updater(opt, dict(policy='CosineAnnealing', min_lr=0, by_epoch=True), max_iters=100)


def test_initial_lr_comes_from_a_resumed_state():
    """a resumed state_dict's groups carry initial_lr (and the decayed lr): the schedule goes on from the initial one"""
    opt = _Opt(0.0123)
    opt.param_groups[0]['initial_lr'] = 0.05
    up = vfs_amd.build_lr_updater(opt, dict(policy='CosineAnnealing', min_lr=0, by_epoch=False), MAX)
    up.before_iter(MAX // 2)
    assert opt.param_groups[0]['lr'] == pytest.approx(0.025) and opt.param_groups[0]['initial_lr'] == 0.05
    q = torch.zeros(3, requires_grad=True)      # through a real optimizer's state_dict
    a = torch.optim.SGD([q], lr=0.05)
    vfs_amd.build_lr_updater(a, dict(policy='CosineAnnealing', min_lr=0, by_epoch=False), MAX).before_iter(150)
    b = torch.optim.SGD([q], lr=1.0)
    b.load_state_dict(a.state_dict())
    up = vfs_amd.build_lr_updater(b, dict(policy='CosineAnnealing', min_lr=0, by_epoch=False), MAX)
    up.before_iter(0)
    assert b.param_groups[0]['lr'] == 0.05


@pytest.mark.parametrize('depth', [18, 50])
def test_shipped_lr_config_builds(depth):
    cfg = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', f'vfs_r{depth}.py'))
    opt = _Opt(cfg.optimizer['lr'])
    up = vfs_amd.build_lr_updater(opt, cfg.lr_config, max_iters=1000)
    assert isinstance(up, vfs_amd.LrUpdater) and up.policy == 'CosineAnnealing' and not up.by_epoch
    up.before_iter(999)
    assert 0 < opt.param_groups[0]['lr'] < 1e-6
    assert dict(cfg.lr_config) == dict(policy='CosineAnnealing', min_lr=0, by_epoch=False)      # build_lr_updater leaves the config alone


def test_refusals():
    opt = _Opt(0.05)
    with pytest.raises(NotImplementedError, match='step'):
        vfs_amd.build_lr_updater(opt, dict(policy='step', step=[30, 60]), MAX)
    with pytest.raises(NotImplementedError, match='Cyclic'):
        vfs_amd.build_lr_updater(opt, dict(policy='Cyclic'), MAX)
    with pytest.raises(NotImplementedError, match='warmup_by_epoch'):
        vfs_amd.build_lr_updater(opt, dict(policy='fixed', warmup_by_epoch=True), MAX)
    with pytest.raises(ValueError):
        vfs_amd.build_lr_updater(opt, dict(policy='CosineAnnealing', by_epoch=False), MAX)
    with pytest.raises(ValueError):
        vfs_amd.build_lr_updater(opt, dict(policy='CosineAnnealing', min_lr=0, min_lr_ratio=0.1, by_epoch=False), MAX)
    with pytest.raises(ValueError):
        vfs_amd.build_lr_updater(opt, dict(policy='fixed', warmup='cosine', warmup_iters=5), MAX)
    with pytest.raises(ValueError):
        vfs_amd.build_lr_updater(opt, dict(policy='fixed', warmup='linear'), MAX)
    with pytest.raises(KeyError):
        vfs_amd.build_lr_updater(opt, dict(by_epoch=False), MAX)
