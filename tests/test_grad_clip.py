"""Gradient clipping on the flat arena (optimizer_config = dict(grad_clip=...), configs/r*_*.py:136 -> mmcv OptimizerHook.clip_grads
-> torch.nn.utils.clip_grad_norm_): the norm reduction and its finish, the clipped SGD step, the in-place scale by a device scalar,
their argument checks, and the whole thing through vfs_amd.build_optimizer / SGD.step / vfs_amd.clip_grad_norm_.
backend=emu: CPU fiber emulator; backend=gpu: libvfs_hip.so on the MI355X."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import vfs_oracle as O
from tests.grad_clip_worker import shallow_r18

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, 'tests', 'grad_clip_worker.py')
LR, MOM, WD = 0.05, 0.9, 1e-4      # configs/vfs_r18.py optimizer


def _within_1ulp(x, ref):
    """x (an fp32 value) against float32(ref), ref in fp64"""
    r = np.float32(ref)
    return abs(float(np.float32(x)) - float(r)) <= float(np.spacing(np.abs(r)))


def _rows(lib):
    n = torch.zeros(1, dtype=torch.int32)
    lib.grad_norm_rows(n)
    return int(n)


def _norm(backend, segments, norm_type, max_norm):
    """reduction over the segments (the first overwrites the rows, the others accumulate) + finish -> float32 [norm, coefficient]"""
    rows = torch.full((_rows(backend.lib),), 7.0, dtype=torch.float64)      # stale values: the first launch must overwrite them
    out = torch.zeros(2)
    for i, g in enumerate(segments):
        backend.hostlib.grad_norm_partial(g, g.numel(), norm_type, rows, int(i > 0), None)
    backend.hostlib.grad_norm_finish(rows, norm_type, max_norm, out, None)
    return out.numpy().copy()


def _values(n, kind, seed=0):
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed + n)) * 1e-3
    if kind == 'spike':      # one large element: an fp32 accumulator would lose the small squares next to 1e8
        g[n // 2] = 1e4
    return g


def _ref_l2(*segments):
    return float(np.sqrt(sum(float((s.double().numpy() ** 2).sum()) for s in segments)))


# ---------------------------------------------------------------------------------------------- 1. the reduction
@pytest.mark.parametrize('kind', ['small', 'spike'])
@pytest.mark.parametrize('n', [1, 3, 4, 255, 1027, 'pass+5'])
def test_l2_norm_and_coefficient_against_fp64(backend, n, kind):
    """out[0] and out[1] within 1 fp32 ulp of the fp64 reference (the double sum differs from numpy's by at most n 2^-53 relative,
    so only the final rounding to fp32 can differ), and the same bits on a second run.  'pass+5': five words more than one pass
    of the grid covers (rows x 256 lanes x 4 words), so the stride loop runs a second time and the scalar tail is used"""
    if n == 'pass+5':
        n = _rows(backend.lib) * 1024 + 5
    g = _values(n, kind)
    ref = _ref_l2(g)
    max_norm = 0.5 * ref
    got = _norm(backend, [g], 2.0, max_norm)
    print(n, kind, got, ref, max_norm / (ref + 1e-6))
    assert _within_1ulp(got[0], ref)
    assert _within_1ulp(got[1], min(1.0, max_norm / (ref + 1e-6)))
    again = _norm(backend, [g], 2.0, max_norm)
    assert got.tobytes() == again.tobytes()


@pytest.mark.parametrize('kind', ['small', 'spike'])
def test_two_segments_accumulate_into_the_same_rows(backend, kind):
    a, b = _values(1027, kind), _values(515, kind, seed=1)
    ref = _ref_l2(a, b)
    got = _norm(backend, [a, b], 2.0, 0.25 * ref)
    assert _within_1ulp(got[0], ref)
    assert _within_1ulp(got[1], min(1.0, 0.25 * ref / (ref + 1e-6)))
    assert got.tobytes() == _norm(backend, [a, b], 2.0, 0.25 * ref).tobytes()
    inf = _norm(backend, [a, b], math.inf, 1.0)
    assert float(inf[0]) == max(float(a.abs().max()), float(b.abs().max()))


@pytest.mark.parametrize('n', [1, 3, 4, 255, 1027, 'pass+5'])
def test_infinity_norm_is_exact(backend, n):
    if n == 'pass+5':
        n = _rows(backend.lib) * 1024 + 5
    g = _values(n, 'small')
    g[n - 1] = -0.5      # the maximum in the last word (the scalar tail when n % 4 != 0), negative
    ref = float(g.abs().max())
    got = _norm(backend, [g], math.inf, 0.125)
    assert float(got[0]) == ref == 0.5
    assert _within_1ulp(got[1], 0.125 / (ref + 1e-6))
    g[n - 1] = 1e-9
    assert float(_norm(backend, [g], math.inf, 0.125)[0]) == float(g.abs().max())


@pytest.mark.parametrize('norm_type', [2.0, math.inf])
@pytest.mark.parametrize('n,at', [(1, 0), (1027, 1026), (1027, 0), (5000, 2049)])
def test_nan_gives_nan_norm_and_coefficient(backend, norm_type, n, at):
    g = _values(n, 'small')
    g[at] = float('nan')
    got = _norm(backend, [g], norm_type, 1.0)
    assert np.isnan(got[0]) and np.isnan(got[1])
    clean = _values(515, 'small')      # a NaN in either segment survives the accumulation
    for segs in ([g, clean], [clean, g]):
        got = _norm(backend, segs, norm_type, 1.0)
        assert np.isnan(got[0]) and np.isnan(got[1])


# ---------------------------------------------------------------------------------------------- 2. the clipped step
def _sgd_inputs(n, seed=5):
    gen = torch.Generator().manual_seed(seed + n)
    return (torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1, torch.randn(n, generator=gen) * 0.1)


@pytest.mark.parametrize('n', [1, 5, 1027, 70001])
def test_clipped_step_below_max_norm_equals_unclipped_bits(backend, n):
    p, g, buf = _sgd_inputs(n)
    out = torch.from_numpy(_norm(backend, [g], 2.0, 2.0 * _ref_l2(g)))
    assert float(out[1]) == 1.0
    p0, b0 = p.clone(), buf.clone()
    backend.hostlib.sgd_step(p0, g, b0, n, LR, MOM, WD, None, None)
    g_before = g.clone()
    backend.hostlib.sgd_step_clip(p, g, buf, n, LR, MOM, WD, out[1:2], None, None)
    assert torch.equal(p, p0) and torch.equal(buf, b0)
    assert torch.equal(g, g_before)


@pytest.mark.parametrize('n', [1, 5, 1027, 70001])
def test_clipped_step_above_max_norm_against_fp64(backend, n):
    """p, buf against an fp64 evaluation that uses the kernel's own fp32 coefficient c: every element within
    8 x 2^-24 x (|p| + lr (|m buf| + |g c| + |wd p|)) - a few fp32 roundings per element, with or without contraction;
    c itself within 1 ulp of the fp64 coefficient"""
    p, g, buf = _sgd_inputs(n)
    ref_norm = _ref_l2(g)
    max_norm = 0.3 * ref_norm
    out = torch.from_numpy(_norm(backend, [g], 2.0, max_norm))
    assert _within_1ulp(out[1], max_norm / (ref_norm + 1e-6)) and float(out[1]) < 0.31
    c = float(out[1])
    pd, gd, bd = p.double(), g.double(), buf.double()
    lr, mom, wd = float(np.float32(LR)), float(np.float32(MOM)), float(np.float32(WD))      # the scalars as the kernel receives them
    b_ref = mom * bd + (gd * c + wd * pd)
    p_ref = pd - lr * b_ref
    mag = (mom * bd).abs() + (gd * c).abs() + (wd * pd).abs()
    g_before = g.clone()
    backend.hostlib.sgd_step_clip(p, g, buf, n, LR, MOM, WD, out[1:2], None, None)
    eb, ep = (buf.double() - b_ref).abs(), (p.double() - p_ref).abs()
    print(n, 'worst / bound', float((eb / (8 * 2.0 ** -24 * mag)).max()), float((ep / (8 * 2.0 ** -24 * (pd.abs() + lr * mag))).max()))
    assert bool((eb <= 8 * 2.0 ** -24 * mag).all())
    assert bool((ep <= 8 * 2.0 ** -24 * (pd.abs() + lr * mag)).all())
    assert torch.equal(g, g_before)


def test_skip_flag_leaves_the_clipped_step_untouched(backend):
    n = 1027
    p, g, buf = _sgd_inputs(n)
    clip = torch.tensor([0.5])
    p0, g0, b0 = p.clone(), g.clone(), buf.clone()
    backend.hostlib.sgd_step_clip(p, g, buf, n, LR, MOM, WD, clip, torch.ones(1, dtype=torch.int64), None)
    assert torch.equal(p, p0) and torch.equal(buf, b0) and torch.equal(g, g0)
    backend.hostlib.sgd_step_clip(p, g, buf, n, LR, MOM, WD, clip, torch.zeros(1, dtype=torch.int64), None)
    assert not torch.equal(p, p0) and not torch.equal(buf, b0) and torch.equal(g, g0)


@pytest.mark.parametrize('n', [1, 3, 1027, 70001])
def test_scale_by_equals_scale(backend, n):
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    a, b = x.clone(), x.clone()
    coef = torch.tensor([0.3337], dtype=torch.float32)
    backend.hostlib.scale(a, n, float(coef[0]), None)
    backend.hostlib.scale_by(b, n, coef, None)
    assert torch.equal(a, b) and not torch.equal(a, x)


# ---------------------------------------------------------------------------------------------- 3. argument errors
def _error_cases():
    P = torch.zeros(64)
    ARG = -3
    inf = math.inf
    return [
        ('grad_norm_rows', (None,), ARG, 'grad_norm_rows: bad argument'),
        ('grad_norm_partial', (None, 4, 2.0, P, 0, None), ARG, 'grad_norm_partial: null buffer'),
        ('grad_norm_partial', (P, 4, 2.0, None, 0, None), ARG, 'grad_norm_partial: null buffer'),
        ('grad_norm_partial', (P, -1, 2.0, P, 0, None), ARG, 'grad_norm_partial: n < 0'),
        ('grad_norm_partial', (P[1:], 4, 2.0, P, 0, None), ARG, 'grad_norm_partial: 16-byte aligned gradients'),
        ('grad_norm_partial', (P, 4, 3.0, P, 0, None), ARG, 'grad_norm_partial: norm_type must be 2 or infinity'),
        ('grad_norm_partial', (P, 4, 1.0, P, 0, None), ARG, 'grad_norm_partial: norm_type must be 2 or infinity'),
        ('grad_norm_partial', (P, 4, -inf, P, 0, None), ARG, 'grad_norm_partial: norm_type must be 2 or infinity'),
        ('grad_norm_finish', (None, 2.0, 1.0, P, None), ARG, 'grad_norm_finish: null buffer'),
        ('grad_norm_finish', (P, 2.0, 1.0, None, None), ARG, 'grad_norm_finish: null buffer'),
        ('grad_norm_finish', (P, 0.0, 1.0, P, None), ARG, 'grad_norm_finish: norm_type must be 2 or infinity'),
        ('grad_norm_finish', (P, float('nan'), 1.0, P, None), ARG, 'grad_norm_finish: norm_type must be 2 or infinity'),
        ('grad_norm_finish', (P, 2.0, 0.0, P, None), ARG, 'grad_norm_finish: max_norm <= 0'),
        ('grad_norm_finish', (P, inf, -1.0, P, None), ARG, 'grad_norm_finish: max_norm <= 0'),
        ('sgd_step_clip', (None, P, P, 4, LR, MOM, WD, P, None, None), ARG, 'sgd_step_clip: null buffer'),
        ('sgd_step_clip', (P, None, P, 4, LR, MOM, WD, P, None, None), ARG, 'sgd_step_clip: null buffer'),
        ('sgd_step_clip', (P, P, None, 4, LR, MOM, WD, P, None, None), ARG, 'sgd_step_clip: null buffer'),
        ('sgd_step_clip', (P, P, P, 4, LR, MOM, WD, None, None, None), ARG, 'sgd_step_clip: null buffer'),
        ('sgd_step_clip', (P, P, P, -4, LR, MOM, WD, P, None, None), ARG, 'sgd_step_clip: n < 0'),
        ('scale_by', (None, 4, P, None), ARG, 'scale_by: null buffer'),
        ('scale_by', (P, 4, None, None), ARG, 'scale_by: null buffer'),
        ('scale_by', (P, -1, P, None), ARG, 'scale_by: n < 0'),
        ('scale_by', (P[1:], 4, P, None), ARG, 'scale_by: 16-byte aligned buffer'),
    ]


@pytest.mark.parametrize('name,args,code,message', _error_cases())
def test_argument_errors(name, args, code, message):
    """each bad argument returns its code before anything is launched; the message names the entry point"""
    from tests.emu_util import emu_lib
    lib = emu_lib()
    fn = lib.cfunc(name)
    assert len(args) == len(lib.protos['vfs_' + name][1]), 'the case does not match the prototype'
    rc = fn(*[a.data_ptr() if hasattr(a, 'data_ptr') else a for a in args])
    assert (rc, lib.last_error()) == (code, message)
    assert message.startswith(name + ':')


# ---------------------------------------------------------------------------------------------- 4. the public interface
SHAPE = [4, 2, 3, 1, 32, 32]


def _sync(dev):
    if dev.type == 'cuda':
        torch.cuda.synchronize()


def _forward_backward(model, opt, imgs):
    out = model.train_step(dict(imgs=imgs, label=torch.zeros(imgs.shape[0], 1)), opt)
    opt.zero_grad()
    out['loss'].backward()
    return out


def _grad_norm64(model, norm_type=2.0):
    gs = [p.grad.detach().cpu().double().reshape(-1) for p in model.parameters() if p.requires_grad]
    allg = torch.cat(gs)
    return float(allg.abs().max()) if norm_type == math.inf else float(allg.pow(2).sum().sqrt())


def _snapshot(model):
    return {n: p.detach().cpu().clone() for n, p in model.named_parameters()}


def _torch_clipped_step(before, grads, trainable, max_norm, norm_type=2.0):
    """what the reference does on the CPU: clip_grad_norm_ on fp32 copies of the gradients, then the oracle's SGD step"""
    names = [n for n in before if trainable[n]]
    params = [before[n].clone().requires_grad_(True) for n in names]
    for q, n in zip(params, names):
        q.grad = grads[n].clone()
    total = torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=norm_type)
    with torch.no_grad():
        O.sgd_step(params, [q.grad for q in params], [None] * len(params), lr=LR, momentum=MOM, weight_decay=WD)
    return dict(zip(names, [q.detach() for q in params])), float(total), {n: q.grad for q, n in zip(params, names)}


def _assert_params_match(model, want, before, clipped_grads):
    """the per-element bar of the clipped-step test: 8 x 2^-24 x (|p| + lr (|g c| + |wd p|)); no momentum yet on a first step"""
    worst = 0.0
    for n, p in model.named_parameters():
        if n not in want:
            assert torch.equal(p.detach().cpu(), before[n]), f'{n} is frozen but was updated'
            continue
        p0, gc = before[n].double(), clipped_grads[n].double()
        bound = 8 * 2.0 ** -24 * (p0.abs() + LR * (gc.abs() + (WD * p0).abs()))
        err = (p.detach().cpu().double() - want[n].double()).abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (n, float((err / bound.clamp_min(1e-300)).max()))
    print('worst error / bound', worst)


@pytest.mark.parametrize('extra,norm_type', [(dict(), 2), (dict(frozen_stages=1), 2), (dict(), 'inf'), (dict(), math.inf)])
def test_clipped_train_step_matches_torch(backend, extra, norm_type):
    """one step with grad_clip through build_optimizer: parameters equal an identical model stepped by torch on the CPU
    (clip_grad_norm_ over the trainable parameters, then SGD), last_grad_norm() is the fp64 norm of the step's gradients, and with
    a max_norm the norm stays under the result is the unconfigured optimizer's, bit for bit"""
    dev = backend.dev
    imgs = O.fill_tensor(SHAPE, seed=11, scale=2.0).to(dev)
    nt = math.inf if norm_type in ('inf', math.inf) else 2.0
    # an unclipped step: its gradients, their norm N, and the parameters it ends with
    model, opt, _ = shallow_r18(dev, **extra)
    before = _snapshot(model)
    trainable = {n: p.requires_grad for n, p in model.named_parameters()}
    assert all(trainable.values()) != bool(extra)
    _forward_backward(model, opt, imgs)
    grads = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
    N = _grad_norm64(model, nt)
    assert N > 0
    f = model._ensure_arena()
    pad = torch.ones_like(f['grads'], dtype=torch.bool)
    for p, o in zip(f['plist'], f['offsets']):
        pad[o:o + p.numel()] = False
    assert float(f['grads'][pad].abs().sum()) == 0.0, 'the padding words of the gradient arena are not zero'
    assert opt.last_grad_norm() is None
    opt.step()
    _sync(dev)
    unclipped = _snapshot(model)

    # clipping certainly active
    model, opt, _ = shallow_r18(dev, dict(grad_clip=dict(max_norm=0.5 * N, norm_type=norm_type)), **extra)
    _forward_backward(model, opt, imgs)
    for n, p in model.named_parameters():
        assert torch.equal(p.grad.detach().cpu(), grads[n]), n      # same model, same input: same gradients
    opt.step()
    for n, p in model.named_parameters():
        assert torch.equal(p.grad.detach().cpu(), grads[n]), f'{n}: step() changed the stored gradient'
    want, total, clipped = _torch_clipped_step(before, grads, trainable, 0.5 * N, nt)
    assert abs(total - N) <= 1e-5 * N
    _assert_params_match(model, want, before, clipped)
    assert _within_1ulp(opt.last_grad_norm(), N)
    assert any(not torch.equal(p.detach().cpu(), unclipped[n]) for n, p in model.named_parameters())

    # never active: the bits of the optimizer built without optimizer_config
    model, opt, _ = shallow_r18(dev, dict(grad_clip=dict(max_norm=2.0 * N, norm_type=norm_type)), **extra)
    _forward_backward(model, opt, imgs)
    opt.step()
    _sync(dev)
    for n, p in model.named_parameters():
        assert torch.equal(p.detach().cpu(), unclipped[n]), n
    assert _within_1ulp(opt.last_grad_norm(), N)


def _assert_fp64_update(model, before, grads, bufs, c, tag=None):
    """trainable parameters against the fp64 update with the fp64 coefficient c.  The bar of the clipped-step test, 8 x 2^-24 x
    (|p| + lr (|m buf| + |g c| + |wd p|)), plus 2 x 2^-24 x lr |g c|: there the kernel's own fp32 coefficient is used, here it is
    within 1 ulp (at most 2^-23 relative) of c.  Frozen parameters must not move."""
    lr, mom, wd = float(np.float32(LR)), float(np.float32(MOM)), float(np.float32(WD))
    for n, p in model.named_parameters():
        if not p.requires_grad:
            assert torch.equal(p.detach().cpu(), before[n]), f'{n} is frozen but was updated'
            continue
        p0, g, b = before[n].double(), grads[n].double(), bufs[n].double()
        mag = (mom * b).abs() + (g * c).abs() + (wd * p0).abs()
        ref = p0 - lr * (mom * b + g * c + wd * p0)
        bound = 2.0 ** -24 * (8 * (p0.abs() + lr * mag) + 2 * lr * (g * c).abs())
        assert bool(((p.detach().cpu().double() - ref).abs() <= bound).all()), (tag, n)


def test_grad_norm_follows_each_replayed_step(backend, monkeypatch):
    """five steps on different inputs, the later ones from the recorded chains: last_grad_norm() is the norm of THAT step's
    gradients, and the update uses THAT step's coefficient (a host value baked into a recording would repeat an earlier one)"""
    monkeypatch.setenv('VFS_TAPE', '1')
    monkeypatch.setenv('VFS_GRAPHS', '0')
    dev = backend.dev
    model, opt, _ = shallow_r18(dev, dict(grad_clip=dict(max_norm=0.05)))
    seen = []
    for step in range(5):
        imgs = O.fill_tensor(SHAPE, seed=20 + step, scale=1.0 + 0.5 * step).to(dev)
        _forward_backward(model, opt, imgs)
        N = _grad_norm64(model)
        before = _snapshot(model)
        grads = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
        bufs = {n: opt.state[p]['momentum_buffer'].detach().cpu().clone() if step else torch.zeros_like(before[n])
                for n, p in model.named_parameters()}
        opt.step()
        assert _within_1ulp(opt.last_grad_norm(), N), (step, opt.last_grad_norm(), N)
        assert N > 0.05, 'the case must clip'
        _assert_fp64_update(model, before, grads, bufs, 0.05 / (N + 1e-6), step)
        seen.append(N)
    assert model._gs.fwd is not None and model._gs.bwd is not None, 'the later steps did not run from recorded chains'
    assert len(set(seen)) == 5


def test_unknown_options_are_refused(emu_backend):
    model, _, cfg = shallow_r18(emu_backend.dev)
    import vfs_amd
    with pytest.raises(NotImplementedError, match='3'):
        vfs_amd.build_optimizer(model, cfg.optimizer, optimizer_config=dict(grad_clip=dict(max_norm=1.0, norm_type=3)))
    with pytest.raises(NotImplementedError, match='clip_value'):
        vfs_amd.build_optimizer(model, cfg.optimizer, optimizer_config=dict(grad_clip=dict(max_norm=1.0, clip_value=0.1)))
    with pytest.raises(NotImplementedError, match='detect_anomalous_params'):
        vfs_amd.build_optimizer(model, cfg.optimizer, optimizer_config=dict(grad_clip=None, detect_anomalous_params=True))
    with pytest.raises(NotImplementedError, match='1'):
        vfs_amd.clip_grad_norm_(model, 1.0, norm_type=1)
    for oc in (None, dict(), dict(grad_clip=None)):
        assert vfs_amd.build_optimizer(model, cfg.optimizer, optimizer_config=oc).grad_clip is None


def _fake_grads(model, seed, dev):
    f = model._ensure_arena()
    g = torch.zeros_like(f['grads'], device='cpu')
    gen = torch.Generator().manual_seed(seed)
    for p, o in zip(f['plist'], f['offsets']):      # every parameter, frozen ones too; the padding words stay zero
        g[o:o + p.numel()] = torch.randn(p.numel(), generator=gen) * 0.01
    f['grads'].copy_(g.to(dev))


def _freeze_layer1(model):
    """frozen parameters in the MIDDLE of the arena: the trainable ones form two ranges"""
    for n, p in model.named_parameters():
        if n.startswith('backbone.layer1.'):
            p.requires_grad = False


@pytest.mark.parametrize('norm_type', [2.0, math.inf])
def test_eager_clip_grad_norm_scales_trainable_gradients_in_place(backend, norm_type):
    """vfs_amd.clip_grad_norm_(model, ...) against torch's over the requires_grad parameters, with two trainable ranges and
    non-zero gradients on the frozen parameters in between (they must neither count nor change)"""
    import vfs_amd
    dev = backend.dev
    model, _, _ = shallow_r18(dev)
    _freeze_layer1(model)
    _fake_grads(model, 3, dev)
    grads = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
    N = _grad_norm64(model, norm_type)
    ret = vfs_amd.clip_grad_norm_(model, 0.25 * N, norm_type=norm_type)
    assert isinstance(ret, torch.Tensor) and ret.dim() == 0 and ret.device.type == dev.type
    assert _within_1ulp(float(ret), N)
    c = np.float32(0.25 * N / (N + 1e-6))
    for n, p in model.named_parameters():
        got = p.grad.detach().cpu()
        if not p.requires_grad:
            assert torch.equal(got, grads[n]), n
            continue
        ref = grads[n].double() * float(c)      # c to 1 ulp, one rounding of the product
        assert bool(((got.double() - ref).abs() <= 3 * 2.0 ** -24 * ref.abs()).all()), n
    # below max_norm: nothing changes
    _fake_grads(model, 3, dev)
    vfs_amd.clip_grad_norm_(model, 4.0 * N, norm_type=norm_type)
    for n, p in model.named_parameters():
        assert torch.equal(p.grad.detach().cpu(), grads[n]), n


class _CountingLib:
    """stands in for the engine's library object and notes the entry points called through it"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        attr = getattr(self._lib, name)
        if not callable(attr) or name in ('last_error', 'cfunc', 'check', 'stream_index'):
            return attr

        def call(*args):
            self.calls.append(name)
            return attr(*args)
        return call


@pytest.mark.parametrize('freeze,segments', [(False, 1), (True, 2)])
def test_launch_count_of_the_step(backend, freeze, segments):
    """grad_clip=None: exactly the launches of the optimizer without the feature (one sgd_step per trainable range); with
    clipping at most two more per step, plus one reduction launch per extra trainable range"""
    dev = backend.dev

    def launches(optimizer_config):
        model, opt, _ = shallow_r18(dev, optimizer_config)
        if freeze:
            _freeze_layer1(model)
        _fake_grads(model, 4, dev)
        opt.step()      # arenas and workspaces exist now
        _fake_grads(model, 5, dev)
        counting = _CountingLib(backend.eng.lib)
        backend.eng.lib = counting
        try:
            opt.step()
        finally:
            backend.eng.lib = counting._lib
        _sync(dev)
        return counting.calls, _snapshot(model)

    plain, p_plain = launches(None)
    off, p_off = launches(dict(grad_clip=None))
    assert plain == off == ['sgd_step'] * segments
    on, p_on = launches(dict(grad_clip=dict(max_norm=1e-3)))
    assert on == ['grad_norm_partial'] * segments + ['grad_norm_finish'] + ['sgd_step_clip'] * segments
    assert len(on) <= len(plain) + 2 + (segments - 1)
    for n in p_plain:
        assert torch.equal(p_plain[n], p_off[n]), n
    assert any(not torch.equal(p_plain[n], p_on[n]) for n in p_plain)


def test_multi_segment_step_clips_by_the_trainable_norm(backend):
    """two trainable ranges through SGD.step: norm over the requires_grad parameters only, frozen ones untouched"""
    dev = backend.dev
    model, _, cfg = shallow_r18(dev)
    _freeze_layer1(model)
    import vfs_amd
    _fake_grads(model, 9, dev)
    N = _grad_norm64(model)
    opt = vfs_amd.build_optimizer(model, cfg.optimizer, optimizer_config=dict(grad_clip=dict(max_norm=0.5 * N)))
    before = _snapshot(model)
    grads = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
    assert len(opt._arena()[1]) == 2
    opt.step()
    _assert_fp64_update(model, before, grads, {n: torch.zeros_like(v) for n, v in before.items()}, 0.5 * N / (N + 1e-6))
    assert _within_1ulp(opt.last_grad_norm(), N)


# ---------------------------------------------------------------------------------------------- 5. two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_compute_the_same_norm_and_stay_identical(tmp_path):
    """data parallel on the CPU (gloo, emulator): step() runs behind the gradient all-reduce, so both ranks reduce the same
    gradients - the same last_grad_norm() bit for bit, without a collective of its own, and identical parameters afterwards"""
    from tests.emu_util import emu_lib
    emu_lib()                                  # build once, before the ranks race for it
    port = str(_free_port())
    procs, outs = [], []
    for r in range(2):
        o = str(tmp_path / f'rank{r}.npz')
        outs.append(o)
        env = dict(os.environ, WORLD_SIZE='2', RANK=str(r), MASTER_ADDR='127.0.0.1', MASTER_PORT=port, VFS_TEST_MAX_NORM='0.05')
        procs.append(subprocess.Popen([sys.executable, WORKER, o], env=env))
    for p in procs:
        assert p.wait(timeout=600) == 0
    r0, r1 = np.load(outs[0]), np.load(outs[1])
    assert r0['norms'].tobytes() == r1['norms'].tobytes()
    assert np.all(r0['norms'] > 0.05) and r0['norms'][0] != r0['norms'][1]
    for k in r0.files:
        assert np.array_equal(r0[k], r1[k]), k
