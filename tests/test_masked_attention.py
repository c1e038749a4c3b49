"""vfs_amd.masked_attention (vfs_amd/attention.py, csrc/attn_train.hip): forward and the gradients wrt query, key and value
against vectors captured from the reference function (tests/golden/gen_masked_attention_grad_golden.py ->
masked_attention_grad.npz, masked_attention_grad_f64.npz), determinism, requires_grad subsets, the refusals, and the composition
with the module-level autograd path.  Every case runs on the fiber emulator and, through the same C ABI, on the GPU.

The bar on values: ||kernel - fp64||_2 / ||fp64||_2 <= 4 x (the reference's own fp32-against-fp64 error, stored in the fixture)
+ one fp32 ulp of the tensor's largest magnitude / ||fp64||_2.  4 x: the kernel's order of summation differs from torch's; both are
fp32 evaluations of the same sums.  The selected keys must be the reference's exactly (the generator refuses seeds at which
top-k membership could depend on the order of summation).  Measured ratios: MEASUREMENTS.md."""
import functools

import numpy as np
import pytest
import torch

from oracle import vfs_oracle as O
from tests import masked_attention_oracle as MO
from tests.golden.gen_masked_attention_grad_golden import CASES, TENSORS, load_case

CASE = {c[0]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def _golden(name):
    return load_case(name)


def _kwargs(case):
    _, N, C, T, H, W, CO, nr, topk, temp, normalize = case
    return dict(neighbor_range=nr, temperature=temp, topk=topk, normalize=normalize)


def _run(backend, name, needs=(True, True, True)):
    """-> out and the gradients wrt (query, key, value) of <out, dout> (None where not required), on the host"""
    import vfs_amd
    g = _golden(name)
    ops = [g[a].clone().to(backend.dev).requires_grad_(need) for a, need in zip(('query', 'key', 'value'), needs)]
    out = vfs_amd.masked_attention(*ops, **_kwargs(CASE[name]))
    assert out.requires_grad == any(needs) and out.dtype == torch.float32
    if any(needs):
        out.backward(g['dout'].to(backend.dev))
    return [out.detach().cpu()] + [None if t.grad is None else t.grad.cpu() for t in ops]


def _ulp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def _bar(got, want64, err_ref):
    """(relative L2 error of `got` against the fp64 array, the bar it has to meet)"""
    err = float((got.double() - want64).norm() / want64.norm())
    return err, 4.0 * err_ref + _ulp(want64.abs().max()) / float(want64.norm())


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_forward_and_gradients_against_the_reference(backend, name):
    from vfs_amd import attention
    case, g = CASE[name], _golden(name)
    _, N, C, T, H, W, CO, nr, topk, temp, normalize = case
    # the selected keys: exactly the reference's, as sets per query (the zero-weight fill is -1 on both sides)
    q, k, v = (g[a].to(backend.dev) for a in ('query', 'key', 'value'))
    _, idx, w, _, _ = attention.attention_forward(backend.lib, backend.eng.stream(backend.dev), q, k, v, (N, C, max(T, 1), H, W, CO),
                                                  nr, temp, topk, normalize)
    idx, w = idx.cpu(), w.cpu()
    assert tuple(idx.shape) == (N, topk, H * W) and bool(((idx >= 0) | (w == 0)).all()) and bool((idx < max(T, 1) * H * W).all())
    assert torch.equal(idx.permute(0, 2, 1).sort(dim=2).values, g['idx']), 'selected keys differ from the reference'
    assert torch.allclose(w.sum(dim=1), torch.ones(N, H * W), atol=1e-6)
    if name == 'fewer_than_topk':
        assert int((idx < 0).sum()) == N * H * W      # two in-window keys, topk = 3: one fill per query
    got = dict(zip(TENSORS, _run(backend, name)))
    failed = []
    for t in TENSORS:
        assert got[t].shape == g[t].shape and torch.isfinite(got[t]).all(), t
        err, bar = _bar(got[t], g[t + '64'], g['err/' + t])
        print(f'{name} [{backend.name}] {t}: rel-L2 against fp64 {err:.3e}, reference fp32 {g["err/" + t]:.3e}, ratio {err / g["err/" + t]:.2f}')
        if not err <= bar:
            failed.append((t, err, bar))
    assert not failed, failed


def test_backward_is_deterministic(backend):
    a, b = _run(backend, 'odd_channels'), _run(backend, 'odd_channels')
    for t, x, y in zip(TENSORS, a, b):
        assert torch.equal(x, y), t
    assert all(float(x.abs().sum()) > 0 for x in a)


@pytest.mark.parametrize('only', [0, 1, 2], ids=['query', 'key', 'value'])
def test_requires_grad_subsets(backend, only):
    full = _run(backend, 'borders_two_frames')
    part = _run(backend, 'borders_two_frames', needs=tuple(i == only for i in range(3)))
    assert torch.equal(part[0], full[0])
    for i in range(3):
        if i == only:
            assert torch.equal(part[1 + i], full[1 + i]) and float(part[1 + i].abs().sum()) > 0
        else:
            assert part[1 + i] is None


def test_no_grad_inputs_and_non_contiguous_operands(backend):
    import vfs_amd
    g, kw = _golden('borders_two_frames'), _kwargs(CASE['borders_two_frames'])
    q, k, v = (g[a].to(backend.dev) for a in ('query', 'key', 'value'))
    out = vfs_amd.masked_attention(q, k, v, **kw)
    assert not out.requires_grad and out.grad_fn is None
    qt = q.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not qt.is_contiguous()
    assert torch.equal(vfs_amd.masked_attention(qt, k, v, **kw), out)
    assert torch.equal(out.cpu(), _run(backend, 'borders_two_frames')[0])


# ---------------------------------------------------------------------------------------------------------------- refusals
class _NoLaunch:
    """a library that fails the test on any call: the refusals come before a launch"""

    def __init__(self, path):
        self.path = path

    def __getattr__(self, name):
        raise AssertionError(f'vfs_{name} was called')


def _ops(C=64, T=2, CO=3, H=4, W=4):
    return torch.zeros(1, C, H, W), torch.zeros(1, C, T, H, W), torch.zeros(1, CO, T, H, W)


@pytest.mark.parametrize('ops, kw, exc, match', [
    (_ops(), dict(topk=None), NotImplementedError, 'topk=None'),
    (_ops(), dict(topk=11), NotImplementedError, r'1 <= topk <= 10 \(got 11\)'),
    (_ops(), dict(neighbor_range=1), ValueError, r'neighbor_range >= 2 or None \(got 1\)'),
    (_ops(C=96), dict(), NotImplementedError, r'C % 64 == 0 and C <= 2048 \(got C = 96\)'),
    (_ops(T=65), dict(), NotImplementedError, r'1 <= T <= 64 key frames \(got T = 65\)'),
    (_ops(CO=257), dict(), NotImplementedError, r'1 <= CO <= 256 value channels \(got CO = 257\)'),
], ids=['topk-none', 'topk-11', 'neighbor_range-1', 'C-96', 'T-65', 'CO-257'])
def test_refusals(ops, kw, exc, match):
    import vfs_amd
    from vfs_amd import build, engine
    engine.set_shared_engine(engine.Engine(lib=_NoLaunch(build.EMU_LIB)))      # host tensors are this library's operands: only the shape is wrong
    try:
        with pytest.raises(exc, match=match):
            vfs_amd.masked_attention(*ops, **kw)
    finally:
        engine._ENGINES.clear()


def test_cpu_tensors_are_refused():
    import vfs_amd
    from vfs_amd import _lib, engine
    engine.set_shared_engine(engine.Engine(lib=_NoLaunch(_lib.LIB_PATH)))      # the product library
    try:
        with pytest.raises(RuntimeError, match='cpu tensors; the operator runs on the HIP kernels only'):
            vfs_amd.masked_attention(*_ops())
    finally:
        engine._ENGINES.clear()


@pytest.mark.parametrize('bad, text', [
    (dict(topk=11), '1 <= topk <= 10'), (dict(neighbor_range=1), 'neighbor_range >= 2'), (dict(C=96), 'C % 64 == 0 and C <= 2048'),
    (dict(T=65), '1 <= T <= 64'), (dict(CO=257), '1 <= CO <= 256'), (dict(T=64, H=8192, W=8192), 'T * H * W < 2^31'),
], ids=['topk-11', 'neighbor_range-1', 'C-96', 'T-65', 'CO-257', 'THW-2^32'])
def test_c_boundary_refuses_the_same_shapes(bad, text):
    """the entry points check before they touch an operand: null pointers and no launch"""
    from tests.emu_util import emu_lib
    from vfs_amd._lib import VfsError
    lib = emu_lib()
    a = dict(N=1, C=64, T=2, H=4, W=4, CO=3, neighbor_range=4, topk=3)
    a.update(bad)
    shape = (a['N'], a['C'], a['T'], a['H'], a['W'], a['CO'])
    with pytest.raises(VfsError, match='masked_attention_fwd.*' + text.replace('^', r'\^').replace('*', r'\*')):
        lib.masked_attention_fwd(None, None, None, None, None, None, None, None, *shape, a['neighbor_range'], a['topk'], 1.0, 1, None)
    with pytest.raises(VfsError, match='masked_attention_bwd.*' + text.replace('^', r'\^').replace('*', r'\*')):
        lib.masked_attention_bwd(None, None, None, None, None, None, None, None, None, None, None, None, 0, *shape, a['neighbor_range'],
                                 a['topk'], 1.0, 1, None)
    if 'neighbor_range' not in bad:
        nbytes = torch.zeros(1, dtype=torch.int64)
        with pytest.raises(VfsError, match='masked_attention_workspace_bytes'):
            lib.masked_attention_workspace_bytes(*shape, a['topk'], 1, nbytes)


# ---------------------------------------------------------------------------------------------------------------- composition
def _backbone(dev):
    from vfs_amd.resnet import ResNet
    kw = dict(num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,), zero_init_residual=False)
    ref = O.ResNet(18, **kw)
    O.fill_state_dict_(ref, seed=118)
    net = ResNet(18, **kw)
    net.load_state_dict(ref.state_dict())
    return net.to(dev).train()


def test_loss_on_the_autograd_path(backend):
    """ResNet-18 (train mode, stage 2: 4 x 4 maps, C = 256) on two frames -> masked_attention -> MSE -> backward(): the cotangents
    that reach the two stage outputs against torch autograd over the restatement (tests/masked_attention_oracle.py) applied to
    the detached stage outputs, under the bar of this file with the restatement's own fp32-against-fp64 error as the reference
    error; every backbone parameter gets a finite, non-zero gradient."""
    import vfs_amd
    dev = backend.dev
    kw = dict(neighbor_range=4, topk=3, temperature=0.07)
    net = _backbone(dev)
    frames = O.fill_tensor([2, 2, 3, 64, 64], 11, scale=2.0).to(dev)
    value, target = O.fill_tensor([2, 3, 4, 4], 12, scale=1.0).to(dev), O.fill_tensor([2, 3, 4, 4], 13, scale=1.0).to(dev)
    x_q, x_k = net(frames[:, 0].contiguous()), net(frames[:, 1].contiguous())
    assert tuple(x_q.shape) == (2, 256, 4, 4) and x_q.requires_grad and x_q.dtype == torch.float32
    x_q.retain_grad()
    x_k.retain_grad()
    rec = vfs_amd.masked_attention(x_q, x_k, value, **kw)
    loss = torch.nn.functional.mse_loss(rec, target)
    loss.backward()
    want = {}
    for dt in (torch.float32, torch.float64):
        a, b = x_q.detach().cpu().to(dt).requires_grad_(), x_k.detach().cpu().to(dt).requires_grad_()
        r, sel, _ = MO.masked_attention(a, b, value.cpu().to(dt), return_selection=True, **kw)
        lo = torch.nn.functional.mse_loss(r, target.cpu().to(dt))
        lo.backward()
        want[dt] = (lo.detach(), a.grad, b.grad, sel.sort(dim=1).values)
    # the precondition of a comparison of values: fp32 and fp64 select the same keys
    assert torch.equal(want[torch.float32][3], want[torch.float64][3]), 'top-k membership of this input depends on the precision'
    assert abs(float(loss.detach()) - float(want[torch.float64][0])) <= 1e-5 * abs(float(want[torch.float64][0]))
    for name, got, i in (('d x_q', x_q.grad, 1), ('d x_k', x_k.grad, 2)):
        w64 = want[torch.float64][i]
        err_ref = float((want[torch.float32][i].double() - w64).norm() / w64.norm())
        err, bar = _bar(got.cpu(), w64, err_ref)
        print(f'composition [{backend.name}] {name}: rel-L2 against fp64 {err:.3e}, restatement fp32 {err_ref:.3e}, ratio {err / err_ref:.2f}')
        assert err <= bar, (name, err, bar)
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, n
