"""Optimizers on the flat arena with param groups (optimizer = dict(type='SGD' | 'Adam' | 'AdamW', ..., paramwise_cfg=...),
configs/r*_*.py:134 -> mmcv build_optimizer, apis/train.py:72): the table-driven update kernel vfs_opt_step_table against the
single-group kernels and against torch.optim on the CPU, its segment map and argument checks, and the whole thing through
vfs_amd.build_optimizer / step() / state_dict().  backend=emu: CPU fiber emulator; backend=gpu: libvfs_hip.so on the MI355X."""
import copy
import os

import numpy as np
import pytest
import torch

from tests.grad_clip_worker import shallow_r18

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SGD, ADAM, ADAMW = 0, 1, 2
LR, MOM, WD = 0.05, 0.9, 1e-4      # configs/vfs_r18.py optimizer
GRID_PASS = 4096 * 1024            # words one pass of the update kernels' grid covers (4096 workgroups x 256 lanes x 4 words)
U = 2.0 ** -24


def _map(lib, segs, n, ngroups):
    """host: the segment map for segments [(begin, end, group), ...] of an arena of n words"""
    words = torch.zeros(1, dtype=torch.int64)
    lib.opt_segment_map_words(n, len(segs), words)
    m = torch.zeros(max(int(words), 4), dtype=torch.int32)
    lib.opt_segment_map(torch.tensor(segs, dtype=torch.int64).reshape(-1, 3), len(segs), n, ngroups, m, m.numel())
    return m


def _table_step(backend, kind, p, g, s1, s2, segs, rows, nesterov=0, step=1, clip=None, skip=None):
    """one vfs_opt_step_table launch on host tensors; rows: per group (lr, wd, momentum) or (lr, wd, beta1, beta2, eps)"""
    n = p.numel()
    m = _map(backend.lib, segs, n, len(rows))
    hyper = torch.zeros(len(rows), 8)
    hyper[:, :len(rows[0])] = torch.tensor(rows, dtype=torch.float32)
    table = torch.zeros(len(rows) * 8)
    # hyper stays host memory on both backends: its address goes in as an integer
    backend.hostlib.opt_step_table(kind, p, g, s1, s2, n, m, len(segs), hyper.data_ptr(), len(rows), table, nesterov, step, clip, skip, None)


def _inputs(n, seed=5):
    gen = torch.Generator().manual_seed(seed + n)
    return (torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1, torch.randn(n, generator=gen) * 0.1,
            torch.rand(n, generator=gen) * 0.01)


def _clip_of(backend, g, max_norm):
    """the device coefficient as the optimizer gets it: reduction + finish -> float32 [norm, coefficient]"""
    r = torch.zeros(1, dtype=torch.int32)
    backend.lib.grad_norm_rows(r)
    rows = torch.zeros(int(r), dtype=torch.float64)
    out = torch.zeros(2)
    backend.hostlib.grad_norm_partial(g, g.numel(), 2.0, rows, 0, None)
    backend.hostlib.grad_norm_finish(rows, 2.0, max_norm, out, None)
    return out


# ---------------------------------------------------------------------------------------------- 1. against the parent's kernels
@pytest.mark.parametrize('clip', [False, True])
@pytest.mark.parametrize('n', [4, 8, 1028, 'pass+5'])
def test_one_group_equals_the_single_group_kernels_bit_for_bit(backend, n, clip):
    """one group, multipliers 1, no nesterov: p and buf are vfs_sgd_step's / vfs_sgd_step_clip's bits.  'pass+5': five words past
    one pass of the grid, so the stride loop runs a second time and the segment ends in a partial vector"""
    if n == 'pass+5':
        n = GRID_PASS + 5
    p, g, buf, _ = _inputs(n)
    c = torch.tensor([0.37]) if clip else None
    p0, b0, g0 = p.clone(), buf.clone(), g.clone()
    if clip:
        backend.hostlib.sgd_step_clip(p0, g, b0, n, LR, MOM, WD, c, None, None)
    else:
        backend.hostlib.sgd_step(p0, g, b0, n, LR, MOM, WD, None, None)
    _table_step(backend, SGD, p, g, buf, None, [(0, n, 0)], [(LR, WD, MOM)], clip=c)
    assert torch.equal(p, p0) and torch.equal(buf, b0)
    assert torch.equal(g, g0)
    assert not torch.equal(p, _inputs(n)[0])


# ---------------------------------------------------------------------------------------------- 2. segments and groups
# parameter sizes 1, 3, 4, 5, 1024, 1021, 1027 (each padded to 4 words), a frozen range in front, one between two trainable
# parameters, one at the end.  Offsets: the 1024-word parameter begins and ends ON a chunk edge (1024, 2048), the 1021-word one
# ends three words BEFORE the edge 3072 (its padding reaches it), the 1027-word one ends three words AFTER the edge 4096.
LAYOUT = [(1, None), (1, 0), (3, 1), (4, 2), (5, 0), (1000, None), (1024, 1), (1021, 2), (1027, 0), (9, None)]      # (numel, group | frozen)
GROUPS_SGD = [(0.05, 1e-4, 0.9), (0.5, 0.0, 0.5), (0.01, 1e-2, 0.0)]
GROUPS_ADAM = [(1e-3, 1e-2, 0.9, 0.999, 1e-8), (1e-2, 0.0, 0.8, 0.99, 1e-6), (3e-4, 0.1, 0.95, 0.9, 1e-8)]


def _layout():
    offs, o = [], 0
    for numel, _ in LAYOUT:
        offs.append(o)
        o += (numel + 3) // 4 * 4
    assert [offs[6], offs[7], offs[7] + 1021, offs[8], offs[8] + 1027] == [1024, 2048, 3069, 3072, 4099]
    return offs, o


@pytest.mark.parametrize('kind', [SGD, ADAMW])
def test_segments_and_groups(backend, kind):
    """every trainable parameter equals the single-segment kernel run on that parameter alone with its group's values (SGD: the
    parent's vfs_sgd_step; AdamW: this kernel with one segment), every frozen and padding word of p and of the state arenas keeps
    its bit pattern, and a second run from the same inputs gives the same bits"""
    offs, n = _layout()
    rows = GROUPS_SGD if kind == SGD else GROUPS_ADAM
    p, g, s1, s2 = _inputs(n)
    inside = torch.zeros(n, dtype=torch.bool)
    for (numel, grp), o in zip(LAYOUT, offs):
        inside[o:o + numel] = True
    for t in (p, s1, s2):
        t[~inside] = 7.0      # padding: a sentinel
    segs = [(o, o + numel, grp) for (numel, grp), o in zip(LAYOUT, offs) if grp is not None]
    trainable = torch.zeros(n, dtype=torch.bool)
    for b, e, _ in segs:
        trainable[b:e] = True
    runs = []
    for _ in range(2):
        q, a, b = p.clone(), s1.clone(), s2.clone()
        _table_step(backend, kind, q, g, a, b if kind != SGD else None, segs, rows, step=3)
        runs.append((q, a, b))
    (q, a, b), again = runs
    assert all(torch.equal(x, y) for x, y in zip(runs[0], again))
    for lo, hi, grp in segs:
        qp, qg, qa, qb = p[lo:hi].clone(), g[lo:hi].clone(), s1[lo:hi].clone(), s2[lo:hi].clone()
        if kind == SGD:
            lr, wd, mom = rows[grp]
            backend.hostlib.sgd_step(qp, qg, qa, hi - lo, lr, mom, wd, None, None)
        else:
            _table_step(backend, kind, qp, qg, qa, qb, [(0, hi - lo, 0)], [rows[grp]], step=3)
        assert torch.equal(q[lo:hi], qp) and torch.equal(a[lo:hi], qa), (lo, hi)
        assert not torch.equal(qp, p[lo:hi])
        if kind != SGD:
            assert torch.equal(b[lo:hi], qb), (lo, hi)
    for new, old in ((q, p), (a, s1), (b, s2)):
        assert new[~trainable].numpy().tobytes() == old[~trainable].numpy().tobytes()
    assert float((q[~inside] - 7.0).abs().max()) == 0.0


@pytest.mark.parametrize('ngroups', [224, 225, 448])
def test_group_counts_around_the_by_value_limit(backend, ngroups):
    """up to 224 groups the rows are arguments of the update launch, more go through the device table in launches of 224: one
    5-word parameter per group, each group its own lr, wd and momentum; every parameter is vfs_sgd_step's bits with its group's
    values, the padding keeps its sentinel"""
    n = 8 * ngroups
    p, g, buf, _ = _inputs(n)
    pad = torch.ones(n, dtype=torch.bool)
    for k in range(ngroups):
        pad[8 * k:8 * k + 5] = False
    p[pad], buf[pad] = 7.0, 7.0
    rows = [(0.01 * (k + 1), 1e-4 * (k % 7), 0.5 + 0.001 * k) for k in range(ngroups)]
    segs = [(8 * k, 8 * k + 5, k) for k in range(ngroups)]
    q, a = p.clone(), buf.clone()
    _table_step(backend, SGD, q, g, a, None, segs, rows)
    for k in (0, 1, 111, 112, 223, 224, 225, 300, 447):
        if k >= ngroups:
            continue
        qp, qa = p[8 * k:8 * k + 5].clone(), buf[8 * k:8 * k + 5].clone()
        lr, wd, mom = rows[k]
        backend.hostlib.sgd_step(qp, g[8 * k:8 * k + 5].clone(), qa, 5, lr, mom, wd, None, None)
        assert torch.equal(q[8 * k:8 * k + 5], qp) and torch.equal(a[8 * k:8 * k + 5], qa), k
    assert bool((q[pad] == 7.0).all()) and bool((a[pad] == 7.0).all())
    assert not bool((q[~pad] == p[~pad]).any())


# ---------------------------------------------------------------------------------------------- 3. against torch.optim on the CPU
def _fresh_grad(n, step):
    return torch.randn(n, generator=torch.Generator().manual_seed(100 + step)) * 0.1


@pytest.mark.parametrize('clip', [False, True])
def test_nesterov_sgd_against_torch(backend, clip):
    """three steps with fresh gradients and weight decay.  Each step is compared with torch.optim.SGD(nesterov=True) in fp64,
    stepped from the kernel's own state before the step (the scalars as the kernel receives them, rounded to fp32), with the bound
    test_grad_clip.py applies to the clipped step: a few fp32 roundings per element, 8 x 2^-24 x the magnitudes that are added -
    buf: |m buf| + |g c| + |wd p|; p: |p| + lr (|g c| + |wd p| + m |buf'|), the nesterov term included.  With clip the reference
    is torch after clip_grad_norm_; the kernel's fp32 coefficient is within 1 ulp of that one: 2 x 2^-24 x lr (1 + m) |g c| more"""
    n = 1027
    p, _, buf, _ = _inputs(n)
    buf.zero_()      # torch's first step: buf = g'
    lr, mom, wd = (float(np.float32(v)) for v in (LR, MOM, 1e-2))
    for step in range(3):
        g = _fresh_grad(n, step)
        q = p.double().clone().requires_grad_(True)
        q.grad = g.double().clone()
        c = None
        if clip:
            max_norm = 0.5 * float(g.double().norm())
            c = _clip_of(backend, g, max_norm)[1:2].clone()
            torch.nn.utils.clip_grad_norm_([q], max_norm)
        opt = torch.optim.SGD([q], lr=lr, momentum=mom, weight_decay=wd, nesterov=True)
        if step:
            opt.state[q]['momentum_buffer'] = buf.double().clone()
        gc, p0, b0 = q.grad.clone(), p.double(), buf.double()
        opt.step()
        _table_step(backend, SGD, p, g, buf, None, [(0, n, 0)], [(LR, 1e-2, MOM)], nesterov=1, clip=c)
        mag = (mom * b0).abs() + gc.abs() + (wd * p0).abs()
        extra = 2 * U * gc.abs() if clip else 0.0
        eb = (buf.double() - opt.state[q]['momentum_buffer']).abs()
        ep = (p.double() - q.detach()).abs()
        bound_b = 8 * U * mag + extra
        bound_p = 8 * U * (p0.abs() + lr * (gc.abs() + (wd * p0).abs() + mom * mag)) + lr * (1 + mom) * extra
        print(step, clip, 'worst / bound', float((eb / bound_b).max()), float((ep / bound_p).max()))
        assert bool((eb <= bound_b).all()) and bool((ep <= bound_p).all())
    assert not torch.equal(p, _inputs(n)[0])


@pytest.mark.parametrize('clip', [False, True])
@pytest.mark.parametrize('kind', [ADAM, ADAMW])
def test_adam_and_adamw_against_torch(backend, kind, clip):
    """three steps with fresh gradients and weight decay against torch.optim.Adam / AdamW on the CPU: max abs difference < 1e-6
    with lr = 1e-3 and unit-scale parameters (tests/test_siamfc.py:test_adam_kernel_equals_torch)"""
    n = 1027
    p, _, _, _ = _inputs(n)
    m, v = torch.zeros(n), torch.zeros(n)
    ref = p.clone().requires_grad_(True)
    opt = (torch.optim.Adam if kind == ADAM else torch.optim.AdamW)([ref], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for step in range(1, 4):
        g = _fresh_grad(n, step)
        ref.grad = g.clone()
        c = None
        if clip:
            max_norm = 0.5 * float(g.double().norm())
            c = _clip_of(backend, g, max_norm)[1:2].clone()
            torch.nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
        _table_step(backend, kind, p, g, m, v, [(0, n, 0)], [(1e-3, 1e-2, 0.9, 0.999, 1e-8)], step=step, clip=c)
        errs = [float((a - b).abs().max()) for a, b in ((p, ref.detach()), (m, opt.state[ref]['exp_avg']), (v, opt.state[ref]['exp_avg_sq']))]
        print(kind, clip, step, errs)
        assert max(errs) < 1e-6
    assert float((p - _inputs(n)[0]).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------- 4. the skip word
@pytest.mark.parametrize('kind', [SGD, ADAM, ADAMW])
def test_skip_word(backend, kind):
    n = 1028
    p, g, s1, s2 = _inputs(n)
    rows = [GROUPS_SGD[0]] if kind == SGD else [GROUPS_ADAM[0]]
    before = [t.clone() for t in (p, g, s1, s2)]
    args = (backend, kind, p, g, s1, s2 if kind != SGD else None, [(0, n, 0)], rows)
    _table_step(*args, skip=torch.ones(1, dtype=torch.int64))
    assert all(torch.equal(a, b) for a, b in zip((p, g, s1, s2), before))
    for skip in (torch.zeros(1, dtype=torch.int64), None):
        p0, s0 = p.clone(), s1.clone()
        _table_step(*args, skip=skip)
        assert not torch.equal(p, p0) and not torch.equal(s1, s0) and torch.equal(g, before[1])


# ---------------------------------------------------------------------------------------------- 5. argument errors
def _error_cases():
    P = torch.zeros(64)
    H = torch.zeros(8)
    H[2] = 0.9
    H0 = torch.zeros(8)
    W = torch.zeros(1, dtype=torch.int64)
    M = torch.zeros(64, dtype=torch.int32)
    ARG = -3

    def step(kind=SGD, p=P, g=P, s1=P, s2=P, n=16, m=M, nseg=1, h=H, ng=1, t=P, nest=0, st=1):
        return (kind, p, g, s1, s2, n, m, nseg, h, ng, t, nest, st, None, None, None)

    def seg(s, nseg=None, n=64, ng=2, m=M, words=64):
        t = torch.tensor(s, dtype=torch.int64) if s is not None else None
        return (t, len(s) if nseg is None else nseg, n, ng, m, words)
    who, mp = 'opt_step_table: ', 'opt_segment_map: '
    return [
        ('opt_step_table', step(kind=3), ARG, who + 'kind must be 0 (SGD), 1 (Adam) or 2 (AdamW)'),
        ('opt_step_table', step(p=None), ARG, who + 'null buffer'),
        ('opt_step_table', step(g=None), ARG, who + 'null buffer'),
        ('opt_step_table', step(s1=None), ARG, who + 'null buffer'),
        ('opt_step_table', step(kind=ADAM, s2=None), ARG, who + 'null buffer'),
        ('opt_step_table', step(m=None), ARG, who + 'null buffer'),
        ('opt_step_table', step(h=None), ARG, who + 'null buffer'),
        ('opt_step_table', step(t=None), ARG, who + 'null buffer'),
        ('opt_step_table', step(p=P[1:]), ARG, who + '16-byte aligned buffers'),
        ('opt_step_table', step(g=P[1:]), ARG, who + '16-byte aligned buffers'),
        ('opt_step_table', step(s1=P[2:]), ARG, who + '16-byte aligned buffers'),
        ('opt_step_table', step(kind=ADAMW, s2=P[3:]), ARG, who + '16-byte aligned buffers'),
        ('opt_step_table', step(n=-1), ARG, who + 'n < 0'),
        ('opt_step_table', step(nseg=-1), ARG, who + 'nseg < 0'),
        ('opt_step_table', step(ng=0), ARG, who + '1 <= ngroups <= 448'),
        ('opt_step_table', step(ng=449), ARG, who + '1 <= ngroups <= 448'),
        ('opt_step_table', step(kind=ADAM, st=0), ARG, who + 'step >= 1'),
        ('opt_step_table', step(kind=ADAMW, st=-2), ARG, who + 'step >= 1'),
        ('opt_step_table', step(kind=ADAM, nest=1), ARG, who + "nesterov is SGD's"),
        ('opt_step_table', step(h=H0, nest=1), ARG, who + 'nesterov needs momentum > 0'),
        ('opt_segment_map_words', (16, 1, None), ARG, 'opt_segment_map_words: bad argument'),
        ('opt_segment_map_words', (-1, 1, W), ARG, 'opt_segment_map_words: bad argument'),
        ('opt_segment_map', seg(None, nseg=1), ARG, mp + 'null buffer'),
        ('opt_segment_map', seg([[0, 4, 0]], m=None), ARG, mp + 'null buffer'),
        ('opt_segment_map', seg([[0, 4, 0]], n=-1), ARG, mp + 'n < 0'),
        ('opt_segment_map', seg([[0, 4, 0]], ng=449), ARG, mp + '1 <= ngroups <= 448'),
        ('opt_segment_map', seg([[0, 4, 0]], words=4), ARG, mp + 'map smaller than vfs_opt_segment_map_words(n, nseg)'),
        ('opt_segment_map', seg([[0, 65, 0]]), ARG, mp + 'segments must be non-empty and inside [0, n)'),
        ('opt_segment_map', seg([[-4, 4, 0]]), ARG, mp + 'segments must be non-empty and inside [0, n)'),
        ('opt_segment_map', seg([[8, 8, 0]]), ARG, mp + 'segments must be non-empty and inside [0, n)'),
        ('opt_segment_map', seg([[2, 8, 0]]), ARG, mp + 'segments must begin on a multiple of 4 words'),
        ('opt_segment_map', seg([[8, 12, 0], [0, 4, 1]]), ARG, mp + 'segments must be sorted and must not share a 16-byte vector'),
        ('opt_segment_map', seg([[0, 9, 0], [8, 12, 1]]), ARG, mp + 'segments must be sorted and must not share a 16-byte vector'),
        ('opt_segment_map', seg([[0, 4, 2]]), ARG, mp + 'segment group outside [0, ngroups)'),
        ('opt_segment_map', seg([[0, 4, -1]]), ARG, mp + 'segment group outside [0, ngroups)'),
    ]


@pytest.mark.parametrize('name,args,code,message', _error_cases())
def test_argument_errors(name, args, code, message):
    """each bad argument returns its code before anything is launched; the message names the entry point and the argument"""
    from tests.emu_util import emu_lib
    lib = emu_lib()
    fn = lib.cfunc(name)
    assert len(args) == len(lib.protos['vfs_' + name][1]), 'the case does not match the prototype'
    rc = fn(*[a.data_ptr() if hasattr(a, 'data_ptr') else a for a in args])
    assert (rc, lib.last_error()) == (code, message)


def test_segment_map_contents():
    """the map of the hand-made layout: per segment {begin / 4, end / 4, group, end % 4}, then per 1024-word chunk the first
    segment that ends behind the chunk's first word"""
    from tests.emu_util import emu_lib
    offs, n = _layout()
    segs = [(o, o + numel, grp) for (numel, grp), o in zip(LAYOUT, offs) if grp is not None]
    m = _map(emu_lib(), segs, n, 3).tolist()
    assert m[:4 * len(segs)] == [v for b, e, grp in segs for v in (b // 4, e // 4, grp, e % 4)]
    assert m[4 * len(segs):4 * len(segs) + (n + 1023) // 1024] == [0, 4, 5, 6, 6]
    assert len(m) == 4 * len(segs) + 5


# ---------------------------------------------------------------------------------------------- 6. through the model
PARAMWISE = dict(norm_decay_mult=0., bias_decay_mult=0., bias_lr_mult=2., custom_keys={'img_head': dict(lr_mult=10.)})


def _sync(dev):
    if dev.type == 'cuda':
        torch.cuda.synchronize()


def _set_grads(model, seed, dev):
    """deterministic gradients through the arena's per-parameter views (no forward / backward: no bf16 noise)"""
    model._ensure_arena()
    gen = torch.Generator().manual_seed(seed)
    grads = {}
    for n, p in model.named_parameters():
        grads[n] = torch.randn(p.shape, generator=gen) * 0.01
        p.grad.copy_(grads[n].to(dev))
    return grads


def _snapshot(model):
    return {n: p.detach().cpu().clone() for n, p in model.named_parameters()}


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


def _counted_step(backend, opt):
    counting = _CountingLib(backend.eng.lib)
    backend.eng.lib = counting
    try:
        opt.step()
    finally:
        backend.eng.lib = counting._lib
    _sync(backend.dev)
    _counted_step.host_only = [c for c in counting.calls if c.startswith('opt_segment_map')]
    # the launches: the map builders and the size query of the norm workspace run on the host, once
    return [c for c in counting.calls if not c.startswith('opt_segment_map') and c != 'grad_norm_rows']


def _build(dev, optimizer, optimizer_config=None):
    import vfs_amd
    model, _, cfg = shallow_r18(dev)
    return model, vfs_amd.build_optimizer(model, optimizer, optimizer_config=optimizer_config), cfg


def _torch_twin(cls, model, opt, dtype, **kw):
    """the same-named torch optimizer over CPU clones of the parameters, built from opt's groups"""
    clones = {id(p): p.detach().cpu().to(dtype).clone().requires_grad_(True) for p in model.parameters()}
    groups = [dict(params=[clones[id(p)] for p in grp['params']], lr=grp['lr'], weight_decay=grp['weight_decay']) for grp in opt.param_groups]
    names = {n: clones[id(p)] for n, p in model.named_parameters() if p.requires_grad}
    return cls(groups, **kw), names


def test_paramwise_groups_are_mmcv_s(emu_backend):
    model, opt, _ = _build(emu_backend.dev, dict(type='SGD', lr=0.05, momentum=0.9, weight_decay=1e-4, paramwise_cfg=PARAMWISE))
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    assert len(opt.param_groups) == len(named)
    got = {}
    for (n, p), grp in zip(named, opt.param_groups):
        assert len(grp['params']) == 1 and grp['params'][0] is p, n
        assert grp['momentum'] == 0.9 and 'initial_lr' not in grp
        got[n] = (grp['lr'], grp['weight_decay'])
    norm_w = next(n for n, _ in named if n.startswith('backbone.') and n.endswith('bn.weight'))
    norm_b = next(n for n, _ in named if n.startswith('backbone.') and n.endswith('bn.bias'))
    conv_w = next(n for n, _ in named if n.startswith('backbone.') and n.endswith('conv.weight'))
    head_b = next(n for n, p in named if n.startswith('img_head.') and n.endswith('.bias') and
                  isinstance(dict(model.named_modules())[n.rsplit('.', 1)[0]], torch.nn.Linear))
    assert got[norm_w] == (0.05, 0.0)          # norm_decay_mult
    assert got[norm_b] == (0.05, 0.0)          # the bias of a norm layer: no bias_lr_mult
    assert got[conv_w] == (0.05, 1e-4)
    assert got[head_b] == (0.5, 1e-4)          # custom key wins alone: lr x 10, neither bias_lr_mult nor bias_decay_mult
    assert all(v == (0.5, 1e-4) for n, v in got.items() if 'img_head' in n)
    # without the custom key the head's Linear bias gets bias_lr_mult and bias_decay_mult
    import vfs_amd
    opt2 = vfs_amd.build_optimizer(model, dict(type='SGD', lr=0.05, paramwise_cfg=dict(PARAMWISE, custom_keys={})))
    assert next((g['lr'], g['weight_decay']) for (n, _), g in zip(named, opt2.param_groups) if n == head_b) == (0.1, 0.0)
    # longest key first
    opt3 = vfs_amd.build_optimizer(model, dict(type='SGD', lr=1.0, weight_decay=1.0, paramwise_cfg=dict(
        custom_keys={'backbone': dict(lr_mult=2.), 'backbone.layer1': dict(decay_mult=3.)})))
    for (n, _), g in zip(named, opt3.param_groups):
        want = (1.0, 3.0) if 'backbone.layer1' in n else (2.0, 1.0) if 'backbone' in n else (1.0, 1.0)
        assert (g['lr'], g['weight_decay']) == want, n
    # frozen parameters get no group
    for n, p in model.named_parameters():
        p.requires_grad = not n.startswith('backbone.layer1.')
    opt4 = vfs_amd.build_optimizer(model, dict(type='SGD', lr=0.05, paramwise_cfg=PARAMWISE))
    assert len(opt4.param_groups) == sum(p.requires_grad for p in model.parameters()) < len(named)


def test_build_optimizer_refusals(emu_backend):
    import vfs_amd
    model, _, cfg = shallow_r18(emu_backend.dev)
    build = lambda **kw: vfs_amd.build_optimizer(model, dict(cfg.optimizer, **kw))
    with pytest.raises(KeyError):
        build(type='LARS')
    with pytest.raises(NotImplementedError, match='centered'):
        build(centered=True)
    with pytest.raises(NotImplementedError, match='dampening'):
        build(dampening=0.1)
    with pytest.raises(ValueError):
        build(nesterov=True, momentum=0)
    with pytest.raises(NotImplementedError, match='amsgrad'):
        vfs_amd.build_optimizer(model, dict(type='Adam', lr=1e-3, amsgrad=True))
    with pytest.raises(NotImplementedError, match='momentum'):
        vfs_amd.build_optimizer(model, dict(type='AdamW', lr=1e-3, momentum=0.9))
    with pytest.raises(NotImplementedError, match='no_such_mult'):
        build(paramwise_cfg=dict(no_such_mult=2.))
    assert len(build(paramwise_cfg=dict(dwconv_decay_mult=0., bypass_duplicate=True)).param_groups) == len(list(model.parameters()))
    assert build(dampening=0, nesterov=True).param_groups[0]['nesterov'] is True
    opt = build()
    opt.param_groups = [dict(opt.param_groups[0]) for _ in range(449)]
    with pytest.raises(ValueError, match='448'):
        opt.param_groups[0]['lr'] = 0.1      # the groups differ now: the table path
        _set_grads(model, 1, emu_backend.dev)
        opt.step()


def test_a_changed_group_list_rebuilds_the_table(emu_backend):
    """groups added after the first table step: the map and the table follow the new list"""
    model, opt, _ = _build(emu_backend.dev, dict(type='SGD', lr=0.05, momentum=0.9, weight_decay=1e-4, paramwise_cfg=PARAMWISE))
    _set_grads(model, 20, emu_backend.dev)
    opt.step()
    last = opt.param_groups[-1]
    opt.param_groups.append(dict(last, params=[]))      # a group that owns nothing
    before = _snapshot(model)
    assert _counted_step(emu_backend, opt) == ['opt_step_table'] and _counted_step.host_only
    assert all(not torch.equal(p.detach(), before[n]) for n, p in model.named_parameters())


def test_paramwise_sgd_steps_match_torch(backend):
    """two step() calls with paramwise groups: one launch each, and after each every parameter matches torch.optim.SGD (fp64, built
    from the same groups on CPU clones of the state before the step) under the bound of test_nesterov_sgd_against_torch without
    its nesterov and clip terms; a group's changed lr holds at the next step"""
    dev = backend.dev
    model, opt, _ = _build(dev, dict(type='SGD', lr=0.05, momentum=0.9, weight_decay=1e-4, paramwise_cfg=PARAMWISE))
    named = dict(model.named_parameters())
    for step in range(2):
        if step:
            for grp in opt.param_groups[::3]:
                grp['lr'] *= 0.5
        grads = _set_grads(model, 30 + step, dev)
        before = _snapshot(model)
        bufs = {n: opt.state[named[n]]['momentum_buffer'].detach().cpu().clone() if step else torch.zeros_like(before[n]) for n in named}
        twin, tw = _torch_twin(torch.optim.SGD, model, opt, torch.float64, momentum=float(np.float32(0.9)))
        for grp in twin.param_groups:
            grp['lr'], grp['weight_decay'] = float(np.float32(grp['lr'])), float(np.float32(grp['weight_decay']))
        for n, q in tw.items():
            q.grad = grads[n].double()
            if step:
                twin.state[q]['momentum_buffer'] = bufs[n].double().clone()
        twin.step()
        assert _counted_step(backend, opt) == ['opt_step_table']
        assert bool(_counted_step.host_only) == (step == 0), 'the segment map is built once per arena layout'
        worst = 0.0
        for (n, q), grp in zip(tw.items(), twin.param_groups):
            p0, g, b0 = before[n].double(), grads[n].double(), bufs[n].double()
            mag = (0.9 * b0).abs() + g.abs() + (grp['weight_decay'] * p0).abs()
            bound = 8 * U * (p0.abs() + grp['lr'] * mag)
            err = (named[n].detach().cpu().double() - q.detach()).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert bool((err <= bound).all()), (step, n)
            assert not torch.equal(named[n].detach().cpu(), before[n]), n
        print(step, 'worst error / bound', worst)


def test_paramwise_adamw_matches_torch_and_state_dict_round_trips(backend):
    """type='AdamW' with paramwise groups: two steps against torch.optim.AdamW on CPU clones (max abs difference < 1e-6, as the
    kernel test), one launch per step; then state_dict() into the torch optimizer and back - a third step there and here, and a
    fourth here from torch's state_dict, end at the same values"""
    dev = backend.dev
    model, opt, _ = _build(dev, dict(type='AdamW', lr=1e-3, weight_decay=1e-2, paramwise_cfg=PARAMWISE))
    assert type(opt).__name__ == 'AdamW' and len(opt.param_groups) == len(list(model.parameters()))
    named = dict(model.named_parameters())
    twin, tw = _torch_twin(torch.optim.AdamW, model, opt, torch.float32, betas=(0.9, 0.999), eps=1e-8)

    def both(step, twin):
        grads = _set_grads(model, 40 + step, dev)
        for n, q in tw.items():
            q.grad = grads[n].clone()
        twin.step()
        assert _counted_step(backend, opt) == ['opt_step_table']
        err = max(float((named[n].detach().cpu() - q.detach()).abs().max()) for n, q in tw.items())
        print(step, 'max abs difference', err)
        assert err < 1e-6
    before = _snapshot(model)
    both(0, twin)
    both(1, twin)
    assert all(not torch.equal(named[n].detach().cpu(), before[n]) for n in named)
    assert all(float(opt.state[p]['step']) == 2.0 for p in model.parameters())
    # into a fresh torch optimizer over the current values ...
    sd = copy.deepcopy(opt.state_dict())      # state_dict() hands out the arena views themselves, as torch's hands out its tensors
    assert sorted(sd['state'][0]) == ['exp_avg', 'exp_avg_sq', 'step']
    for n, q in tw.items():
        q.data.copy_(named[n].detach().cpu())
    fresh = torch.optim.AdamW([dict(params=g['params']) for g in twin.param_groups], lr=1.0)
    fresh.load_state_dict(sd)
    both(2, fresh)
    # ... and back
    opt.load_state_dict(fresh.state_dict())
    assert all(float(opt.state[p]['step']) == 3.0 for p in model.parameters())
    both(3, fresh)
    bad = fresh.state_dict()
    bad['state'][1]['step'] = bad['state'][1]['step'] + 1
    with pytest.raises(ValueError, match='step'):
        opt.load_state_dict(bad)


def test_sgd_state_dict_round_trips_with_torch(backend):
    """nesterov SGD with paramwise groups: state_dict() loads into torch.optim.SGD (the buffers bit for bit, the groups with every key
    torch's step reads) and torch's state_dict() loads back (the same bits in the momentum arena); the run then goes on: each of
    two further steps equals torch.optim.SGD(nesterov=True) in fp64 stepped from the state before it, under the bound of
    test_nesterov_sgd_against_torch (8 x 2^-24 x the magnitudes that are added; no clip term)"""
    dev = backend.dev
    model, opt, _ = _build(dev, dict(type='SGD', lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True, paramwise_cfg=PARAMWISE))
    named = dict(model.named_parameters())
    _set_grads(model, 50, dev)
    opt.step()
    _sync(dev)
    twin, tw = _torch_twin(torch.optim.SGD, model, opt, torch.float32, momentum=0.5)
    twin.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert twin.param_groups[0]['nesterov'] is True and twin.param_groups[0]['momentum'] == 0.9
    bufs = {n: opt.state[named[n]]['momentum_buffer'].detach().cpu().clone() for n in tw}
    for n, q in tw.items():
        assert torch.equal(twin.state[q]['momentum_buffer'], bufs[n]), n
    for n, q in tw.items():      # torch takes a step of its own, so that what comes back differs from what went out
        q.grad = torch.full_like(q, 0.01)
    twin.step()
    opt.load_state_dict(copy.deepcopy(twin.state_dict()))
    for n, q in tw.items():
        got = opt.state[named[n]]['momentum_buffer']
        assert got.device.type == dev.type and torch.equal(got.detach().cpu(), twin.state[q]['momentum_buffer']), n
        assert not torch.equal(got.detach().cpu(), bufs[n]), n
    mom = float(np.float32(0.9))
    for step in (51, 52):
        grads = _set_grads(model, step, dev)
        before = _snapshot(model)
        bufs = {n: opt.state[named[n]]['momentum_buffer'].detach().cpu().clone() for n in tw}
        ref, rw = _torch_twin(torch.optim.SGD, model, opt, torch.float64, momentum=mom, nesterov=True)
        for grp in ref.param_groups:
            grp['lr'], grp['weight_decay'] = float(np.float32(grp['lr'])), float(np.float32(grp['weight_decay']))
        for n, q in rw.items():
            q.grad = grads[n].double()
            ref.state[q]['momentum_buffer'] = bufs[n].double().clone()
        ref.step()
        assert _counted_step(backend, opt) == ['opt_step_table']
        for (n, q), grp in zip(rw.items(), ref.param_groups):
            p0, g, b0 = before[n].double(), grads[n].double(), bufs[n].double()
            mag = (mom * b0).abs() + g.abs() + (grp['weight_decay'] * p0).abs()
            bound_p = 8 * U * (p0.abs() + grp['lr'] * (g.abs() + (grp['weight_decay'] * p0).abs() + mom * mag))
            assert bool(((named[n].detach().cpu().double() - q.detach()).abs() <= bound_p).all()), (step, n)
            eb = (opt.state[named[n]]['momentum_buffer'].detach().cpu().double() - ref.state[q]['momentum_buffer']).abs()
            assert bool((eb <= 8 * U * mag).all()), (step, n)


def test_eval_after_a_table_step_sees_the_new_weights(backend):
    """the fp32 evaluation executor caches repacked weights; the table step writes them through raw pointers and must bump the
    parameter epoch as SGD.step does (tests/test_emu_train_step.py:test_eval_after_training_sees_current_weights)"""
    dev = backend.dev
    model, opt, _ = _build(dev, dict(type='SGD', lr=0.5, momentum=0.9, weight_decay=1e-4, paramwise_cfg=PARAMWISE))
    from oracle import vfs_oracle as O
    frame = O.fill_tensor([1, 3, 32, 32], seed=12, scale=2.0).to(dev)

    def evaluate(fresh):
        model.eval()
        if fresh:
            model.backbone._exact_state = None
        with torch.no_grad():
            y = model.backbone(frame).cpu().clone()
        model.train()
        return y
    y1 = evaluate(False)
    _set_grads(model, 60, dev)
    assert _counted_step(backend, opt) == ['opt_step_table']
    y2 = evaluate(False)
    assert torch.equal(y2, evaluate(True)) and not torch.equal(y1, y2)


# ---------------------------------------------------------------------------------------------- 7. the default stays
@pytest.mark.parametrize('optimizer_config,want', [(None, ['sgd_step']), (dict(grad_clip=dict(max_norm=1e-3)), ['grad_norm_partial', 'grad_norm_finish', 'sgd_step_clip'])])
def test_shipped_config_keeps_the_single_group_launches(backend, optimizer_config, want):
    import vfs_amd
    model, _, cfg = shallow_r18(backend.dev)
    opt = vfs_amd.build_optimizer(model, cfg.optimizer, optimizer_config=optimizer_config)
    assert type(opt) is vfs_amd.SGD and len(opt.param_groups) == 1
    _set_grads(model, 70, backend.dev)
    assert _counted_step(backend, opt) == want
    opt.param_groups[0]['lr'] = 0.01      # one group, edited: still one group
    assert _counted_step(backend, opt) == want


def test_clipped_table_step_uses_the_device_coefficient(backend):
    """grad_clip with param groups: reduction, finish, one table launch; last_grad_norm() is the norm of the trainable gradients"""
    dev = backend.dev
    model, opt, _ = _build(dev, dict(type='SGD', lr=0.05, momentum=0.9, weight_decay=1e-4, paramwise_cfg=PARAMWISE), dict(grad_clip=dict(max_norm=1e-3)))
    grads = _set_grads(model, 80, dev)
    before = _snapshot(model)
    assert _counted_step(backend, opt) == ['grad_norm_partial', 'grad_norm_finish', 'opt_step_table']
    N = float(torch.cat([g.double().reshape(-1) for g in grads.values()]).norm())
    assert abs(opt.last_grad_norm() - N) <= 1e-6 * N
    c = 1e-3 / (N + 1e-6)
    for (n, p), grp in zip(model.named_parameters(), opt.param_groups):
        p0, g = before[n].double(), grads[n].double() * c
        lr, wd = float(np.float32(grp['lr'])), float(np.float32(grp['weight_decay']))
        ref = p0 - lr * (g + wd * p0)
        bound = U * (8 * (p0.abs() + lr * (g.abs() + (wd * p0).abs())) + 2 * lr * g.abs())
        assert bool(((p.detach().cpu().double() - ref).abs() <= bound).all()), n
