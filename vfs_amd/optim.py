"""Fused SGD over the tracker's flat parameter arena (torch.optim.SGD semantics of configs/r*_*.py:134: lr, momentum,
weight_decay; dampening 0): one HIP launch per contiguous range of TRAINABLE parameters (one launch for the shipped
configs).  Parameters with requires_grad=False are never touched - the reference's optimizer does not hold them, so
they get neither weight decay nor momentum.  The momentum arena is exposed through `state[p]['momentum_buffer']`
(views), so `state_dict()` / `load_state_dict()` - what mmcv's checkpoint hook and `--resume-from` use - carry it.

Gradient clipping (`optimizer_config = dict(grad_clip=dict(max_norm=..., norm_type=2))`, configs/r*_*.py:136 -> mmcv
OptimizerHook.clip_grads -> torch.nn.utils.clip_grad_norm_, apis/train.py:85-93) runs on the same arena: one streaming reduction
per trainable range into fixed per-workgroup rows, a one-workgroup finish that leaves norm and coefficient in device memory, and
the update kernel multiplies the gradient by the coefficient it reads there.  Nothing of it passes through the host, so the step
stays free of synchronisation and of values baked into a recorded chain; `last_grad_norm()` (what OptimizerHook logs as
`grad_norm`) reads a pinned copy queued behind the step.  The padding words between parameters in the gradient arena are zero
(allocated zeroed; gradients are written through the per-parameter views, the bucket scaling and all-reduce keep zeros zero),
so the reduction may sweep them.

Param groups (mmcv's build_optimizer with `paramwise_cfg`, configs/r*_*.py:134, apis/train.py:72: one group per parameter with its
own lr and weight decay), nesterov momentum, Adam and AdamW take a second path: one call of vfs_opt_step_table - ONE update launch
over the whole arena, behind two small table-write launches when there are more than 224 groups.  A segment map on the
device (built once per arena layout) tells the kernel which 16-byte vectors are trainable and which group they belong to; the
groups' hyperparameters travel with every step as launch arguments, so `param_groups[i]['lr'] = ...` (an LR schedule,
`build_lr_updater`) holds from the next step on and nothing waits for a copy.  One group of plain SGD - every
shipped config - keeps the launches above."""
import inspect
import math

import torch

from . import knobs
from .engine import bump_params_epoch, shared_engine


def _trainable_segments(f):
    """the contiguous arena ranges [lo, hi) that hold trainable parameters (each parameter with its padding to 4 words)"""
    segs = []
    for p, o in zip(f['plist'], f['offsets']):
        if not p.requires_grad:
            continue
        end = o + (p.numel() + 3) // 4 * 4
        if segs and segs[-1][1] == o:
            segs[-1][1] = end
        else:
            segs.append([o, end])
    return segs


def _norm_type(norm_type):
    """2 or infinity as the float the C ABI takes; anything else is not on this path"""
    if isinstance(norm_type, str):
        if norm_type == 'inf':
            return math.inf
    elif isinstance(norm_type, (int, float)) and not isinstance(norm_type, bool) and (norm_type == 2 or norm_type == math.inf):
        return float(norm_type)
    raise NotImplementedError(f'grad_clip norm_type {norm_type!r} is not on the VFS path (2 or inf)')


def _grad_norm(eng, grads, segs, max_norm, norm_type, out):
    """total norm of the arena ranges `segs` -> out[0], torch's clip_coef_clamped -> out[1]: one reduction launch per range
    (the first overwrites the partial rows, the others accumulate) and the finish; all on the launch stream, no host read"""
    dev = grads.device
    if eng.grad_norm_rows is None:
        n = torch.zeros(1, dtype=torch.int32)
        eng.host_lib.grad_norm_rows(n)
        eng.grad_norm_rows = int(n)
    rows = eng.ws('grad_norm_rows', eng.grad_norm_rows, torch.float64, dev)
    st = eng.stream(dev)
    for i, (lo, hi) in enumerate(segs):
        eng.timed('grad_norm', (0.0, 4.0 * (hi - lo)), dev, eng.lib.grad_norm_partial, grads[lo:hi], hi - lo, norm_type, rows, int(i > 0), st)
    eng.lib.grad_norm_finish(rows, norm_type, float(max_norm), out, st)


def clip_grad_norm_(model, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_ for a model on the flat arena, for callers that drive the loop themselves: the gradients of
    the trainable parameters are scaled in place by min(1, max_norm / (norm + 1e-6)); returns the norm as a 0-d device tensor.
    Three small launch families on the arena (reduction, finish, scale), no synchronisation."""
    nt = _norm_type(norm_type)
    if not float(max_norm) > 0:
        raise ValueError(f'max_norm must be positive, got {max_norm!r}')
    f = model._ensure_arena()
    g, segs = f['grads'], _trainable_segments(f)
    out = torch.empty(2, dtype=torch.float32, device=g.device)
    if not segs:
        return out.zero_()[0]
    eng = shared_engine()
    _grad_norm(eng, g, segs, max_norm, nt, out)
    for lo, hi in segs:
        eng.lib.scale_by(g[lo:hi], hi - lo, out[1:2], eng.stream(g.device))
    return out[0]


_KINDS = dict(SGD=0, Adam=1, AdamW=2)      # vfs_opt_step_table's `kind`
_MAX_GROUPS = 448                          # VFS_OPT_MAX_GROUPS (csrc/opt_table.h)


def _torch_defaults(name, **kw):
    """the `defaults` of the same-named torch.optim class for these options: the param groups then carry every key torch's own
    step() reads, so a state_dict() loads into torch.optim.<name> and runs there; torch's argument checks (negative lr, nesterov
    without momentum, ...) come along"""
    return dict(getattr(torch.optim, name)([torch.zeros(1)], **kw).defaults)


class _ArenaOptimizer(torch.optim.Optimizer):
    """What SGD, Adam and AdamW on the flat arena share: the state arenas with their per-parameter views, the choice between the
    single-group launches and the table-driven one, gradient clipping, the SyncBN skip word."""
    _kind = 'SGD'
    _state_names = ('momentum_buffer',)

    def __init__(self, model, defaults, grad_clip=None, param_groups=None):
        self.model = model
        params = param_groups if param_groups is not None else [p for p in model.parameters() if p.requires_grad]
        super().__init__(params, defaults)
        if len(self.param_groups) > _MAX_GROUPS:
            raise ValueError(f'{len(self.param_groups)} param groups: the table-driven step holds at most {_MAX_GROUPS}')
        self._arenas = None        # state name -> arena with the layout of the parameter arena
        self._segments = None
        self._table = None         # (key, per-parameter segments, device map, device hyperparameter table, host hyperparameters)
        self._step = 0             # torch's state['step'] (Adam / AdamW), the same for every parameter
        self._steps = None
        self.grad_clip = None      # (max_norm, norm_type) or None
        if grad_clip is not None:
            gc = dict(grad_clip)
            if 'max_norm' not in gc:
                raise KeyError('grad_clip needs max_norm')
            max_norm, nt = float(gc.pop('max_norm')), _norm_type(gc.pop('norm_type', 2))
            if gc:
                raise NotImplementedError(f'grad_clip option {sorted(gc)[0]!r} is not on the VFS path (max_norm, norm_type)')
            if not max_norm > 0:
                raise ValueError(f'grad_clip max_norm must be positive, got {max_norm!r}')
            self.grad_clip = (max_norm, nt)
        self._norm_out = None
        self._norm_pending = None

    @property
    def _buf(self):
        """the first state arena (SGD: the momentum arena)"""
        return None if self._arenas is None else self._arenas[self._state_names[0]]

    def zero_grad(self, set_to_none=False):
        f = self.model._ensure_arena()
        f['grads'].zero_()

    def _arena(self):
        """state arenas + the contiguous arena ranges that hold trainable parameters"""
        f = self.model._ensure_arena()
        flat = f['params']
        if self._arenas is None or self._buf.shape != flat.shape or self._buf.device != flat.device:
            old = {id(p): dict(st) for p, st in self.state.items()}
            self._arenas = {name: torch.zeros_like(flat) for name in self._state_names}
            self._segments = self._table = None
            trainable = [(p, o) for p, o in zip(f['plist'], f['offsets']) if p.requires_grad]
            if self._kind != 'SGD':      # torch keeps `step` as a float32 scalar per parameter: views of one host vector
                self._steps = torch.full((len(trainable),), float(self._step))
            for i, (p, o) in enumerate(trainable):
                for name, arena in self._arenas.items():
                    view = arena[o:o + p.numel()].view(p.shape)
                    prev = old.get(id(p), {}).get(name)
                    if prev is not None:              # a state restored before the arena existed
                        view.copy_(prev)
                    self.state[p][name] = view
                if self._steps is not None:
                    self.state[p]['step'] = self._steps[i]
        key = tuple(p.requires_grad for p in f['plist'])
        if self._segments is None or self._segments[0] != key:
            self._segments = (key, _trainable_segments(f))
        return f, self._segments[1]

    def _group_values(self, grp):
        """one param group's row of the hyperparameter table (vfs_opt_step_table's `hyper`)"""
        if self._kind == 'SGD':
            return (float(grp['lr']), float(grp['weight_decay']), float(grp['momentum']))
        return (float(grp['lr']), float(grp['weight_decay']), float(grp['betas'][0]), float(grp['betas'][1]), float(grp['eps']))

    def _group_rows(self):
        """one pass over the param groups -> (their rows, nesterov); refuses the options the kernels do not take per group, or at all"""
        nesterov = self.param_groups[0].get('nesterov', False)
        values, rows = self._group_values, []
        for grp in self.param_groups:
            if grp.get('dampening', 0) != 0 or grp.get('maximize', False) or grp.get('amsgrad', False) or grp.get('nesterov', False) != nesterov:
                k = next(k for k, want in (('dampening', 0), ('maximize', False), ('amsgrad', False), ('nesterov', nesterov)) if grp.get(k, want) != want)
                raise NotImplementedError(f'param group option {k}={grp[k]!r} is not on the VFS path')
            rows.append(values(grp))
        return rows, bool(nesterov)

    def _device_table(self, eng, f):
        """segment map of the arena (one segment per trainable parameter, with its param group) on the device, the table workspace
        and the host rows; rebuilt when the requires_grad flags (the key _arena() keeps), the arena, the number of groups or the
        identity or length of a group's `params` list change - a fingerprint of one entry per group, not per parameter"""
        key = (self._segments[0], f['params'].data_ptr(), tuple([(id(grp['params']), len(grp['params'])) for grp in self.param_groups]))
        if self._table is None or self._table[0] != key:
            if len(self.param_groups) > _MAX_GROUPS:
                raise ValueError(f'{len(self.param_groups)} param groups: the table-driven step holds at most {_MAX_GROUPS}')
            # a trainable parameter that no group holds follows group 0, as it does on the single-group path
            owner = {id(p): gi for gi, grp in enumerate(self.param_groups) for p in grp['params']}
            segs = [(o, o + p.numel(), owner.get(id(p), 0)) for p, o in zip(f['plist'], f['offsets']) if p.requires_grad]
            n, dev = f['params'].numel(), f['params'].device
            words = torch.zeros(1, dtype=torch.int64)
            eng.host_lib.opt_segment_map_words(n, len(segs), words)
            host_map = torch.zeros(max(int(words), 4), dtype=torch.int32)
            seg_t = torch.tensor(segs, dtype=torch.int64).reshape(-1, 3) if segs else torch.zeros(1, 3, dtype=torch.int64)
            eng.host_lib.opt_segment_map(seg_t, len(segs), n, len(self.param_groups), host_map, host_map.numel())
            table = torch.zeros(len(self.param_groups) * 8, dtype=torch.float32, device=dev)
            self._table = (key, len(segs), host_map.to(dev), table, torch.zeros(len(self.param_groups), 8), sum(e - b for b, e, _ in segs))
        return self._table[1:]

    @torch.no_grad()
    def step(self, closure=None):
        f, segs = self._arena()
        flat, g = f['params'], f['grads']
        rows, nesterov = self._group_rows()
        eng = shared_engine()
        bump_params_epoch()      # raw-pointer update: caches derived from the parameters (vfs_amd/exact.py) must refresh
        # data parallel with the SyncBN window exchange: its error word gates the update on the device (a peer that never arrived
        # poisons the step's statistics with NaN; the host only learns of it when it reads the log values)
        x = eng._p2p
        skip = x.state[1:2] if x is not None and x.state.device == flat.device else None
        clip = self._clip_coefficient(eng, g, segs) if self.grad_clip is not None and segs else None
        st = eng.stream(flat.device)
        if self._kind == 'SGD' and not nesterov and all(r == rows[0] for r in rows):
            # every shipped config: one group of plain SGD, one launch per contiguous trainable range
            lr, wd, momentum = rows[0]
            for lo, hi in segs:
                if clip is None:
                    eng.timed('sgd', (0.0, 20.0 * (hi - lo)), flat.device, eng.lib.sgd_step, flat[lo:hi], g[lo:hi], self._buf[lo:hi], hi - lo,
                              lr, momentum, wd, skip, st)
                else:
                    eng.timed('sgd', (0.0, 20.0 * (hi - lo)), flat.device, eng.lib.sgd_step_clip, flat[lo:hi], g[lo:hi], self._buf[lo:hi], hi - lo,
                              lr, momentum, wd, clip, skip, st)
        elif segs:
            # param groups that differ, nesterov, Adam, AdamW: one update launch over the whole arena, the groups looked up in the kernel.
            # The step count is the host's: a step the device skips (the SyncBN error word) still counts, as it would in torch,
            # which knows nothing of the word - and the word is sticky, _watch_exchange ends such a run.
            nseg, dev_map, table, hyper, ntrain = self._device_table(eng, f)
            hyper.numpy()[:, :len(rows[0])] = rows      # in place: the slots behind stay zero
            self._step += 1
            if self._steps is not None:
                self._steps += 1
            s1 = self._arenas[self._state_names[0]]
            s2 = self._arenas[self._state_names[1]] if len(self._state_names) > 1 else None
            eng.timed('sgd', (0.0, (20.0 if s2 is None else 28.0) * ntrain), flat.device, eng.lib.opt_step_table, _KINDS[self._kind], flat, g, s1, s2,
                      flat.numel(), dev_map, nseg, hyper.data_ptr(), len(rows), table, int(nesterov), max(self._step, 1), clip, skip, st)
        if skip is not None:
            self._watch_exchange(x)

    def _clip_coefficient(self, eng, g, segs):
        """norm and coefficient of this step's gradients (already all-reduced: every rank computes the same bits, no collective of
        its own) into the optimizer's two device words; the norm also travels to pinned host memory behind the launches, as the
        log values of train_step do (trackers.LazyLogVars), for last_grad_norm()"""
        if self._norm_out is None or self._norm_out.device != g.device:
            self._norm_out = torch.zeros(2, dtype=torch.float32, device=g.device)
        out = self._norm_out
        _grad_norm(eng, g, segs, self.grad_clip[0], self.grad_clip[1], out)
        if out.is_cuda:
            host = torch.empty(1, dtype=torch.float32, pin_memory=True)
            host.copy_(out[0:1], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._norm_pending = (host, ev)
        else:
            self._norm_pending = (out[0:1].clone(), None)
        return out[1:2]

    def last_grad_norm(self):
        """total gradient norm of the last step() (before clipping; what mmcv's OptimizerHook logs as grad_norm) as a Python float,
        None without grad_clip or before the first step.  Waits - here, not in step() - only for the small copy queued behind it."""
        if self._norm_pending is None:
            return None
        host, ev = self._norm_pending
        if ev is not None:
            ev.synchronize()
        return float(host[0])

    def _watch_exchange(self, x):
        """the error word of the SyncBN window exchange is sticky: once set, every later update is skipped on every rank (the word is
        MAX-reduced over the ranks, trackers.py).  A consumer that never reads the log values would then train as a silent no-op
        (advisor r05): every `every` steps a copy of the word is queued to pinned memory and the copy queued `every` steps earlier -
        long complete, no stall - is looked at; a set word raises here, at most 2 x `every` steps after the failed exchange."""
        every = knobs.integer('VFS_P2P_CHECK_EVERY')
        self._xsteps = getattr(self, '_xsteps', 0) + 1
        if self._xsteps % every:
            return
        pend = getattr(self, '_xpending', None)
        if pend is not None:
            pend[1].synchronize()
            if int(pend[0][0]):
                raise RuntimeError('SyncBN P2P exchange: a peer did not arrive within the spin limit (VFS_P2P_SPIN) in an earlier step; every '
                                   'update since has been skipped on all ranks - stop, or restart from the last checkpoint')
        host = torch.empty(1, dtype=torch.int64, pin_memory=True)
        host.copy_(x.state[1:2], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._xpending = (host, ev)

    def load_state_dict(self, state_dict):
        """torch's loader replaces the state tensors by copies: put them back into the state arenas.  Adam / AdamW keep one step
        count for the whole arena (the bias corrections are per launch): a state whose parameters disagree on it is refused."""
        super().load_state_dict(state_dict)
        loaded = {id(p): dict(st) for p, st in self.state.items()}
        if self._kind != 'SGD':
            steps = {int(st['step']) for st in loaded.values() if 'step' in st}
            if len(steps) > 1:
                raise ValueError(f'the loaded state holds different step counts ({sorted(steps)[:4]} ...): one count per arena on the VFS path')
            self._step = steps.pop() if steps else 0
        self._arenas = None
        f, _ = self._arena()
        for p in f['plist']:
            st = loaded.get(id(p))
            if st is None or not p.requires_grad:
                continue
            for name in self._state_names:
                if st.get(name) is not None:
                    self.state[p][name].copy_(st[name])


class SGD(_ArenaOptimizer):
    """torch.optim.SGD (dampening 0) on the arena; `param_groups`: torch's list of group dicts instead of one group of every
    trainable parameter"""

    def __init__(self, model, lr=0.05, momentum=0.9, weight_decay=1e-4, grad_clip=None, nesterov=False, dampening=0, param_groups=None):
        if dampening != 0:
            raise NotImplementedError(f'dampening={dampening!r} is not on the VFS path (0)')
        super().__init__(model, _torch_defaults('SGD', lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov),
                         grad_clip=grad_clip, param_groups=param_groups)


class Adam(_ArenaOptimizer):
    """torch.optim.Adam (amsgrad off) on the arena: exp_avg and exp_avg_sq are arenas, one update launch per step"""
    _kind = 'Adam'
    _state_names = ('exp_avg', 'exp_avg_sq')

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, grad_clip=None, param_groups=None):
        if amsgrad:
            raise NotImplementedError('amsgrad=True is not on the VFS path')
        super().__init__(model, _torch_defaults(self._kind, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay),
                         grad_clip=grad_clip, param_groups=param_groups)


class AdamW(Adam):
    """torch.optim.AdamW: the weight decay scales the parameter (p *= 1 - lr wd) instead of joining the gradient"""
    _kind = 'AdamW'

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, grad_clip=None, param_groups=None):
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, grad_clip=grad_clip,
                         param_groups=param_groups)


_OPTIMIZERS = dict(SGD=(SGD, ('lr', 'momentum', 'weight_decay', 'nesterov', 'dampening')),
                   Adam=(Adam, ('lr', 'betas', 'eps', 'weight_decay', 'amsgrad')),
                   AdamW=(AdamW, ('lr', 'betas', 'eps', 'weight_decay', 'amsgrad')))
_PARAMWISE_KEYS = ('custom_keys', 'bias_lr_mult', 'bias_decay_mult', 'norm_decay_mult', 'dwconv_decay_mult', 'bypass_duplicate')


def _paramwise_groups(model, base_lr, base_wd, paramwise_cfg):
    """mmcv's DefaultOptimizerConstructor.add_params: one param group {params, lr, weight_decay} per trainable parameter, in
    model.named_parameters() order.  The first custom key (longest first) that is a substring of the parameter's full name decides
    alone; otherwise bias_lr_mult for the bias of a module that is no norm layer, and norm_decay_mult (BatchNorm modules) or
    bias_decay_mult (biases) on the weight decay.  dwconv_decay_mult and bypass_duplicate are accepted: no depth-wise convolutions
    and no shared parameters here."""
    cfg = dict(paramwise_cfg)
    for k in cfg:
        if k not in _PARAMWISE_KEYS:
            raise NotImplementedError(f'paramwise_cfg option {k!r} is not on the VFS path ({", ".join(_PARAMWISE_KEYS)})')
    custom = dict(cfg.get('custom_keys') or {})
    for k, v in custom.items():
        extra = sorted(set(v) - {'lr_mult', 'decay_mult'})
        if extra:
            raise NotImplementedError(f'custom_keys[{k!r}] option {extra[0]!r} is not on the VFS path (lr_mult, decay_mult)')
    keys = sorted(custom, key=lambda k: (len(k), k), reverse=True)
    bias_lr, bias_wd, norm_wd = (float(cfg.get(k, 1.)) for k in ('bias_lr_mult', 'bias_decay_mult', 'norm_decay_mult'))
    owner = {}
    for m in model.modules():
        for pname, p in m.named_parameters(recurse=False):
            owner.setdefault(id(p), (m, pname))
    groups = []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        lr, wd = base_lr, base_wd
        hit = next((k for k in keys if k in name), None)
        if hit is not None:
            lr, wd = base_lr * custom[hit].get('lr_mult', 1.), base_wd * custom[hit].get('decay_mult', 1.)
        else:
            m, pname = owner[id(p)]
            is_norm = isinstance(m, torch.nn.modules.batchnorm._BatchNorm)
            if pname == 'bias' and not is_norm:
                lr = base_lr * bias_lr
            if is_norm:
                wd = base_wd * norm_wd
            elif pname == 'bias':
                wd = base_wd * bias_wd
        groups.append(dict(params=[p], lr=lr, weight_decay=wd))
    return groups


def build_optimizer(model, cfg, optimizer_config=None):
    """mmcv build_optimizer (apis/train.py:72) for `optimizer = dict(type='SGD' | 'Adam' | 'AdamW', ..., paramwise_cfg=...)`
    (configs/r*_*.py:134); `optimizer_config` is the config's dict of that name (configs/r*_*.py:136; apis/train.py:85-93 makes
    mmcv's OptimizerHook of it): `grad_clip=None` or absent leaves the optimizer as it is, `grad_clip=dict(max_norm=...,
    norm_type=2 | 'inf')` clips inside step()."""
    cfg = dict(cfg)
    t = cfg.pop('type')
    if t not in _OPTIMIZERS:
        raise KeyError(f'optimizer type {t} is not on the VFS path')
    cls, known = _OPTIMIZERS[t]
    paramwise_cfg = cfg.pop('paramwise_cfg', None)
    for k in cfg:
        if k not in known:
            raise NotImplementedError(f'optimizer option {k!r} is not on the VFS path ({t}: {", ".join(known)})')
    oc = dict(optimizer_config or {})
    grad_clip = oc.pop('grad_clip', None)
    if oc:
        raise NotImplementedError(f'optimizer_config option {sorted(oc)[0]!r} is not on the VFS path (grad_clip)')
    groups = None
    if paramwise_cfg is not None:
        sig = inspect.signature(cls.__init__).parameters      # lr / weight_decay the config leaves out: the class's defaults
        groups = _paramwise_groups(model, cfg.get('lr', sig['lr'].default), cfg.get('weight_decay', sig['weight_decay'].default), paramwise_cfg)
        if len(groups) > _MAX_GROUPS:
            raise ValueError(f'paramwise_cfg gives {len(groups)} param groups: the table-driven step holds at most {_MAX_GROUPS}')
    return cls(model, grad_clip=grad_clip, param_groups=groups, **cfg)


class LrUpdater:
    """mmcv's LrUpdaterHook for `lr_config` (configs/r*_*.py:135): before_iter(it) sets every param group's lr from its
    `initial_lr`.  Host code only - the new values reach the device with the next step's launch arguments."""

    def __init__(self, optimizer, policy, max_iters, iters_per_epoch=None, by_epoch=True, warmup=None, warmup_iters=0, warmup_ratio=0.1,
                 min_lr=None, min_lr_ratio=None):
        if policy not in ('fixed', 'CosineAnnealing'):
            raise NotImplementedError(f'lr_config policy {policy!r} is not on the VFS path (fixed, CosineAnnealing)')
        if warmup not in (None, 'linear', 'constant', 'exp'):
            raise ValueError(f'warmup {warmup!r}: None, linear, constant or exp')
        if warmup is not None and not (warmup_iters > 0 and 0 < warmup_ratio <= 1.0):
            raise ValueError('warmup needs warmup_iters > 0 and 0 < warmup_ratio <= 1')
        if policy == 'CosineAnnealing' and (min_lr is None) == (min_lr_ratio is None):
            raise ValueError('CosineAnnealing takes exactly one of min_lr and min_lr_ratio')
        if by_epoch and policy != 'fixed' and not iters_per_epoch:
            raise ValueError('by_epoch=True needs iters_per_epoch')
        if not max_iters > 0:
            raise ValueError('max_iters must be positive')
        self.optimizer, self.policy, self.by_epoch = optimizer, policy, bool(by_epoch)
        self.max_iters, self.iters_per_epoch = int(max_iters), iters_per_epoch
        self.warmup, self.warmup_iters, self.warmup_ratio = warmup, int(warmup_iters), float(warmup_ratio)
        self.min_lr, self.min_lr_ratio = min_lr, min_lr_ratio
        for grp in optimizer.param_groups:      # a resumed state_dict brings its own initial_lr
            grp.setdefault('initial_lr', grp['lr'])

    def _regular(self, base, it):
        if self.policy == 'fixed':
            return base
        if self.by_epoch:
            progress, total = it // self.iters_per_epoch, -(-self.max_iters // self.iters_per_epoch)
        else:
            progress, total = it, self.max_iters
        target = self.min_lr if self.min_lr is not None else base * self.min_lr_ratio
        return target + 0.5 * (base - target) * (math.cos(math.pi * progress / total) + 1)

    def get_lr(self, base, it):
        lr = self._regular(base, it)
        if self.warmup is None or it >= self.warmup_iters:
            return lr
        if self.warmup == 'constant':
            return lr * self.warmup_ratio
        if self.warmup == 'linear':
            return lr * (1 - (1 - it / self.warmup_iters) * (1 - self.warmup_ratio))
        return lr * self.warmup_ratio ** (1 - it / self.warmup_iters)

    def before_iter(self, it):
        for grp in self.optimizer.param_groups:
            grp['lr'] = self.get_lr(grp.setdefault('initial_lr', grp['lr']), it)


def build_lr_updater(optimizer, lr_config, max_iters, iters_per_epoch=None):
    """the config's `lr_config = dict(policy='CosineAnnealing', min_lr=0, by_epoch=False)` -> LrUpdater"""
    cfg = dict(lr_config)
    if 'policy' not in cfg:
        raise KeyError('lr_config needs policy')
    known = ('policy', 'by_epoch', 'warmup', 'warmup_iters', 'warmup_ratio', 'min_lr', 'min_lr_ratio')
    for k in cfg:
        if k not in known:
            raise NotImplementedError(f'lr_config option {k!r} is not on the VFS path ({", ".join(known)})')
    return LrUpdater(optimizer, cfg.pop('policy'), max_iters, iters_per_epoch=iters_per_epoch, **cfg)
