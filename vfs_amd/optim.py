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
so the reduction may sweep them."""
import math
import os

import torch

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


class SGD(torch.optim.Optimizer):
    def __init__(self, model, lr=0.05, momentum=0.9, weight_decay=1e-4, grad_clip=None):
        self.model = model
        params = [p for p in model.parameters() if p.requires_grad]
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))
        self._buf = None
        self._segments = None
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

    def zero_grad(self, set_to_none=False):
        f = self.model._ensure_arena()
        f['grads'].zero_()

    def _arena(self):
        """momentum arena + the contiguous arena ranges that hold trainable parameters"""
        f = self.model._ensure_arena()
        flat = f['params']
        if self._buf is None or self._buf.shape != flat.shape or self._buf.device != flat.device:
            old = {id(p): st.get('momentum_buffer') for p, st in self.state.items()}
            self._buf = torch.zeros_like(flat)
            self._segments = None
            for p, o in zip(f['plist'], f['offsets']):
                if not p.requires_grad:
                    continue
                view = self._buf[o:o + p.numel()].view(p.shape)
                prev = old.get(id(p))
                if prev is not None:              # a state restored before the arena existed
                    view.copy_(prev)
                self.state[p]['momentum_buffer'] = view
        key = tuple(p.requires_grad for p in f['plist'])
        if self._segments is None or self._segments[0] != key:
            self._segments = (key, _trainable_segments(f))
        return f, self._segments[1]

    @torch.no_grad()
    def step(self, closure=None):
        f, segs = self._arena()
        flat, g = f['params'], f['grads']
        grp = self.param_groups[0]
        eng = shared_engine()
        bump_params_epoch()      # raw-pointer update: caches derived from the parameters (vfs_amd/exact.py) must refresh
        # data parallel with the SyncBN window exchange: its error word gates the update on the device (a peer that never arrived
        # poisons the step's statistics with NaN; the host only learns of it when it reads the log values)
        x = eng._p2p
        skip = x.state[1:2] if x is not None and x.state.device == flat.device else None
        clip = self._clip_coefficient(eng, g, segs) if self.grad_clip is not None and segs else None
        for lo, hi in segs:
            if clip is None:
                eng.timed('sgd', (0.0, 20.0 * (hi - lo)), flat.device, eng.lib.sgd_step, flat[lo:hi], g[lo:hi], self._buf[lo:hi], hi - lo,
                          float(grp['lr']), float(grp['momentum']), float(grp['weight_decay']), skip, eng.stream(flat.device))
            else:
                eng.timed('sgd', (0.0, 20.0 * (hi - lo)), flat.device, eng.lib.sgd_step_clip, flat[lo:hi], g[lo:hi], self._buf[lo:hi], hi - lo,
                          float(grp['lr']), float(grp['momentum']), float(grp['weight_decay']), clip, skip, eng.stream(flat.device))
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

    def _watch_exchange(self, x, every=int(os.environ.get('VFS_P2P_CHECK_EVERY', '50'))):
        """the error word of the SyncBN window exchange is sticky: once set, every later update is skipped on every rank (the word is
        MAX-reduced over the ranks, trackers.py).  A consumer that never reads the log values would then train as a silent no-op
        (advisor r05): every `every` steps a copy of the word is queued to pinned memory and the copy queued `every` steps earlier -
        long complete, no stall - is looked at; a set word raises here, at most 2 x `every` steps after the failed exchange."""
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
        """torch's loader replaces the state tensors by copies: put them back into the momentum arena"""
        super().load_state_dict(state_dict)
        loaded = {id(p): st.get('momentum_buffer') for p, st in self.state.items()}
        self._buf = None
        f, _ = self._arena()
        for p in f['plist']:
            buf = loaded.get(id(p))
            if buf is not None and p.requires_grad:
                self.state[p]['momentum_buffer'].copy_(buf)


def build_optimizer(model, cfg, optimizer_config=None):
    """mmcv build_optimizer for the shipped `optimizer = dict(type='SGD', ...)`; `optimizer_config` is the config's dict of that
    name (configs/r*_*.py:136; apis/train.py:85-93 makes mmcv's OptimizerHook of it): `grad_clip=None` or absent leaves the
    optimizer as it is, `grad_clip=dict(max_norm=..., norm_type=2 | 'inf')` clips inside step()."""
    cfg = dict(cfg)
    t = cfg.pop('type')
    if t != 'SGD':
        raise KeyError(f'optimizer type {t} is not on the VFS path')
    oc = dict(optimizer_config or {})
    grad_clip = oc.pop('grad_clip', None)
    if oc:
        raise NotImplementedError(f'optimizer_config option {sorted(oc)[0]!r} is not on the VFS path (grad_clip)')
    return SGD(model, grad_clip=grad_clip, **cfg)
