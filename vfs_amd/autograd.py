"""Module-level autograd on the HIP backward: ResNet.forward, SimSiamHead.forward and DenseSimSiamHead.forward in train mode are
torch.autograd.Functions, so that the reference's own loop - `x1 = backbone(imgs1); z1, p1 = head(x1); loss = ...;
loss.backward()` - trains (mmaction/models/trackers/sim_siam_base_tracker.py:31-56 written with module calls).

The boundary: the caller sees fp32 NCHW tensors, the engine works on bf16 NHWC buffers (csrc/layout.hip converts and joins).
Parameter gradients are ACCUMULATED into .grad through its pointer by the backward kernels, not returned (as in _TrainStepFn);
an anchor tensor gives the outputs their grad_fn.

Live contexts: every grad-mode forward takes a buffer tag, so that a later forward keeps its activations - and its BatchNorm
coefficients - apart from an earlier one's.  The engine's buffers are keyed by NAME ('backbone...', 'img_head...'), not by module
instance, so the pool belongs to the engine's buffer namespace: LIVE_LIMIT tags for all backbones on an engine, LIVE_LIMIT for all
heads - two instances of a class alive at once (two nets under one loss) draw different tags.  The tag goes back when the backward
has run or when the Function's context is collected.  The path is eager (no tape / graph replay) and single-process: with
collectives on (SyncBN, gradient all-reduce) it refuses; the tracker's fused step owns those."""
import weakref

import torch
import torch.nn as nn

from .engine import BF16, NCHWGrad, bump_params_epoch, shared_engine

LIVE_LIMIT = 4      # live grad-mode forwards per buffer namespace of an engine: two views x two modules is the reference's own pattern


def grad_mode(module):
    """does a forward of `module` take the autograd path?  train mode, gradients enabled, something to train"""
    return module.training and torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters())


def ensure_grads(params):
    """a zero .grad for every trainable parameter that has none (the kernels accumulate through the pointer); an existing
    gradient - a view into a tracker's flat arena - stays where it is"""
    for p in params:
        if p.requires_grad and p.grad is None:
            p.grad = torch.zeros_like(p)


def check_head_trainable(head):
    """SimSiamBaseTracker._check_trainable for a head on its own: a frozen or eval-mode head layer is refused by name"""
    who = type(head).__name__
    for name, m in head.named_modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm) and not m.training:
            raise NotImplementedError(f'{who}.{name}: BatchNorm in eval mode inside a training forward is not on the HIP training path')
    for name, p in head.named_parameters():
        if not p.requires_grad:
            raise NotImplementedError(f'{who}.{name}: requires_grad=False inside a training forward is not on the HIP training path')


def _refuse_collectives(eng, who):
    if eng.collectives_on:
        raise NotImplementedError(f'{who}: the module-level autograd path is single-process (no SyncBN exchange, no gradient '
                                  'all-reduce); data-parallel training runs through the tracker\'s train_step')
    if eng.tape is not None:
        raise NotImplementedError(f'{who}: the module-level autograd path is eager; it cannot be recorded onto a launch tape')


class _TagPool:
    def __init__(self, who):
        self.who = who
        self.free = [f'.live{i}' for i in range(LIVE_LIMIT - 1, -1, -1)]

    def take(self):
        if not self.free:
            raise RuntimeError(f"{LIVE_LIMIT} grad-mode forwards are alive in the engine's '{self.who}' buffers (the limit of the buffer-tag "
                               'pool, shared by every module of that kind); run their backward, or drop their outputs, before the next forward')
        return self.free.pop()

    def give(self, tag):
        self.free.append(tag)


def live_pool(eng, namespace):
    """the tag pool of one buffer namespace ('backbone' | 'img_head') of an engine"""
    pools = eng.__dict__.setdefault('_live_pools', {})
    if namespace not in pools:
        pools[namespace] = _TagPool(namespace)
    return pools[namespace]


class _Live:
    """one grad-mode forward: its tag, the engine context, and the per-unit state the backward kernels read through the unit
    (the BatchNorm batch coefficients) as this pass left it"""

    def __init__(self, eng, namespace, who):
        pool = live_pool(eng, namespace)
        self.who = who
        self.tag = pool.take()
        self.release = weakref.finalize(self, pool.give, self.tag)      # on collection; called by hand once the backward has run
        self.ctx = None
        self.units = []

    def keep_units(self, units):
        self.units = [(u, u.bnp) for u in units]

    def open_backward(self):
        if self.ctx is None:
            raise RuntimeError(f'{self.who}: trying to backward through the graph a second time: the activations of this forward were '
                               'released when its backward ran (the HIP path keeps no second copy; retain_graph does not apply)')
        for u, bnp in self.units:
            u.bnp = bnp
        ctx, self.ctx = self.ctx, None
        return ctx


def _anchor(module, dev):
    a = module.__dict__.get('_live_anchor')
    if a is None or a.device != dev:
        a = module.__dict__['_live_anchor'] = torch.zeros(1, device=dev, requires_grad=True)
    return a


def _to_nchw(eng, act, N, HW, C, shape):
    out = torch.empty(shape, dtype=torch.float32, device=act.device)
    eng.lib.nhwc_bf16_to_nchw_f32(act, out, N, HW, C, eng.stream(act.device))
    return out


# ---------------------------------------------------------------------------------------------------------------- ResNet
class _ResNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, net, x):
        ctx.set_materialize_grads(False)
        eng = shared_engine(x.device)
        _refuse_collectives(eng, 'ResNet.forward')
        live = _Live(eng, 'backbone', 'ResNet.forward')
        dev = x.device
        net.attach(eng)
        eng.pack_weights()
        N, _, H, W = x.shape
        Wp = W + (W & 1)
        x4 = eng.buf(f'backbone.x4{live.tag}', (N, H, Wp, 4), BF16, dev)
        eng.lib.imgs_to_nhwc4(x.contiguous().float(), x4, N, 1, 1, H, W, Wp, eng.stream(dev))
        bump_params_epoch()      # running statistics change through raw pointers
        outs, live.ctx = net.forward_nhwc(eng, x4, N, H, W, 1, True, stop_after_out=True, tag=live.tag)
        live.keep_units([m.unit for _, m in net.conv_modules()])
        ctx.live, ctx.net, ctx.stages, ctx.eng = live, net, sorted(outs), eng
        return tuple(_to_nchw(eng, outs[i][0], N, outs[i][1] * outs[i][2], outs[i][3], (N, outs[i][3], outs[i][1], outs[i][2])) for i in ctx.stages)

    @staticmethod
    def backward(ctx, *gs):
        net, live = ctx.net, ctx.live
        dev = next(net.parameters()).device
        eng = ctx.eng      # the engine whose buffers hold this pass
        _refuse_collectives(eng, 'ResNet.forward (backward)')
        nctx = live.open_backward()
        try:
            ensure_grads(net.parameters())
            grads = {si: NCHWGrad(g) for si, g in zip(ctx.stages, gs) if g is not None}      # a stage without a cotangent is skipped, not fed zeros
            if grads:
                net.backward_nhwc(eng, nctx, grads)
            eng.flush_wgrad(dev)
            eng.wgrad_join(dev)      # .grad is final on the caller's stream
        finally:
            live.release()
        return None, None, None


def resnet_forward(net, x):
    outs = _ResNetFn.apply(_anchor(net, x.device), net, x)
    return outs[0] if len(outs) == 1 else outs


# ---------------------------------------------------------------------------------------------------------------- heads
class _HeadFn(torch.autograd.Function):
    """SimSiamHead ([N, C, h, w] -> z, p [N, Cout]) and DenseSimSiamHead (-> z, p [N, Cout, h, w]); the input feature map may
    require grad, both outputs take cotangents"""

    @staticmethod
    def forward(ctx, anchor, head, x):
        ctx.set_materialize_grads(False)
        who = f'{type(head).__name__}.forward'
        eng = shared_engine(x.device)
        _refuse_collectives(eng, who)
        check_head_trainable(head)
        N, C, h, w = x.shape
        if C % 64:
            raise NotImplementedError(f'{who}: {C} input channels; the layout kernels of the autograd path take multiples of 64')
        head.attach(eng)
        for u in (head.units[head._n_proj - 1], head.units[-1]):      # z and p leave through the layout kernels
            if u.cout % 64:
                raise NotImplementedError(f'{who}: {u.name} has {u.cout} output channels; the layout kernels of the autograd path take '
                                          'multiples of 64')
        live = _Live(eng, 'img_head', who)
        dev = x.device
        eng.pack_weights()
        feat = eng.buf(f'img_head.feat{live.tag}', (N, h, w, C), BF16, dev)
        eng.lib.nchw_f32_to_nhwc_bf16(x.contiguous().float(), feat, N, h * w, C, eng.stream(dev))
        bump_params_epoch()
        z, p, live.ctx = head.forward_nhwc(eng, feat, N, h, w, C, 1, True, tag=live.tag)
        live.keep_units(head.units)
        ctx.live, ctx.head, ctx.eng = live, head, eng
        outs = []
        for a in (z, p):
            Co = a.shape[-1]
            dense = a.dim() == 4
            outs.append(_to_nchw(eng, a, N, h * w if dense else 1, Co, (N, Co, h, w) if dense else (N, Co)))
        return tuple(outs)

    @staticmethod
    def backward(ctx, gz, gp):
        head, live = ctx.head, ctx.live
        dev = next(head.parameters()).device
        eng = ctx.eng
        _refuse_collectives(eng, f'{type(head).__name__}.forward (backward)')
        hctx = live.open_backward()
        gx = None
        try:
            ensure_grads(head.parameters())
            if gz is not None or gp is not None:
                gfeat = head.backward_nhwc(eng, hctx, None if gp is None else NCHWGrad(gp), dz=None if gz is None else NCHWGrad(gz))
                if ctx.needs_input_grad[2]:
                    N, h, w, C = hctx['N'], hctx['h'], hctx['w'], hctx['C']
                    gx = _to_nchw(eng, gfeat, N, h * w, C, (N, C, h, w))
            eng.flush_wgrad(dev)
            eng.wgrad_join(dev)
        finally:
            live.release()
        return None, None, gx


def head_forward(head, x):
    return _HeadFn.apply(_anchor(head, x.device), head, x)
