"""SimSiamHead under the reference's registry name and constructor
(mmaction/models/heads/sim_siam_head.py:14-174): avg-pool -> projector
(Linear+BN[+ReLU]) x num_projection_fcs -> z; predictor Linear+BN+ReLU, Linear -> p.
Linear layers run on the same MFMA implicit-GEMM kernel as the convolutions (1x1 "images"),
BN1d on the shared BatchNorm kernels.

DenseSimSiamHead (sim_siam_head.py:177-284) is the per-position form: projector and predictor are 1x1 ConvModules over the
backbone's feature map (no pooling), the loss is the cosine similarity per spatial position (csrc/simloss_dense.hip)."""
import torch
import torch.nn as nn

from .builder import build_loss
from .engine import BF16, ConvUnit
from .registry import HEADS


def _norm1d(cfg, n):
    t = cfg.get('type', 'BN')
    if t not in ('BN', 'BN1d', 'SyncBN'):
        raise KeyError(f'unsupported norm type {t}')
    return nn.BatchNorm1d(n, eps=cfg.get('eps', 1e-5))


@HEADS.register_module()
class SimSiamHead(nn.Module):
    def __init__(self, in_channels, conv_mid_channels=2048, conv_out_channles=2048, num_convs=0, kernel_size=1,
                 conv_cfg=dict(type='Conv2d'), norm_cfg=dict(type='BN'), act_cfg=None, drop_layer_cfg=None,
                 order=('pool', 'drop'), num_projection_fcs=3, projection_mid_channels=2048,
                 projection_out_channels=2048, drop_projection_fc=False, num_predictor_fcs=2,
                 predictor_mid_channels=512, predictor_out_channels=2048, drop_predictor_fc=False, with_norm=True,
                 loss_feat=dict(type='CosineSimLoss', negative=False), spatial_type='avg'):
        super().__init__()
        if num_convs != 0 or drop_layer_cfg is not None or drop_projection_fc or drop_predictor_fc \
                or spatial_type != 'avg':
            raise NotImplementedError('HIP path covers the shipped configs: no convs/dropout, spatial_type avg')
        assert set(order) == {'pool', 'drop'}
        self.in_channels, self.norm_cfg, self.with_norm = in_channels, norm_cfg, with_norm
        self.loss_feat = build_loss(loss_feat)
        self.spatial_type, self.order = spatial_type, order
        last = in_channels
        proj, self._plan = [], []          # plan: (seq name, linear idx, bn idx or None, relu)
        for i in range(num_projection_fcs):
            is_last = i == num_projection_fcs - 1
            out = projection_out_channels if is_last else projection_mid_channels
            self._plan.append(('projection_fcs', len(proj), len(proj) + 1, not is_last))
            proj += [nn.Linear(last, out), _norm1d(norm_cfg, out)]
            if not is_last:
                proj.append(nn.ReLU())
            last = out
        self.projection_fcs = nn.Sequential(*proj) if proj else nn.Identity()
        self._n_proj = num_projection_fcs
        pred = []
        for i in range(num_predictor_fcs):
            is_last = i == num_predictor_fcs - 1
            out = predictor_out_channels if is_last else predictor_mid_channels
            if is_last:
                self._plan.append(('predictor_fcs', len(pred), None, False))
                pred.append(nn.Linear(last, out))
            else:
                self._plan.append(('predictor_fcs', len(pred), len(pred) + 1, True))
                pred += [nn.Linear(last, out), _norm1d(norm_cfg, out), nn.ReLU()]
            last = out
        self.predictor_fcs = nn.Sequential(*pred) if pred else nn.Identity()
        self.avg_pool = nn.AdaptiveAvgPool2d((1, 1))
        self.units = None
        self._engine = None
        from .engine import flush_counters_hook
        self.register_state_dict_pre_hook(flush_counters_hook)

    def init_weights(self):
        pass  # the reference keeps torch's Linear defaults (sim_siam_head.py:127-129)

    def attach(self, engine, prefix='img_head'):
        if self._engine is engine and self.units is not None:
            return
        self.units = []
        for seq, li, bi, relu in self._plan:
            lin = getattr(self, seq)[li]
            bn = getattr(self, seq)[bi] if bi is not None else None
            u = ConvUnit(f'{prefix}.{seq}.{li}', lin.weight, lin.bias, bn, 1, 1, 0, 'linear')
            u.relu = relu
            self.units.append(engine.register(u))
        self._engine = engine

    # ------------------------------------------------------------------ HIP execution
    def forward_nhwc(self, eng, feat, N, h, w, C, G, train, tag=''):
        """feat bf16 [N,h,w,C] (G views stacked) -> z, p bf16 [N,Cout] + ctx.  tag: buffer namespace of the pass (a second
        context alive at the same time keeps its own activations, ResNet.forward_nhwc)."""
        dev = feat.device
        s = eng.stream(dev)
        x = eng.buf(f'img_head.pooled{tag}', (N, C), BF16, dev)
        eng.lib.avgpool_fwd(feat, x, N, h * w, C, s)
        ctx = dict(N=N, G=G, h=h, w=w, C=C, ins=[], raws=[], acts=[], tag=tag)
        a = x
        z = None
        for ui, u in enumerate(self.units):
            tr = train and (u.bn.training if u.bn is not None else True)
            ctx['ins'].append(a)
            raw, _, _, fin = eng.conv_fwd(u, a.view(N, 1, 1, u.cin), N, 1, 1, G, tr, tag=tag, defer_fin=u.bn is not None)
            raw = raw.view(N, u.cout)
            ctx['raws'].append(raw)
            if u.bn is not None:
                a = eng.bn_act(u, raw, N, G, tr, u.relu, fin, tag=tag)
            else:
                a = raw
            ctx['acts'].append(a)
            if ui == self._n_proj - 1:
                z = a
        return z, a, ctx

    def backward_nhwc(self, eng, ctx, dp, dz=None):
        """dp / dz: gradients wrt p / z - bf16 [N,C] or engine.NCHWGrad(fp32 [N,C]), either may be None.  In the SimSiam loss z is
        detached and only feeds the predictor (dz=None); a dz joins the predictor's gradient at the projector's output
        (Engine.grad_join: one launch, one rounding)."""
        N, G, tag = ctx['N'], ctx['G'], ctx.get('tag', '')
        dev = ctx['raws'][0].device
        g = None
        for ui in range(len(self.units) - 1, -1, -1):
            u = self.units[ui]
            if ui == len(self.units) - 1 and dp is not None:
                g = eng.grad_join(None, dp, f'img_head.dp_in{tag}', N, 1, u.cout).view(N, u.cout)
            if ui == self._n_proj - 1 and dz is not None:
                g = eng.grad_join(g, dz, f'img_head.dz_join{tag}', N, 1, u.cout).view(N, u.cout)
            if g is None:
                continue      # no gradient wrt p: the predictor's layers get none
            if u.bn is not None:
                dx, _ = eng.bn_bwd(u, g, None, ctx['raws'][ui], N, G, relu=u.relu, tag=tag)
            else:
                dx = g
            g, _ = eng.conv_bwd(u, dx, ctx['ins'][ui], N, 1, 1, 1, 1, need_dgrad=True, tag=tag)
            g = g.view(N, u.cin)
        gfeat = eng.buf(f'img_head.gfeat{tag}', (N, ctx['h'], ctx['w'], ctx['C']), BF16, dev)
        eng.lib.avgpool_bwd(g, gfeat, N, ctx['h'] * ctx['w'], ctx['C'], eng.stream(dev))
        return gfeat

    def loss_fwd_nhwc(self, eng, p, z, loss, Nv, T, K, weight):
        """the fused step's loss rows [K][Nv] from the two views stacked in p, z [2 Nv, C] (sim_siam_base_tracker.py:39-55)"""
        eng.lib.cosine_loss_fwd(p[:Nv], z[:Nv], p[Nv:], z[Nv:], loss, Nv, p.shape[1], T, K, int(self.loss_feat.negative), weight,
                                eng.stream(p.device))

    def loss_bwd_nhwc(self, eng, p, z, gl, dp, Nv, T, K, weight):
        eng.lib.cosine_loss_bwd(p[:Nv], z[:Nv], p[Nv:], z[Nv:], gl, dp[:Nv], dp[Nv:], Nv, p.shape[1], T, K,
                                int(self.loss_feat.negative), weight, eng.stream(p.device))

    # ------------------------------------------------------------------ reference-compatible API
    def forward(self, x):
        """x [N,C,h,w] fp32 -> (z, p) fp32 (sim_siam_head.py:143-163).  Train mode with gradients enabled: z and p carry a grad_fn
        and x may require grad (vfs_amd/autograd.py); otherwise the inference entry point."""
        from . import autograd
        from .engine import shared_engine
        if autograd.grad_mode(self):
            return autograd.head_forward(self, x)
        if x.requires_grad:
            raise RuntimeError('SimSiamHead.forward is the inference entry point; training runs in the tracker')
        eng = shared_engine()
        self.attach(eng)
        eng.pack_weights()
        N, C, h, w = x.shape
        feat = x.permute(0, 2, 3, 1).contiguous().to(BF16)
        z, p, _ = self.forward_nhwc(eng, feat, N, h, w, C, 1, self.training)
        return z.float(), p.float()

    def loss(self, p1, z1, p2, z2, mask12=None, mask21=None, weight=1.):
        assert mask12 is None and mask21 is None
        loss_feat = self.loss_feat(p1, z2.detach()) * 0.5 + self.loss_feat(p2, z1.detach()) * 0.5
        return dict(loss_feat=loss_feat * weight)


def _norm2d(cfg, n):
    t = cfg.get('type', 'BN')
    if t not in ('BN', 'BN1d', 'BN2d', 'SyncBN'):
        raise KeyError(f'unsupported norm type {t}')
    return nn.BatchNorm2d(n, eps=cfg.get('eps', 1e-5))


class _ConvModule(nn.Module):
    """Parameter container with mmcv ConvModule's sub-module names (conv, bn, activate) for a 1x1 convolution; bias='auto': a
    bias only where there is no norm.  Initialised as ConvModule.init_weights does (kaiming normal, fan_out, relu; BN 1 / 0)."""

    def __init__(self, cin, cout, norm_cfg, relu):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 1, bias=norm_cfg is None)
        nn.init.kaiming_normal_(self.conv.weight, a=0, mode='fan_out', nonlinearity='relu')
        if self.conv.bias is not None:
            nn.init.constant_(self.conv.bias, 0)
        if norm_cfg is not None:
            self.bn = _norm2d(norm_cfg, cout)
        if relu:
            self.activate = nn.ReLU(inplace=True)
        self.relu = relu

    @property
    def norm(self):
        return getattr(self, 'bn', None)

    def forward(self, x):
        raise RuntimeError('a parameter container; run it through vfs_amd.engine')


@HEADS.register_module()
class DenseSimSiamHead(nn.Module):
    """sim_siam_head.py:177-284: conv -> BN [-> ReLU] x num_projection_convs -> z; predictor conv + BN + ReLU, conv -> p, all
    1x1 over [N,h,w,C] maps on the implicit-GEMM and BatchNorm kernels of the backbone's 1x1 layers.

    Channel counts: the head builds (parameters, state_dict, `loss`) with any, but RUNS on the HIP path only where in_channels and
    every layer's output channels are multiples of 64 - what the 1x1 convolution kernels (forward, dgrad, weight gradient) take;
    the reference's defaults (2048 / 512) and configs/vfs_r18_dense.py are.  `attach` refuses other counts by name."""

    def __init__(self, in_channels, kernel_size=1, conv_cfg=dict(type='Conv2d'), norm_cfg=dict(type='BN'),
                 act_cfg=dict(type='ReLU'), num_projection_convs=3, projection_mid_channels=2048,
                 projection_out_channels=2048, num_predictor_convs=2, predictor_mid_channels=512,
                 predictor_out_channels=2048, predictor_plugin=None, loss_feat=dict(type='CosineSimLoss', negative=False)):
        super().__init__()
        if kernel_size != 1:
            raise NotImplementedError(f'kernel_size={kernel_size}: the HIP path of DenseSimSiamHead covers kernel_size=1')
        if predictor_plugin is not None:
            raise NotImplementedError('predictor_plugin is not on the HIP path of DenseSimSiamHead')
        if conv_cfg is not None and conv_cfg.get('type') not in ('Conv2d', 'Conv'):
            raise NotImplementedError(f'conv_cfg={conv_cfg}: the HIP path of DenseSimSiamHead covers Conv2d')
        if act_cfg is None or act_cfg.get('type') != 'ReLU':
            raise NotImplementedError(f'act_cfg={act_cfg}: the HIP path of DenseSimSiamHead covers ReLU')
        self.in_channels, self.conv_cfg, self.norm_cfg, self.act_cfg = in_channels, conv_cfg, norm_cfg, act_cfg
        self.loss_feat = build_loss(loss_feat)
        last = in_channels
        proj = []
        for i in range(num_projection_convs):
            is_last = i == num_projection_convs - 1
            out = projection_out_channels if is_last else projection_mid_channels
            proj.append(_ConvModule(last, out, norm_cfg, relu=not is_last))      # no relu on the output
            last = out
        self.projection_convs = nn.Sequential(*proj) if proj else nn.Identity()
        pred = []
        for i in range(num_predictor_convs):
            is_last = i == num_predictor_convs - 1
            out = predictor_out_channels if is_last else predictor_mid_channels
            pred.append(_ConvModule(last, out, None if is_last else norm_cfg, relu=not is_last))      # no bn / relu on the output
            last = out
        # (the reference tests len(projection_convs) here as well, sim_siam_head.py:249)
        self.predictor_convs = nn.Sequential(*pred) if proj else nn.Identity()
        self.predictor_plugin = nn.Identity()
        self._layers = proj + (pred if proj else [])
        self._names = [f'projection_convs.{i}' for i in range(len(proj))] + [f'predictor_convs.{i}' for i in range(len(pred) if proj else 0)]
        self._n_proj = len(proj)
        self.units = None
        self._engine = None
        self._loss_ws_bytes = {}      # (Nv, S, C, K) -> vfs_dense_cosine_loss_workspace_bytes
        from .engine import flush_counters_hook
        self.register_state_dict_pre_hook(flush_counters_hook)

    def init_weights(self):
        pass  # sim_siam_head.py:258-260: the ConvModules keep their constructor's initialisation

    def attach(self, engine, prefix='img_head'):
        if self._engine is engine and self.units is not None:
            return
        if not self._layers:
            raise NotImplementedError('DenseSimSiamHead without projection convs has nothing to run on the HIP path')
        for name, m in zip(self._names, self._layers):
            if m.conv.in_channels % 64 or m.conv.out_channels % 64:
                raise NotImplementedError(f'{prefix}.{name}: {m.conv.in_channels} -> {m.conv.out_channels} channels; the 1x1 convolution '
                                          'kernels (forward, dgrad, weight gradient) take multiples of 64')
        self.units = []
        for name, m in zip(self._names, self._layers):
            u = ConvUnit(f'{prefix}.{name}', m.conv.weight, m.conv.bias, m.norm, 1, 1, 0, 'conv')
            u.relu = m.relu
            self.units.append(engine.register(u))
        self._engine = engine

    # ------------------------------------------------------------------ HIP execution
    def forward_nhwc(self, eng, feat, N, h, w, C, G, train, tag=''):
        """feat bf16 [N,h,w,C] (G views stacked, each its own BatchNorm batch) -> z, p bf16 [N,h,w,Cout] + ctx.  tag: buffer
        namespace of the pass (SimSiamHead.forward_nhwc)."""
        M = N * h * w
        ctx = dict(N=N, G=G, h=h, w=w, C=C, ins=[], raws=[], acts=[], tag=tag)
        a, z = feat, None
        for ui, u in enumerate(self.units):
            tr = train and (u.bn.training if u.bn is not None else True)
            ctx['ins'].append(a)
            raw, _, _, fin = eng.conv_fwd(u, a, N, h, w, G, tr, tag=tag, defer_fin=u.bn is not None)
            ctx['raws'].append(raw)
            a = eng.bn_act(u, raw, M, G, tr, u.relu, fin, tag=tag) if u.bn is not None else raw
            ctx['acts'].append(a)
            if ui == self._n_proj - 1:
                z = a
        return z, a, ctx

    def backward_nhwc(self, eng, ctx, dp, dz=None):
        """dp / dz: gradients wrt p / z - bf16 [N,h,w,C] or engine.NCHWGrad(fp32 [N,C,h,w]), either may be None (z is detached in
        the loss: dz=None; a dz joins the predictor's gradient at the projector's output, Engine.grad_join) -> gradient wrt the
        feature map [N,h,w,C]."""
        N, G, h, w, tag = ctx['N'], ctx['G'], ctx['h'], ctx['w'], ctx.get('tag', '')
        M = N * h * w
        g, rows = None, None
        for ui in range(len(self.units) - 1, -1, -1):
            u = self.units[ui]
            if ui == len(self.units) - 1 and dp is not None:
                g = eng.grad_join(None, dp, f'img_head.dp_in{tag}', N, h * w, u.cout).view(N, h, w, u.cout)
            if ui == self._n_proj - 1 and dz is not None:
                g = eng.grad_join(g, dz, f'img_head.dz_join{tag}', N, h * w, u.cout).view(N, h, w, u.cout)
                rows = None      # statistics rows the dgrad emitted describe the gradient before the join
            if g is None:
                continue      # no gradient wrt p: the predictor's layers get none
            if u.bn is not None:
                g, _ = eng.bn_bwd(u, g, None, ctx['raws'][ui], M, G, relu=u.relu, rows=rows, tag=tag)
            # the dgrad also emits the BatchNorm-backward statistics of the layer in front (Engine.conv_bwd)
            prev = self.units[ui - 1] if ui > 0 else None
            bn_next = (prev, ctx['raws'][ui - 1], None, prev.relu, G if prev.bn.training else 1) if prev is not None and prev.bn is not None else None
            g, rows = eng.conv_bwd(u, g, ctx['ins'][ui], N, h, w, h, w, need_dgrad=True, bn_next=bn_next, tag=tag)
        return g

    def _check_fused_loss(self):
        lf = self.loss_feat
        if type(lf).__name__ != 'CosineSimLoss' or lf.pairwise or not lf.with_norm:
            raise NotImplementedError('the fused train step of DenseSimSiamHead covers loss_feat = CosineSimLoss(with_norm=True, '
                                      f'pairwise=False); got {type(lf).__name__}(with_norm={getattr(lf, "with_norm", None)}, '
                                      f'pairwise={getattr(lf, "pairwise", None)}) - DenseSimSiamHead.loss serves it outside the fused step')

    def loss_fwd_nhwc(self, eng, p, z, loss, Nv, T, K, weight):
        """the fused step's loss rows [K][Nv] from the two views stacked in p, z [2 Nv, h, w, C]: the cosine similarity per
        position, averaged over the positions (sim_siam_head.py:277-284 inside sim_siam_base_tracker.py:39-55)"""
        self._check_fused_loss()
        dev = p.device
        S, C = p.shape[1] * p.shape[2], p.shape[3]
        nbytes = self._loss_ws_bytes.get((Nv, S, C, K))
        if nbytes is None:      # host-only size query, once per shape: not a launch of the chain
            out = torch.zeros(1, dtype=torch.int64)
            eng.host_lib.dense_cosine_loss_workspace_bytes(Nv, S, C, K, out)
            nbytes = self._loss_ws_bytes[(Nv, S, C, K)] = int(out)
        ws = eng.ws('ws.dense_loss', (nbytes + 3) // 4, torch.float32, dev)
        eng.lib.dense_cosine_loss_fwd(p[:Nv], z[:Nv], p[Nv:], z[Nv:], loss, ws, nbytes, Nv, S, C, T, K,
                                      int(self.loss_feat.negative), weight, eng.stream(dev))

    def loss_bwd_nhwc(self, eng, p, z, gl, dp, Nv, T, K, weight):
        S, C = p.shape[1] * p.shape[2], p.shape[3]
        eng.lib.dense_cosine_loss_bwd(p[:Nv], z[:Nv], p[Nv:], z[Nv:], gl, dp[:Nv], dp[Nv:], Nv, S, C, T, K,
                                      int(self.loss_feat.negative), weight, eng.stream(p.device))

    # ------------------------------------------------------------------ reference-compatible API
    def forward(self, x):
        """x [N,C,h,w] fp32 -> (z, p) [N,Cout,h,w] fp32 (sim_siam_head.py:262-275).  Train mode with gradients enabled: z and p
        carry a grad_fn and x may require grad (vfs_amd/autograd.py); otherwise the inference entry point."""
        from . import autograd
        from .engine import shared_engine
        if autograd.grad_mode(self):
            return autograd.head_forward(self, x)
        if x.requires_grad:
            raise RuntimeError('DenseSimSiamHead.forward is the inference entry point; training runs in the tracker')
        eng = shared_engine()
        self.attach(eng)
        eng.pack_weights()
        N, C, h, w = x.shape
        feat = x.permute(0, 2, 3, 1).contiguous().to(BF16)
        z, p, _ = self.forward_nhwc(eng, feat, N, h, w, C, 1, self.training)
        return z.float().permute(0, 3, 1, 2).contiguous(), p.float().permute(0, 3, 1, 2).contiguous()

    def loss(self, p1, z1, p2, z2, mask12=None, mask21=None, weight=1.):
        loss_feat = self.loss_feat(p1, z2.detach(), mask12) * 0.5 + self.loss_feat(p2, z1.detach(), mask21) * 0.5
        return dict(loss_feat=loss_feat * weight)
