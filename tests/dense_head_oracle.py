"""CPU restatement of DenseSimSiamHead and of the tracker around it, with the bf16-storage emulation of oracle/vfs_oracle.py:
test infrastructure for tests/test_dense_head.py.  fp32 mode is pinned against tests/golden/dense_head.npz (captured from the
reference class); emulate_bf16 rounds at the points the HIP path stores bf16 (packed weights, conv outputs, activations and
their gradients)."""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import vfs_oracle as O


class Conv1x1(nn.Module):
    """mmcv ConvModule for a 1x1 conv: conv (bias only without a norm) -> bn -> relu; sub-module names conv / bn"""

    def __init__(self, cin, cout, bn, relu):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 1, bias=not bn)
        if bn:
            self.bn = nn.BatchNorm2d(cout)
        self.has_bn, self.relu, self.emulate_bf16 = bn, relu, False

    def forward(self, x):
        e = self.emulate_bf16
        y = O._act_round(F.conv2d(x, O._w_round(self.conv.weight, e), self.conv.bias), e)
        if not self.has_bn:
            return y
        y = self.bn(y)
        return O._act_round(F.relu(y) if self.relu else y, e)


class DenseHead(nn.Module):
    def __init__(self, in_channels, num_projection_convs=3, projection_mid_channels=2048, projection_out_channels=2048,
                 num_predictor_convs=2, predictor_mid_channels=512, predictor_out_channels=2048):
        super().__init__()
        last, proj, pred = in_channels, [], []
        for i in range(num_projection_convs):
            is_last = i == num_projection_convs - 1
            out = projection_out_channels if is_last else projection_mid_channels
            proj.append(Conv1x1(last, out, True, not is_last))
            last = out
        for i in range(num_predictor_convs):
            is_last = i == num_predictor_convs - 1
            out = predictor_out_channels if is_last else predictor_mid_channels
            pred.append(Conv1x1(last, out, not is_last, not is_last))
            last = out
        self.projection_convs, self.predictor_convs = nn.Sequential(*proj), nn.Sequential(*pred)

    def set_emulate_bf16(self, on=True):
        for m in self.modules():
            if hasattr(m, 'emulate_bf16'):
                m.emulate_bf16 = on
        return self

    def forward(self, x):
        z = self.projection_convs(x)
        return z, self.predictor_convs(z)

    @staticmethod
    def loss(p1, z1, p2, z2, weight=1.0, **kw):
        """symmetric, stop-gradient on z; the cosine similarity per position, averaged over the positions"""
        half = lambda p, z: O.cosine_sim_loss_general(p, z.detach(), **kw)      # noqa: E731
        return (half(p1, z2) * 0.5 + half(p2, z1) * 0.5) * weight


class DenseTracker(O.SimSiamTracker):
    """O.SimSiamTracker with the dense head: the same roll loop over [N,C,h,w] maps"""

    def __init__(self, depth, head_kwargs, intra_video=False, **backbone_kwargs):
        super().__init__(depth, dict(in_channels=head_kwargs['in_channels']), intra_video, **backbone_kwargs)
        self.img_head = DenseHead(**head_kwargs)

    def forward_img_head(self, x1, x2, clip_len):
        losses = OrderedDict()
        z1, p1 = self.img_head(x1)
        z2, p2 = self.img_head(x2)
        w = 1.0 / clip_len if self.intra_video else 1.0
        losses['0.loss_feat'] = DenseHead.loss(p1, z1, p2, z2, w)
        if self.intra_video:
            z2v, p2v = O.images2video(z2, clip_len), O.images2video(p2, clip_len)
            for i in range(1, clip_len):
                losses[f'{i}.loss_feat'] = DenseHead.loss(p1, z1, O.video2images(p2v.roll(i, dims=2)),
                                                          O.video2images(z2v.roll(i, dims=2)), w)
        return losses
