"""Heads of the SiamFC linear probe (§8f rank 4; projects/siamfc-pytorch/siamfc/heads.py): `SiamFC` (:7-23, plain
cross-correlation) and `SiamConvFC` (:26-58, a 1x1 conv on exemplar and search features first), same constructor
arguments and state_dict names.  forward() is the inference side of a trained probe: the 1x1 convs run through
vfs_conv_fwd, the correlation through vfs_xcorr_fwd (csrc/xcorr.hip).  Each 1x1 conv also is an engine.ConvUnit with its
packed bf16 weights; training the probe (losses, backward through these units, optimizers) and the tracking loop are in
siamfc.py."""
import torch
import torch.nn as nn

from .engine import BF16, ConvUnit, params_epoch, shared_engine
from .packing import build_pack_table


def _nhwc_bf16(t):
    return t.permute(0, 2, 3, 1).contiguous().to(BF16)


def _xcorr(z, x, scale):
    """z, x: NHWC bf16 features -> fp32 [nx, 1, ho, wo]"""
    eng = shared_engine(x.device)
    nz, hz, wz, c = z.shape
    nx, h, w, c2 = x.shape
    assert c == c2 and nx % nz == 0, (z.shape, x.shape)
    out = torch.empty(nx, 1, h - hz + 1, w - wz + 1, device=x.device)
    eng.lib.xcorr_fwd(z, x, out, nz, nx, hz, wz, h, w, c, float(scale), eng.stream(x.device))
    return out


class SiamFC(nn.Module):
    def __init__(self, out_scale=0.001):
        super().__init__()
        self.out_scale = out_scale

    def forward(self, z, x):
        """z [nz,C,hz,wz], x [nx,C,h,w] (fp32 NCHW, as the backbone returns them) -> responses [nx,1,ho,wo]"""
        return _xcorr(_nhwc_bf16(z), _nhwc_bf16(x), self.out_scale)


class SiamConvFC(nn.Module):
    def __init__(self, in_channels, channels, num_convs=1, kernel_size=1, out_scale=0.001):
        super().__init__()
        if kernel_size != 1:
            raise NotImplementedError('SiamConvFC: the probe uses kernel_size=1 (siamfc_tracker_base.py:110-115)')
        self.out_scale = out_scale
        zc, xc, last = [], [], in_channels
        for _ in range(num_convs):
            zc.append(nn.Conv2d(last, channels, kernel_size))
            xc.append(nn.Conv2d(last, channels, kernel_size))
            last = channels
        self.z_convs, self.x_convs = nn.Sequential(*zc), nn.Sequential(*xc)
        # one engine unit per conv, NOT registered with the shared engine: Engine.pack_weights repacks every registered unit on
        # each call, and the tracking loop must not pay for the backbone per frame (_pack below packs these)
        self.z_units = [self._unit(f'siamfc_head.z_convs.{i}', c) for i, c in enumerate(zc)]
        self.x_units = [self._unit(f'siamfc_head.x_convs.{i}', c) for i, c in enumerate(xc)]

    @staticmethod
    def _unit(name, conv):
        u = ConvUnit(name, conv.weight, conv.bias, bn=None, k=1, stride=1, pad=0, kind='conv')
        u.need_wd = False      # until a backward asks for the dgrad packing
        u.packed = None        # (key, pack table) of the last _pack
        return u

    def _pack(self, u, need_wd=False):
        """u.wf [Cout][1][1][Cin] and, once a backward has asked for it, u.wd [Cin][1][1][Cout]: the bf16 copies of the unit's
        weight, one vfs_pack_weights launch.  Repeated when the weight changes (the probe's optimizers update it through raw
        pointers - no _version bump - hence the params epoch) and when wd is first asked for."""
        w = u.weight
        u.need_wd |= need_wd
        key = (w.data_ptr(), w._version, params_epoch())
        if u.packed is None or u.packed[0] != key or (u.need_wd and u.wd is None):
            eng = shared_engine(w.device)
            u.wf = torch.empty(u.cout, 1, 1, u.cin, dtype=BF16, device=w.device)
            u.wd = torch.empty(u.cin, 1, 1, u.cout, dtype=BF16, device=w.device) if u.need_wd else None
            tab = build_pack_table([(w.data, u.wf, u.wd, 0)], w.device)
            eng.lib.pack_weights(*tab, eng.stream(w.device))
            u.packed = (key, tab)

    def _conv1x1(self, u, t):
        """t NHWC bf16 -> conv(t) + bias of unit u, NHWC bf16 (vfs_conv_fwd on the packed u.wf, a fresh output tensor)"""
        eng = shared_engine(t.device)
        self._pack(u)
        n, h, w, c = t.shape
        if c != u.cin:      # the kernel takes C from the tensor: a mismatch would read past the packed weight
            raise ValueError(f'SiamConvFC: features with {c} channels for a conv with in_channels={u.cin} (cfg out_channels)')
        y = torch.empty(n, h, w, u.cout, dtype=BF16, device=t.device)
        eng.lib.conv_fwd(t, u.wf, y, u.bias.data if u.bias is not None else None, None, n, h, w, c, h, w, u.cout, 1, 1, 1, 0,
                         eng.stream(t.device))
        return y

    def forward(self, z, x):
        z, x = _nhwc_bf16(z), _nhwc_bf16(x)
        for uz, ux in zip(self.z_units, self.x_units):
            z, x = self._conv1x1(uz, z), self._conv1x1(ux, x)
        return _xcorr(z, x, self.out_scale)
