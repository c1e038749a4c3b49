"""The SiamFC probe on a frozen or partly unfrozen VFS backbone (OTB-100 metric of the reference, README.md:87-90): the training and
tracking logic of `TrackerSiamFC` (projects/siamfc-pytorch/siamfc/siamfc_tracker_base.py:88-500) on the HIP kernels, without
its third-party scaffolding (got10k's Tracker base / dataset classes, cv2, torchvision).

  train_step   (:364-387)  frozen dilated backbone (eval) -> 1x1 convs -> cross-correlation -> Balanced / Focal loss ->
                           backward through the head (vfs_xcorr_bwd, Engine.conv_bwd of the 1x1 convs) -> Adam / SGD
                           frozen_stages < 4 (:131-144, the optimizer holds the backbone too): both branches through the bf16
                           training path, the backward continues through the 1x1 convs' input gradients into
                           ResNet.backward_nhwc (dilated layers: vfs_conv_dgrad_dilated / vfs_conv_wgrad_dilated)
  _create_labels (:456-500), current_lr (:349-362), the optimizer / scheduler choices of __init__ (:131-166)
  init / update / track (:199-347): the tracking loop.  Crops and the response up-sampling are cv2 calls in the reference
                           (ops.crop_and_resize -> image_utils.get_cropped_input, cv2.resize INTER_CUBIC); cv2 is absent in
                           this image, so `crop_and_resize` / `resize_cubic` below restate the published OpenCV arithmetic -
                           parity UNPINNED for those two functions (said in DESIGN.md); everything downstream of them is
                           pinned by tests/golden/siamfc_*.npz.
Only num_convs=1, kernel_size=1 heads train here (what the probe's config builds, default_config_base.py:33-37)."""
import numpy as np
import torch

from .engine import BF16, bump_params_epoch, shared_engine
from .siamfc_heads import SiamConvFC, SiamFC, _nhwc_bf16

DEFAULT_CFG = dict(      # default_config_base.py:2-51
    out_scale=0.001, exemplar_sz=120, instance_sz=255, context=0.5, scale_num=3, scale_step=1.0375, scale_lr=0.59, scale_penalty=0.9745,
    window_influence=0.176, response_sz=17, response_up=16, total_stride=8, epoch_num=50, batch_size=8, initial_lr=1e-3,
    ultimate_lr=1e-5, weight_decay=5e-4, momentum=0.9, r_pos=16, r_neg=0, optimizer='Adam', loss='focal', lr_schedule='exp',
    lr_step_size=10, extra_conv=True, out_channels=512, reduction=1, force_wd=False,
    backbone=dict(frozen_stages=4, dilations=(1, 1, 2, 4), strides=(1, 2, 1, 1), out_indices=(3,), norm_eval=True))
MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)


class _PerTensorOptimizer(torch.optim.Optimizer):
    """one launch per parameter tensor (the frozen probe has four); subclasses name their state and launch their kernel"""

    @torch.no_grad()
    def step(self, closure=None):
        eng = shared_engine()
        bump_params_epoch()      # raw-pointer update: packed / folded copies of the parameters must refresh
        for grp in self.param_groups:
            for p in grp['params']:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st.update(self._new_state(p))
                self._launch(eng.lib, grp, p, st, eng.stream(p.device))


class Adam(_PerTensorOptimizer):
    """torch.optim.Adam (amsgrad off) through vfs_adam_step"""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _new_state(self, p):
        return dict(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))

    def _launch(self, lib, grp, p, st, s):
        st['step'] += 1
        lib.adam_step(p.data, p.grad, st['exp_avg'], st['exp_avg_sq'], p.numel(), float(grp['lr']), float(grp['betas'][0]),
                      float(grp['betas'][1]), float(grp['eps']), float(grp['weight_decay']), int(st['step']), s)


class ParamSGD(_PerTensorOptimizer):
    """torch.optim.SGD (momentum, weight decay) through vfs_sgd_step"""

    def __init__(self, params, lr=1e-2, momentum=0.9, weight_decay=0):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))

    def _new_state(self, p):
        return dict(momentum_buffer=torch.zeros_like(p))

    def _launch(self, lib, grp, p, st, s):
        lib.sgd_step(p.data, p.grad, st['momentum_buffer'], p.numel(), float(grp['lr']), float(grp['momentum']),
                     float(grp['weight_decay']), None, s)


def _ensure_grads(params):
    """a zero .grad for every trainable parameter that has none: the backward kernels accumulate into it through its pointer"""
    for p in params:
        if p.requires_grad and p.grad is None:
            p.grad = torch.zeros_like(p)


def create_labels(size, r_pos, r_neg, total_stride, device):
    """siamfc_tracker_base.py:456-500: logistic labels on the response grid (block distance to the centre)"""
    n, c, h, w = size
    x, y = np.meshgrid(np.arange(w) - (w - 1) / 2, np.arange(h) - (h - 1) / 2)
    dist = np.abs(x) + np.abs(y)
    lab = np.where(dist <= r_pos / total_stride, 1.0, np.where(dist < r_neg / total_stride, 0.5, 0.0))
    return torch.from_numpy(np.tile(lab.reshape(1, 1, h, w), (n, c, 1, 1))).float().to(device)


def head_loss_backward(head, zf, xf, labels, loss='focal', param=None, backward=True):
    """responses = head(z, x); loss (losses.py: 'balance' | 'focal'); with backward=True the head's parameter gradients are
    ACCUMULATED into .grad (create them with zero_grad first).  zf / xf: NCHW fp32 features.  -> (loss tensor [1], responses)"""
    out, resp, _, _ = head_loss_backward_nhwc(head, _nhwc_bf16(zf), _nhwc_bf16(xf), labels, loss, param, backward)
    return out, resp


def head_loss_backward_nhwc(head, z, x, labels, loss='focal', param=None, backward=True, feat_grads=False):
    """head_loss_backward on NHWC bf16 features (what the backbone's training path hands over); SiamConvFC's 1x1 convs go back
    through Engine.conv_bwd (weight / bias gradients on the side stream, joined before the return).  feat_grads (fine-tuning,
    siamfc_tracker_base.py:131-144: the optimizer holds the backbone too): also the gradients wrt z and x, bf16 NHWC - for
    SiamConvFC ENGINE BUFFERS (<unit name>.gin), valid until the next call.  -> (loss tensor [1], responses, dz, dx)"""
    eng = shared_engine(x.device)
    dev = x.device
    s = eng.stream(dev)
    n_resp = x.shape[0] * (x.shape[1] - z.shape[1] + 1) * (x.shape[2] - z.shape[2] + 1)      # the 1x1 convs keep the size
    if labels.numel() != n_resp:      # the loss kernel reads n_resp labels: a map built for another response size would be read past its end
        raise ValueError(f'head_loss_backward: {labels.numel()} labels {tuple(labels.shape)} for {n_resp} responses')
    convs = isinstance(head, SiamConvFC)
    if convs and (len(head.z_convs) != 1):
        raise NotImplementedError('probe training: num_convs=1 heads (siamfc_tracker_base.py:108-113)')
    zc, xc = (head._conv1x1(head.z_units[0], z), head._conv1x1(head.x_units[0], x)) if convs else (z, x)
    nz, hz, wz, c = zc.shape
    nx, h, w, _ = xc.shape
    ho, wo = h - hz + 1, w - wz + 1
    resp = torch.empty(nx, 1, ho, wo, device=dev)
    eng.lib.xcorr_fwd(zc, xc, resp, nz, nx, hz, wz, h, w, c, float(head.out_scale), s)
    mode = {'balance': 0, 'focal': 1}[loss]
    if param is None:
        param = 1.0 if mode == 0 else 2.0
    out = torch.empty(1, device=dev)
    g = torch.empty_like(resp) if backward else None
    eng.lib.siamfc_loss(resp, labels.contiguous(), out, g, resp.numel(), mode, float(param), 1.0, s)
    dz = dx = None
    if backward and (convs or feat_grads):
        dz, dx = torch.empty_like(zc), torch.empty_like(xc)
        eng.lib.xcorr_bwd(zc, xc, g, dz, dx, nz, nx, hz, wz, h, w, c, float(head.out_scale), s)
    if backward and convs:
        _ensure_grads(head.parameters())
        gins = []
        for u, feat, d in ((head.z_units[0], z, dz), (head.x_units[0], x, dx)):
            n_, hh, ww, _ = feat.shape
            head._pack(u, need_wd=feat_grads)
            gins.append(eng.conv_bwd(u, d, feat, n_, hh, ww, hh, ww, need_dgrad=feat_grads)[0])
        dz, dx = gins
        eng.wgrad_join(dev)      # callers step an optimizer right after
    return out, resp, dz, dx


class SiamFCProbe:
    """TrackerSiamFC (siamfc_tracker_base.py:88-500): `cfg` = the reference's default_cfg keys (DEFAULT_CFG above)."""

    def __init__(self, cfg=None, depth=50, backbone=None, device=None, device_loop=False):
        from .resnet import ResNet
        self.cfg = dict(DEFAULT_CFG, **(cfg or {}))
        self.device_loop = bool(device_loop)      # tracking: crops, up-sampling and peak search on the device (csrc/siamfc_track.hip)
        c = self.cfg
        self.device = torch.device(device) if device is not None else torch.device('cuda:0' if torch.cuda.is_available() else 'cpu')
        self.backbone = backbone if backbone is not None else ResNet(depth, norm_cfg=dict(type='BN', requires_grad=True), **c['backbone'])
        self.head = (SiamConvFC(c['out_channels'], c['out_channels'] // c['reduction'], out_scale=c['out_scale']) if c['extra_conv']
                     else SiamFC(out_scale=c['out_scale']))
        self.backbone.to(self.device).eval()          # frozen_stages=4 + norm_eval: train(True) leaves every layer in eval mode
        self.head.to(self.device)
        # frozen_stages < 4 (siamfc_tracker_base.py:131-144): the optimizer holds self.net.parameters(), backbone included; the
        # backbone runs its bf16 training path inside train_step and stays in eval mode (fp32 executor) everywhere else
        self.finetune = c['backbone'].get('frozen_stages', -1) < 4 and any(p.requires_grad for p in self.backbone.parameters())
        params = [p for p in self.backbone.parameters() if p.requires_grad] if self.finetune else []
        params += [p for p in self.head.parameters() if p.requires_grad]
        wd = c['weight_decay'] if (c['backbone'].get('frozen_stages', -1) < 4 or c['force_wd']) else 0     # :135-137
        if not params:
            self.optimizer = None
        elif c['optimizer'] == 'SGD':
            self.optimizer = ParamSGD(params, lr=c['initial_lr'], weight_decay=wd, momentum=c['momentum'])
        elif c['optimizer'] == 'Adam':
            self.optimizer = Adam(params, lr=c['initial_lr'], weight_decay=wd)
        else:
            raise NotImplementedError(c['optimizer'])
        self.lr_scheduler = None
        if self.optimizer is not None:
            if c['lr_schedule'] == 'exp':
                gamma = np.power(c['ultimate_lr'] / c['initial_lr'], 1.0 / c['epoch_num'])
                self.lr_scheduler = torch.optim.lr_scheduler.ExponentialLR(self.optimizer, gamma)
            elif c['lr_schedule'] == 'step':
                self.lr_scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, c['lr_step_size'])
            elif c['lr_schedule'] != 'fixed':
                raise NotImplementedError(c['lr_schedule'])
        if c['loss'] not in ('balance', 'focal'):
            raise NotImplementedError(c['loss'])
        self._mean = torch.tensor(MEAN, device=self.device).view(1, 3, 1, 1)
        self._std = torch.tensor(STD, device=self.device).view(1, 3, 1, 1)
        self.labels = None

    # ------------------------------------------------------------------ training
    def normalize(self, imgs):
        return (imgs - self._mean) / self._std

    def features(self, imgs):
        """frozen backbone, eval mode (reference precision: the fp32 evaluation path)"""
        with torch.no_grad():
            return self.backbone(self.normalize(imgs.to(self.device).float()))

    def _create_labels(self, size):
        if self.labels is not None and tuple(self.labels.size()) == tuple(size):
            return self.labels
        c = self.cfg
        self.labels = create_labels(size, c['r_pos'], c['r_neg'], c['total_stride'], self.device)
        return self.labels

    def current_lr(self):
        return [g['lr'] for g in self.optimizer.param_groups]

    def _zero_grads(self):
        """every optimizer parameter gets a zeroed .grad: the backward kernels accumulate into it"""
        self.optimizer.zero_grad(set_to_none=False)
        _ensure_grads(p for grp in self.optimizer.param_groups for p in grp['params'])

    def train_step(self, batch, backward=True):
        """batch = (z [N,3,ez,ez], x [N,3,ix,ix]) uint8-range RGB floats, as the reference's Pair dataset yields them"""
        if self.finetune and backward and self.optimizer is not None:
            return self._train_step_finetune(batch)
        zf, xf = self.features(batch[0]), self.features(batch[1])
        nz, _, hz, wz = zf.shape
        nx, _, h, w = xf.shape
        labels = self._create_labels((nx, 1, h - hz + 1, w - wz + 1))
        if backward and self.optimizer is not None:
            self._zero_grads()
        loss, _ = head_loss_backward(self.head, zf, xf, labels, self.cfg['loss'], backward=backward and self.optimizer is not None)
        if backward and self.optimizer is not None:
            self.optimizer.step()
        return float(loss.item())

    def _train_step_finetune(self, batch):
        """train_step with a partly unfrozen backbone: loss + gradients of backbone and head, one optimizer step over both"""
        loss = self.finetune_loss_backward(batch)
        self.optimizer.step()
        return float(loss.item())

    def finetune_loss_backward(self, batch, branches=('z', 'x')):
        """exemplar and search images through the bf16 training path (train() mode; norm_eval keeps every BatchNorm on its running
        statistics), the loss backward through the head into the backbone passes named in `branches` (the reference: both) - two
        contexts of different sizes alive at once, each in its own buffer namespace.  Gradients of every optimizer parameter are
        zeroed, then accumulated into .grad.  -> loss tensor [1]"""
        eng = shared_engine(self.device)
        dev, bb = self.device, self.backbone
        s = eng.stream(dev)
        bb.train()
        try:
            bb.attach(eng)
            eng.pack_weights()
            stage = bb.last_stage()
            feats, ctxs = [], []
            for tag, imgs in (('.z', batch[0]), ('.x', batch[1])):
                x = self.normalize(imgs.to(dev).float()).contiguous()
                N, _, H, W = x.shape
                Wp = W + (W & 1)
                x4 = eng.buf(f'backbone.x4{tag}', (N, H, Wp, 4), BF16, dev)
                eng.lib.imgs_to_nhwc4(x, x4, N, 1, 1, H, W, Wp, s)
                outs, ctx = bb.forward_nhwc(eng, x4, N, H, W, 1, True, tag=tag)
                feats.append(outs[stage][0])
                ctxs.append(ctx)
            z, x = feats
            labels = self._create_labels((x.shape[0], 1, x.shape[1] - z.shape[1] + 1, x.shape[2] - z.shape[2] + 1))
            self._zero_grads()
            loss, _, dz, dx = head_loss_backward_nhwc(self.head, z, x, labels, self.cfg['loss'], backward=True, feat_grads=True)
            if 'x' in branches:
                bb.backward_nhwc(eng, ctxs[1], {stage: dx})
            if 'z' in branches:
                bb.backward_nhwc(eng, ctxs[0], {stage: dz})
            eng.wgrad_join(dev)
        finally:
            bb.eval()
        return loss

    # ------------------------------------------------------------------ tracking (:199-347)
    def _start_state(self, img, box):
        """the tracker state init() derives from the first frame and its 1-indexed ltwh box
        -> center [2], target_sz [2] (float32 arrays), z_sz, x_sz (float32 scalars), avg_color [3] (float64)"""
        c = self.cfg
        box = np.array([box[1] - 1 + (box[3] - 1) / 2, box[0] - 1 + (box[2] - 1) / 2, box[3], box[2]], dtype=np.float32)
        center, target_sz = box[:2], box[2:]
        context = c['context'] * np.sum(target_sz)
        z_sz = np.sqrt(np.prod(target_sz + context))
        x_sz = z_sz * c['instance_sz'] / c['exemplar_sz']
        return center, target_sz, z_sz, x_sz, np.mean(img, axis=(0, 1))

    def _init_windows(self):
        c = self.cfg
        self.upscale_sz = c['response_up'] * c['response_sz']
        self.hann_window = np.outer(np.hanning(self.upscale_sz), np.hanning(self.upscale_sz))
        self.hann_window /= self.hann_window.sum()
        self.scale_factors = c['scale_step'] ** np.linspace(-(c['scale_num'] // 2), c['scale_num'] // 2, c['scale_num'])

    @torch.no_grad()
    def init(self, img, box):
        c = self.cfg
        self._init_windows()
        self.center, self.target_sz, self.z_sz, self.x_sz, self.avg_color = self._start_state(img, box)
        if self.device_loop:
            self._init_device_loop(img)
            return
        z = crop_and_resize(img, self.center, self.z_sz, c['exemplar_sz'], self.avg_color)
        z = torch.from_numpy(z).to(self.device).permute(2, 0, 1).unsqueeze(0).float()
        self.kernel = self.features(z)

    @torch.no_grad()
    def update(self, img):
        if self.device_loop:
            return self._update_device(img)
        c = self.cfg
        x = np.stack([crop_and_resize(img, self.center, self.x_sz * f, c['instance_sz'], self.avg_color) for f in self.scale_factors])
        x = torch.from_numpy(x).to(self.device).permute(0, 3, 1, 2).float()
        responses = self.head(self.kernel, self.features(x)).squeeze(1).cpu().numpy()
        responses = np.stack([resize_cubic(u, self.upscale_sz, self.upscale_sz) for u in responses])
        responses[:c['scale_num'] // 2] *= c['scale_penalty']
        responses[c['scale_num'] // 2 + 1:] *= c['scale_penalty']
        scale_id = np.argmax(np.amax(responses, axis=(1, 2)))
        response = responses[scale_id]
        response -= response.min()
        response /= response.sum() + 1e-16
        response = (1 - c['window_influence']) * response + c['window_influence'] * self.hann_window
        loc = np.unravel_index(response.argmax(), response.shape)
        return self._apply_peak(scale_id, loc)

    def _apply_peak(self, scale_id, loc):
        """the peak (scale_id, (row, col) in the up-sampled response) -> new centre and sizes (host state), the frame's ltwh box"""
        c = self.cfg
        disp_in_response = np.array(loc) - (self.upscale_sz - 1) / 2
        disp_in_instance = disp_in_response * c['total_stride'] / c['response_up']
        disp_in_image = disp_in_instance * self.x_sz * self.scale_factors[scale_id] / c['instance_sz']
        self.center += disp_in_image
        scale = (1 - c['scale_lr']) * 1.0 + c['scale_lr'] * self.scale_factors[scale_id]
        self.target_sz *= scale
        self.z_sz *= scale
        self.x_sz *= scale
        return np.array([self.center[1] + 1 - (self.target_sz[1] - 1) / 2, self.center[0] + 1 - (self.target_sz[0] - 1) / 2,
                         self.target_sz[1], self.target_sz[0]])

    def track(self, frames, box):
        """frames: iterable of RGB uint8 arrays [H,W,3] (the reference reads files with cv2); box: 1-indexed ltwh"""
        boxes = []
        for f, img in enumerate(frames):
            if f == 0:
                self.init(img, box)
                boxes.append(np.asarray(box, dtype=np.float64))
            else:
                boxes.append(self.update(img))
        return np.stack(boxes)

    # ------------------------------------------------------------------ tracking, device loop (csrc/siamfc_track.hip)
    def _upload_frame(self, img):
        d = self._dl
        if tuple(img.shape) != d['shape'] or img.dtype != np.uint8:
            raise ValueError(f'device_loop: frames must be uint8 {d["shape"]} like the first one, got {img.dtype} {tuple(img.shape)}')
        d['frame'].copy_(torch.from_numpy(np.ascontiguousarray(img)))

    def _device_crops(self, sizes, out_size, out):
        """crop_and_resize of the uploaded frame around self.center for every size -> `out` fp32 [len(sizes),3,out_size,out_size]"""
        d = self._dl
        params = np.stack([crop_params(d['shape'], self.center, sz, out_size, self.avg_color) for sz in sizes])
        eng = shared_engine(self.device)
        eng.lib.siamfc_crops(d['frame'], params.ctypes.data, out, d['shape'][0], d['shape'][1], len(sizes), int(out_size),
                             eng.stream(self.device))

    def _device_tables(self, r):
        """the constant operands of the up-sampling and peak kernels for r x r responses, on the device"""
        c, dev = self.cfg, self.device
        S, up = int(c['scale_num']), int(self.upscale_sz)
        idx, w = _cubic_taps(r, up)
        pen = np.ones(S, np.float32)
        pen[:S // 2] = pen[S // 2 + 1:] = np.float32(c['scale_penalty'])
        return dict(tap_idx=torch.from_numpy(idx.astype(np.int32)).to(dev), tap_w=torch.from_numpy(w).to(dev),
                    penalty=torch.from_numpy(pen).to(dev), hann=torch.from_numpy(np.ascontiguousarray(self.hann_window)).to(dev),
                    one_minus_wi=float(np.float32(1 - c['window_influence'])))      # the host multiplies its fp32 map by this scalar

    def _init_device_loop(self, img):
        """the exemplar through the crop kernel, then everything update() needs per frame, uploaded / allocated once"""
        c, dev = self.cfg, self.device
        S, up = int(c['scale_num']), int(self.upscale_sz)
        d = self._dl = dict(shape=tuple(img.shape))
        d['frame'] = torch.empty(d['shape'], dtype=torch.uint8, device=dev)
        d['z'] = torch.zeros(1, 3, c['exemplar_sz'], c['exemplar_sz'], device=dev)
        d['x'] = torch.zeros(S, 3, c['instance_sz'], c['instance_sz'], device=dev)
        self._upload_frame(img)
        self._device_crops([self.z_sz], c['exemplar_sz'], d['z'])
        self.kernel = self.features(d['z'])
        shape = self.head(self.kernel, self.features(d['x'])).shape      # a dry pass on the blank search batch: the response size
        if shape[0] != S or shape[-1] != shape[-2]:
            raise ValueError(f'device_loop: {S} square response maps expected, got {tuple(shape)}')
        d['r'] = r = int(shape[-1])
        d.update(self._device_tables(r))
        d['up'] = torch.empty(S, up, up, device=dev)
        d['scale_max'] = torch.zeros(S, dtype=torch.int64, device=dev)
        d['record'] = torch.zeros(4, dtype=torch.int32, device=dev)

    def _update_device(self, img):
        """update() with one frame upload and one 16-byte read-back: crops -> features -> head -> up-sampling -> peak on the device;
        the state (centre, sizes) stays on the host and advances through the same _apply_peak as the host loop"""
        c, d = self.cfg, self._dl
        S, r, up = int(c['scale_num']), d['r'], int(self.upscale_sz)
        eng = shared_engine(self.device)
        s = eng.stream(self.device)
        self._upload_frame(img)
        self._device_crops([self.x_sz * f for f in self.scale_factors], c['instance_sz'], d['x'])
        d['responses'] = resp = self.head(self.kernel, self.features(d['x']))
        if tuple(resp.shape) != (S, 1, r, r):
            raise ValueError(f'device_loop: response maps {tuple(resp.shape)} differ from those init() sized its buffers for')
        eng.lib.siamfc_upsample(resp, d['tap_idx'], d['tap_w'], d['penalty'], d['up'], d['scale_max'], S, r, up, s)
        eng.lib.siamfc_peak(d['up'], d['scale_max'], d['hann'], d['record'], S, up, d['one_minus_wi'], float(c['window_influence']), s)
        scale_id, row, col, _ = d['record'].tolist()      # the frame's only read-back (and its only synchronisation)
        self.last_peak = (scale_id, row, col)
        return self._apply_peak(scale_id, (row, col))

    # ------------------------------------------------------------------ tracking, a batch of sequences (csrc/siamfc_track.hip)
    @torch.no_grad()
    def track_batch(self, sequences, boxes, batch=16):
        """track() for many sequences at once, the tracker state on the device (vfs_siamfc_batch_crops / _upsample / _peak;
        state layout in include/vfs_hip.h).  sequences: indexable frame sequences with len(), frames RGB uint8 [H,W,3]; boxes:
        their 1-indexed ltwh boxes; -> a list of float64 [T_i,4] arrays, what track() returns for each sequence.

        At most `batch` (<= 64) slots advance in lock-step: per frame step the slots' frames are packed into one pinned staging
        buffer and go up in one copy, then crops -> features -> head -> up-sampling -> peak run for all slots, and the peak kernel
        moves every slot's state and writes its box.  The lengths are known up front, so the schedule is the host's: a slot whose
        sequence has ended is refilled with the next waiting one (its initial state as init() computes it, uploaded; its exemplar
        through a one-image feature pass), and goes inactive when none is left.  Nothing is read back before the last step; the
        host only ever waits for the upload that used the same staging buffer three steps earlier.  Every buffer is allocated
        once per call, sized by `batch` and the largest frame (the first frame of every sequence is looked at up front).
        Always the device path, whatever `device_loop` says, with its limitation: one frame size per sequence (sequences may
        differ).  A slot whose state left the checked range raises RuntimeError naming the sequence."""
        from collections import deque
        c, dev = self.cfg, self.device
        eng = shared_engine(dev)
        lib = eng.lib
        nseq = len(sequences)
        if len(boxes) != nseq:
            raise ValueError(f'track_batch: {nseq} sequences, {len(boxes)} boxes')
        if not 1 <= int(batch) <= 64:
            raise ValueError(f'track_batch: 1 <= batch <= 64, got {batch}')
        lengths = [len(q) for q in sequences]
        if min(lengths, default=1) < 1:
            raise ValueError('track_batch: an empty sequence')
        if nseq == 0:
            return []
        self._init_windows()
        N, S, up = min(int(batch), nseq), int(c['scale_num']), int(self.upscale_sz)
        ez, ix = int(c['exemplar_sz']), int(c['instance_sz'])
        shapes = [tuple(q[0].shape) for q in sequences]
        if any(len(sh) != 3 or sh[2] != 3 for sh in shapes):
            raise ValueError('track_batch: frames must be [H,W,3]')
        nbytes = [sh[0] * sh[1] * 3 for sh in shapes]
        slot_bytes = (max(nbytes) + 255) // 256 * 256
        bases = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)      # sequence i owns rows bases[i] .. bases[i + 1] - 1
        rows_cap = int(bases[-1])
        cuda = dev.type == 'cuda'

        b = self._bl = dict()
        b['frames'] = torch.empty(N * slot_bytes, dtype=torch.uint8, device=dev)
        b['init_frame'] = torch.empty(slot_bytes, dtype=torch.uint8, device=dev)
        b['state'] = torch.zeros(N, 8, dtype=torch.float64, device=dev)
        b['meta'] = torch.zeros(N, 8, dtype=torch.int32, device=dev)
        b['frame_off'] = torch.zeros(N, dtype=torch.int64, device=dev)
        b['zero_off'] = torch.zeros(1, dtype=torch.int64, device=dev)
        b['factors'] = torch.from_numpy(np.ascontiguousarray(self.scale_factors, dtype=np.float64)).to(dev)
        b['one'] = torch.ones(1, dtype=torch.float64, device=dev)
        b['z'] = torch.zeros(1, 3, ez, ez, device=dev)
        b['x'] = torch.zeros(S * N, 3, ix, ix, device=dev)
        b['boxes'] = torch.zeros(rows_cap, 4, dtype=torch.float64, device=dev)
        b['records'] = torch.zeros(rows_cap, 4, dtype=torch.int32, device=dev)
        b['seq_status'] = torch.zeros(nseq, dtype=torch.int32, device=dev)
        one_z = self.features(b['z'])      # a dry pass on blank crops: the exemplar bank's and the responses' sizes
        b['bank'] = torch.zeros(N, *one_z.shape[1:], device=dev)
        shape = self.head(b['bank'], self.features(b['x'])).shape
        if shape[0] != S * N or shape[-1] != shape[-2]:
            raise ValueError(f'track_batch: {S * N} square response maps expected, got {tuple(shape)}')
        r = int(shape[-1])
        b.update(self._device_tables(r))
        b['up'] = torch.empty(S * N, up, up, device=dev)
        b['scale_max'] = torch.zeros(N, S, dtype=torch.int64, device=dev)
        ring = [torch.empty(N * slot_bytes, dtype=torch.uint8, pin_memory=cuda) for _ in range(3)]
        ring_np = [t.numpy() for t in ring]
        ring_ev = [torch.cuda.Event() if cuda else None for _ in ring]
        uploads = 0

        def upload(dst, parts):
            """parts [(byte offset, frame)] -> dst, through the next staging buffer; the copy is asynchronous"""
            nonlocal uploads
            k = uploads % len(ring)
            if cuda and uploads >= len(ring):
                ring_ev[k].synchronize()      # the copy that last read this staging buffer, three uploads ago
            end = 0
            for off, img in parts:
                ring_np[k][off:off + img.size].reshape(img.shape)[...] = img
                end = max(end, off + img.size)
            dst[:end].copy_(ring[k][:end], non_blocking=True)
            if cuda:
                ring_ev[k].record()
            uploads += 1

        def frame_of(i, t):
            img = sequences[i][t]
            if tuple(img.shape) != shapes[i] or img.dtype != np.uint8:
                raise ValueError(f'track_batch: sequence {i}: frames must be uint8 {shapes[i]} like the first one, got {img.dtype} {tuple(img.shape)}')
            return img

        def retire(n):
            b['seq_status'][slot_seq[n]:slot_seq[n] + 1].copy_(b['meta'][n, 7:8])      # device to device: the refill clears the word
            slot_seq[n] = None

        def refill(n, i):
            img = frame_of(i, 0)
            center, target_sz, z_sz, x_sz, avg = self._start_state(img, boxes[i])
            fill = np.clip(np.rint(avg), 0, 255)
            b['state'][n].copy_(torch.tensor([center[0], center[1], target_sz[0], target_sz[1], z_sz, x_sz, 0, 0], dtype=torch.float64))
            b['meta'][n].copy_(torch.tensor([1, shapes[i][0], shapes[i][1], fill[0], fill[1], fill[2], bases[i] + 1, 0], dtype=torch.int32))
            upload(b['init_frame'], [(0, img)])
            lib.siamfc_batch_crops(b['init_frame'], b['zero_off'], b['state'][n:n + 1], b['meta'][n:n + 1], b['one'], b['z'], 1, 1, ez, 1,
                                   eng.stream(dev))
            b['bank'][n].copy_(self.features(b['z'])[0])
            slot_seq[n], slot_t[n] = i, 1

        waiting = deque(i for i in range(nseq) if lengths[i] > 1)
        slot_seq, slot_t = [None] * N, [0] * N
        while True:
            moved = False
            for n in range(N):
                if slot_seq[n] is not None and slot_t[n] >= lengths[slot_seq[n]]:
                    retire(n)
                    if not waiting:
                        b['meta'][n, 0:1].zero_()      # inactive from here on
                    moved = True
                if slot_seq[n] is None and waiting:
                    refill(n, waiting.popleft())
                    moved = True
            live = [n for n in range(N) if slot_seq[n] is not None]
            if not live:
                break
            if moved:      # the frames are packed back to back: the offsets change only when a slot changes hands
                offs = np.zeros(N, np.int64)
                offs[live] = np.concatenate([[0], np.cumsum([(nbytes[slot_seq[n]] + 255) // 256 * 256 for n in live])])[:-1]
                b['frame_off'].copy_(torch.from_numpy(offs))
            upload(b['frames'], [(int(offs[n]), frame_of(slot_seq[n], slot_t[n])) for n in live])
            s = eng.stream(dev)
            lib.siamfc_batch_crops(b['frames'], b['frame_off'], b['state'], b['meta'], b['factors'], b['x'], N, S, ix, 0, s)
            b['responses'] = resp = self.head(b['bank'], self.features(b['x']))
            if tuple(resp.shape) != (S * N, 1, r, r):
                raise ValueError(f'track_batch: response maps {tuple(resp.shape)} differ from those the buffers were sized for')
            lib.siamfc_batch_upsample(resp, b['tap_idx'], b['tap_w'], b['penalty'], b['up'], b['scale_max'], N, S, r, up, s)
            lib.siamfc_batch_peak(b['up'], b['scale_max'], b['hann'], b['factors'], b['state'], b['meta'], b['boxes'], b['records'], rows_cap,
                                  N, S, up, b['one_minus_wi'], float(c['window_influence']), float(c['total_stride']), float(c['response_up']),
                                  float(c['instance_sz']), float(c['scale_lr']), s)
            for n in live:
                slot_t[n] += 1

        out = b['boxes'].cpu().numpy()      # the call's only read-backs (and its only synchronisation with the results)
        status = b['seq_status'].cpu().numpy()
        rec = b['records'].cpu().numpy()
        bad = np.flatnonzero(status)
        if len(bad):
            raise RuntimeError('track_batch: ' + ', '.join(f'sequence {i}: status {int(status[i])}' for i in bad) +
                               ' (1: state not finite or out of range, 2: crop geometry, 4: out of box rows; include/vfs_hip.h)')
        res = []
        for i in range(nseq):
            bx = out[bases[i]:bases[i + 1]].copy()
            bx[0] = np.asarray(boxes[i], dtype=np.float64)
            res.append(bx)
        self.last_batch_records = [rec[bases[i] + 1:bases[i + 1], :3].copy() for i in range(nseq)]      # per frame: scale_id, row, col
        return res


# ---------------------------------------------------------------------------------------------
# cv2 stand-ins (cv2 is not in this image).  Restated from the published OpenCV implementation; parity UNPINNED.
# ---------------------------------------------------------------------------------------------
def _resize_linear_u8(img, ow, oh):
    """cv2.resize(INTER_LINEAR) on 8-bit data: 11-bit fixed-point coefficients, horizontal then vertical pass"""
    ih, iw = img.shape[:2]

    def coeffs(n_in, n_out):
        scale = n_in / n_out
        f = (np.arange(n_out) + 0.5) * scale - 0.5
        i0 = np.floor(f).astype(np.int64)
        fr = f - i0
        lo = i0 < 0
        fr[lo], i0[lo] = 0.0, 0
        hi = i0 >= n_in - 1
        fr[hi] = 0.0
        i0 = np.minimum(i0, n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        c1 = np.rint(fr * 2048).astype(np.int64)
        return i0, i1, 2048 - c1, c1
    x0, x1, a0, a1 = coeffs(iw, ow)
    y0, y1, b0, b1 = coeffs(ih, oh)
    src = img.astype(np.int64)
    rows = src[:, x0] * a0[None, :, None] + src[:, x1] * a1[None, :, None]            # [ih, ow, c], scaled by 2^11
    out = ((b0[:, None, None] * (rows[y0] >> 4)) >> 16) + ((b1[:, None, None] * (rows[y1] >> 4)) >> 16)
    return np.clip((out + 2) >> 2, 0, 255).astype(np.uint8)


def crop_and_resize(img, center, size, out_size, border_value):
    """ops.crop_and_resize(faster=True) -> image_utils.get_cropped_input: the in-image part of the square box is resized to
    its share of out_size, the rest is padded with the average colour"""
    size = max(2, float(size))
    yc, xc = float(center[0]), float(center[1])
    box = np.round(np.array([xc - size / 2, yc - size / 2, xc + size / 2, yc + size / 2])).astype(int)     # x0, y0, x1, y1
    wh = np.array([box[2] - box[0], box[3] - box[1]])
    H, W = img.shape[:2]
    patch = img[max(box[1], 0):min(box[3], H), max(box[0], 0):min(box[2], W)]
    out_size = int(out_size)
    fill = np.asarray(border_value, dtype=np.float64)
    if patch.shape[0] == 0 or patch.shape[1] == 0:
        return np.zeros((out_size, out_size, 3), img.dtype)
    bounded = np.clip(box, 0, [W, H, W, H])
    bwh = np.array([bounded[2] - bounded[0], bounded[3] - bounded[1]])
    ow = max(1, int(np.round(out_size * bwh[0] / wh[0])))
    oh = max(1, int(np.round(out_size * bwh[1] / wh[1])))
    patch = _resize_linear_u8(np.ascontiguousarray(patch), ow, oh)
    pad = np.zeros(4, dtype=int)
    pad[:2] = np.maximum(0, -box[:2] * out_size / wh)
    pad[2:] = out_size - (pad[:2] + np.array([patch.shape[1], patch.shape[0]]))
    if np.any(pad != 0):
        if np.any(pad < 0):
            return np.zeros((out_size, out_size, 3))
        full = np.empty((out_size, out_size, 3), patch.dtype)
        full[:] = np.clip(np.rint(fill), 0, 255).astype(patch.dtype) if patch.dtype == np.uint8 else fill
        full[pad[1]:pad[1] + patch.shape[0], pad[0]:pad[0] + patch.shape[1]] = patch
        patch = full
    return patch


def crop_params(shape, center, size, out_size, border_value):
    """the geometry of crop_and_resize(img, ...) for an image of `shape`, as the int32 row vfs_siamfc_crops takes (include/vfs_hip.h):
    [valid, x / y origin and width / height of the in-image patch, its width / height after the resize, x / y pad, fill colour];
    valid = 0 where crop_and_resize returns zeros.  Same float64 expressions, same order."""
    size = max(2, float(size))
    yc, xc = float(center[0]), float(center[1])
    box = np.round(np.array([xc - size / 2, yc - size / 2, xc + size / 2, yc + size / 2])).astype(int)     # x0, y0, x1, y1
    wh = np.array([box[2] - box[0], box[3] - box[1]])
    H, W = shape[:2]
    rows = range(*slice(max(box[1], 0), min(box[3], H)).indices(H))      # what the patch slice selects (a negative stop counts from the end)
    cols = range(*slice(max(box[0], 0), min(box[2], W)).indices(W))
    out_size = int(out_size)
    p = np.zeros(12, np.int32)
    if len(rows) == 0 or len(cols) == 0:
        return p
    bounded = np.clip(box, 0, [W, H, W, H])
    bwh = np.array([bounded[2] - bounded[0], bounded[3] - bounded[1]])
    ow = max(1, int(np.round(out_size * bwh[0] / wh[0])))
    oh = max(1, int(np.round(out_size * bwh[1] / wh[1])))
    pad = np.zeros(4, dtype=int)
    pad[:2] = np.maximum(0, -box[:2] * out_size / wh)
    pad[2:] = out_size - (pad[:2] + np.array([ow, oh]))
    if np.any(pad < 0):
        return p
    p[:9] = 1, cols[0], rows[0], len(cols), len(rows), ow, oh, pad[0], pad[1]
    p[9:] = np.clip(np.rint(np.asarray(border_value, dtype=np.float64)), 0, 255)
    return p


def _cubic_taps(n_in, n_out):
    """resize_cubic along one axis: the four source indices [n_out,4] (border replicated) and fp32 weights [n_out,4] of every output"""
    f = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
    i0 = np.floor(f).astype(np.int64)
    t = (f - i0).astype(np.float32)
    A = np.float32(-0.75)
    w = np.stack([((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1,
                  ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1, np.zeros_like(t)], 1).astype(np.float32)
    w[:, 3] = 1 - w[:, 0] - w[:, 1] - w[:, 2]
    idx = np.clip(i0[:, None] + np.arange(-1, 3)[None], 0, n_in - 1)
    return idx, w


def resize_cubic(a, ow, oh):
    """cv2.resize(INTER_CUBIC) of a float32 map: Keys kernel with a = -0.75, pixel centres aligned, replicated border"""
    a = np.asarray(a, dtype=np.float32)
    xi, xw = _cubic_taps(a.shape[1], ow)
    yi, yw = _cubic_taps(a.shape[0], oh)
    rows = (a[:, xi] * xw[None]).sum(-1)              # [ih, ow]
    return (rows[yi] * yw[:, :, None]).sum(1).astype(np.float32)
