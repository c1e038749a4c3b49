"""DenseSimSiamHead: registry / state_dict contract against the reference's own vectors (tests/golden/dense_head.npz), the fused
train step with the dense head against the bf16-storage yardstick of tests/dense_head_oracle.py, chain replay, refusals.
backend=emu: CPU fiber emulator; backend=gpu: libvfs_hip.so on the MI355X.  Tiny shapes."""
import os

import numpy as np
import pytest
import torch

from oracle import vfs_oracle as O
from tests.dense_head_oracle import DenseHead, DenseTracker
from tests.emu_util import relerr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHALLOW = dict(num_stages=2, strides=(1, 2), out_indices=(1,))
SHALLOW_HEAD = dict(in_channels=128, projection_mid_channels=128, projection_out_channels=128, predictor_mid_channels=64,
                    predictor_out_channels=128)
IMGS = [2, 2, 3, 2, 32, 32]
# the two heads of tests/golden/gen_dense_head_golden.py (weights: fill_state_dict_ seed 21, inputs: fill_tensor seeds 31 / 32)
GOLDEN_HEAD = dict(in_channels=40, projection_mid_channels=48, projection_out_channels=72, predictor_mid_channels=24,
                   predictor_out_channels=72)
GOLDEN_SHAPE = [4, 40, 3, 5]
GOLDEN_HEAD64 = dict(in_channels=64, projection_mid_channels=64, projection_out_channels=128, predictor_mid_channels=64,
                     predictor_out_channels=128)      # channel counts the 1x1 convolution kernels take
GOLDEN_SHAPE64 = [4, 64, 3, 5]


def _l2rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _golden():
    return np.load(os.path.join(REPO, 'tests', 'golden', 'dense_head.npz'))


def test_registry_builds_the_reference_state_dict():
    import vfs_amd
    g = _golden()
    head = vfs_amd.build_head(dict(type='DenseSimSiamHead', **GOLDEN_HEAD))
    assert type(head) is vfs_amd.HEADS.get('DenseSimSiamHead')
    assert list(head.state_dict().keys()) == [str(k) for k in g['keys']]
    assert [n for n, _ in head.named_children()] == ['loss_feat', 'projection_convs', 'predictor_convs', 'predictor_plugin']
    assert [n for n, _ in head.projection_convs[0].named_children()] == ['conv', 'bn', 'activate']
    assert [n for n, _ in head.projection_convs[2].named_children()] == ['conv', 'bn']
    assert [n for n, _ in head.predictor_convs[1].named_children()] == ['conv']
    ref = DenseHead(**GOLDEN_HEAD)
    assert list(ref.state_dict().keys()) == list(head.state_dict().keys())
    head.load_state_dict(O.fill_state_dict_(ref, seed=21).state_dict())


def test_fp32_helper_matches_the_reference_vectors():
    """pins tests/dense_head_oracle.py: forward, loss and every gradient of the fp32 helper against the reference class"""
    g = _golden()
    ref = O.fill_state_dict_(DenseHead(**GOLDEN_HEAD), seed=21).train()
    x1 = O.fill_tensor(GOLDEN_SHAPE, 31, scale=1.5).requires_grad_(True)
    x2 = O.fill_tensor(GOLDEN_SHAPE, 32, scale=1.5).requires_grad_(True)
    (z1, p1), (z2, p2) = ref(x1), ref(x2)
    loss = DenseHead.loss(p1, z1, p2, z2)
    loss.mean().backward()
    for name, mine in (('z1', z1), ('p1', p1), ('z2', z2), ('p2', p2), ('loss', loss), ('dx1', x1.grad), ('dx2', x2.grad)):
        assert relerr(mine, torch.from_numpy(g[name])) < 1e-5, name
    for n, p in ref.named_parameters():
        assert relerr(p.grad, torch.from_numpy(g['grad/' + n])) < 1e-5, n


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def _nchw(t):
    return t.detach().cpu().float().permute(0, 3, 1, 2).contiguous()


def _helper64(emulate, train=True):
    """the helper on the k64 golden's weights and (bf16 emulation: bf16-rounded, as the HIP head reads them) inputs"""
    ref = O.fill_state_dict_(DenseHead(**GOLDEN_HEAD64), seed=21).set_emulate_bf16(emulate).train(train)
    xs = [O.fill_tensor(GOLDEN_SHAPE64, s, scale=1.5) for s in (31, 32)]
    return ref, [(O.round_bf16(x) if emulate else x).requires_grad_(True) for x in xs]


def _bar_report(name, mine, emu, scale, offset, failed):
    print(f'{name}: mine {mine:.3g} emu {emu:.3g}')
    if not mine <= scale * emu + offset:
        failed.append((name, mine, emu))


def test_hip_head_matches_the_reference_vectors(backend):
    """The head built through HEADS with the k64 golden's weights: forward_nhwc over the G = 2 view groups (each input its own
    BatchNorm batch, as one img_head(x) call each in the reference), the dense loss, backward_nhwc - against the vectors of the
    reference class.  Yardstick: emu = the deviation of the helper's bf16-storage emulation from the same vectors (relative L2);
    z, p, loss: mine <= 1.6 emu + 2e-3; every gradient: mine <= 2 emu + 5e-3."""
    import vfs_amd
    g = _golden()
    eng, dev = backend.eng, backend.dev
    head = vfs_amd.HEADS.get('DenseSimSiamHead')(**GOLDEN_HEAD64)
    assert list(head.state_dict().keys()) == [str(k) for k in g['k64/keys']]
    head.load_state_dict(_helper64(False)[0].state_dict())
    head.to(dev).train()
    for p in head.parameters():
        p.grad = torch.zeros_like(p)
    ref, (x1, x2) = _helper64(True)
    (rz1, rp1), (rz2, rp2) = ref(x1), ref(x2)
    rloss = DenseHead.loss(rp1, rz1, rp2, rz2)
    rloss.mean().backward()

    N, C, h, w = 8, *GOLDEN_SHAPE64[1:]
    Nv = N // 2
    head.attach(eng)
    eng.pack_weights()
    feat = _nhwc(torch.cat([x1.detach(), x2.detach()])).to(dev)
    z, p, ctx = head.forward_nhwc(eng, feat, N, h, w, C, 2, True)
    loss = torch.empty(1, Nv, device=dev)
    head.loss_fwd_nhwc(eng, p, z, loss, Nv, 1, 1, 1.0)
    dp = torch.empty_like(p)
    head.loss_bwd_nhwc(eng, p, z, torch.full((1, Nv), 1.0 / Nv, device=dev), dp, Nv, 1, 1, 1.0)      # d mean(loss) / d loss
    gfeat = head.backward_nhwc(eng, ctx, dp)
    eng.wgrad_join(dev)
    if dev.type == 'cuda':
        torch.cuda.synchronize()

    failed = []
    zc, pc, gc = _nchw(z), _nchw(p), _nchw(gfeat)
    for name, mine, emu in (('z1', zc[:Nv], rz1), ('z2', zc[Nv:], rz2), ('p1', pc[:Nv], rp1), ('p2', pc[Nv:], rp2),
                            ('loss', loss[0].cpu(), rloss)):
        want = torch.from_numpy(g['k64/' + name])
        _bar_report(name, _l2rel(mine, want), _l2rel(emu, want), 1.6, 2e-3, failed)
    for name, mine, emu in (('dx1', gc[:Nv], x1.grad), ('dx2', gc[Nv:], x2.grad)):
        want = torch.from_numpy(g['k64/' + name])
        _bar_report(name, _l2rel(mine, want), _l2rel(emu, want), 2.0, 5e-3, failed)
    rgrads = dict(ref.named_parameters())
    for n, prm in head.named_parameters():
        want = torch.from_numpy(g['k64/grad/' + n])
        if n == 'projection_convs.2.bn.bias':      # exactly 0 in exact arithmetic (see the train-step test): no relative bar
            assert want.norm() < 1e-6 and prm.grad.norm().cpu() < 5e-3, n
            continue
        assert want.norm() > 1e-6, n
        _bar_report('grad/' + n, _l2rel(prm.grad, want), _l2rel(rgrads[n].grad, want), 2.0, 5e-3, failed)
    assert not failed, failed
    # running statistics: both views updated them, one after the other
    sd, rsd = head.state_dict(), ref.state_dict()
    for k in rsd:
        if k.endswith('num_batches_tracked'):
            assert int(sd[k]) == int(rsd[k]) == 2, k


@pytest.mark.parametrize('train', [True, False])
def test_inference_entry_matches_the_reference_vectors(backend, train):
    """DenseSimSiamHead.forward: NCHW fp32 in, (z, p) NCHW fp32 out, one BatchNorm batch per call; train mode (batch statistics)
    and eval mode (the filled running statistics) against the reference's vectors under the forward bar of the test above"""
    import vfs_amd
    g = _golden()
    head = vfs_amd.build_head(dict(type='DenseSimSiamHead', **GOLDEN_HEAD64))
    head.load_state_dict(_helper64(False)[0].state_dict())
    head.to(backend.dev).train(train)
    ref, (x1, _) = _helper64(True, train)
    with torch.no_grad():
        rz, rp = ref(x1)
        z, p = head(O.fill_tensor(GOLDEN_SHAPE64, 31, scale=1.5).to(backend.dev))
    assert z.dtype == p.dtype == torch.float32 and tuple(z.shape) == (4, 128, 3, 5) and tuple(p.shape) == (4, 128, 3, 5)
    failed = []
    for name, mine, emu in (('z1', z, rz), ('p1', p, rp)):
        want = torch.from_numpy(g['k64/' + name + ('' if train else '_eval')])
        _bar_report(name, _l2rel(mine, want), _l2rel(emu, want), 1.6, 2e-3, failed)
    assert not failed, failed


def _mine(intra_video, loss_feat=None, head='DenseSimSiamHead'):
    import vfs_amd
    cfg = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', 'vfs_r18_dense.py' if head == 'DenseSimSiamHead' else 'vfs_r18.py'))
    mcfg = dict(cfg.model)
    mcfg['backbone'] = dict(mcfg['backbone'], **SHALLOW, dilations=(1, 1))
    mcfg['img_head'] = dict(mcfg['img_head'], **SHALLOW_HEAD)
    if loss_feat is not None:
        mcfg['img_head']['loss_feat'] = loss_feat
    return vfs_amd.build_model(mcfg, train_cfg=dict(intra_video=intra_video), test_cfg=cfg.test_cfg)


def _filled(intra_video):
    ref = DenseTracker(18, SHALLOW_HEAD, intra_video, **SHALLOW)
    O.fill_state_dict_(ref, seed=3)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, O.BasicBlock):
                m.conv2.bn.weight.mul_(0.25)
    return ref


def _run_oracle(imgs, emulate, intra_video):
    ref = _filled(intra_video)
    ref.set_emulate_bf16(emulate).train()
    rloss, rlog = O.parse_losses(ref.forward_train(imgs))
    rloss.backward()
    return ref, rlog


def _step(model, imgs):
    for p in model.parameters():
        if p.grad is not None:
            p.grad.zero_()
    out = model.train_step(dict(imgs=imgs, label=torch.zeros(imgs.shape[0], 1)), None)
    out['loss'].backward()
    if imgs.is_cuda:
        torch.cuda.synchronize()
    return dict(out['log_vars']), {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize('intra_video', [True, False])
def test_dense_train_step_matches_yardstick_and_replays(backend, intra_video, monkeypatch):
    """the project's yardstick (test_emu_train_step.py): the HIP step is as close to the fp32 helper as the helper's own
    bf16-storage emulation is - log vars: mine <= 1.6 emu + 2e-3, gradients (relative L2): mine <= 2 emu + 5e-3.  Then the
    replayed chain (step 4 of a model: the tape recorded during step 3) against a plain eager run of the same weights and inputs,
    bit for bit; on the GPU also the hipGraph replay."""
    imgs = O.fill_tensor(IMGS, seed=11, scale=2.0)
    ref32, log32 = _run_oracle(imgs, False, intra_video)
    refbf, logbf = _run_oracle(imgs, True, intra_video)

    def fresh():
        model = _mine(intra_video)
        assert list(model.state_dict().keys()) == list(ref32.state_dict().keys())
        model.load_state_dict(_filled(intra_video).state_dict())
        return model.to(backend.dev).train()

    monkeypatch.setenv('VFS_TAPE', '0')
    monkeypatch.setenv('VFS_GRAPHS', '0')
    model = fresh()
    log, grads = _step(model, imgs.to(backend.dev))
    assert getattr(model, '_gs', None) is None
    assert list(log.keys()) == list(log32.keys()) and len(log) == (IMGS[3] if intra_video else 1) + 1
    for k in log32:
        mine, emu = abs(log[k] - log32[k]), abs(logbf[k] - log32[k])
        print(f'{k}: mine {mine:.3g} emu {emu:.3g}')
        assert mine <= 1.6 * emu + 2e-3, (k, log[k], log32[k], logbf[k])
    g32, gbf = dict(ref32.named_parameters()), dict(refbf.named_parameters())
    for n, gr in grads.items():
        r = g32[n].grad
        assert torch.isfinite(gr).all(), n
        if n == 'img_head.projection_convs.2.bn.bias':
            # beta of the projector's last BatchNorm: a per-channel constant on z, which the predictor's first BatchNorm removes
            # again, and z itself is detached in the loss - its gradient is exactly 0 in exact arithmetic (1e-9 in the fp32
            # helper), so a relative bar has no meaning; here it is the rounding residue of the bf16 gradient sums
            assert r.norm() < 1e-6 and gr.norm() < 5e-3, (n, float(r.norm()), float(gr.norm()))
            continue
        assert r.norm() > 1e-6, n
        mine, emu = _l2rel(gr, r), _l2rel(gbf[n].grad, r)
        if n.startswith('img_head'):
            print(f'{n}: mine {mine:.3g} emu {emu:.3g}')
        assert mine <= 2.0 * emu + 5e-3, (n, mine, emu)

    modes = [dict(VFS_TAPE='1')] + ([dict(VFS_TAPE='1', VFS_GRAPHS='1')] if backend.name == 'gpu' and intra_video else [])
    for env in modes:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        replayed = fresh()
        dimgs = imgs.to(backend.dev)
        for _ in range(4):      # two eager steps (the buffers settle), the recording pass, one replay
            rlog, rgrads = _step(replayed, dimgs)
        assert replayed._gs.fwd is not None and replayed._gs.bwd is not None
        if 'VFS_GRAPHS' not in env:
            names = [op[0] for op in replayed._gs.fwd.ops]
            assert 'dense_cosine_loss_fwd' in names and 'cosine_loss_fwd' not in names and 'avgpool_fwd' not in names
            assert 'dense_cosine_loss_bwd' in [op[0] for op in replayed._gs.bwd.ops]
        assert rlog == log, (env, rlog, log)
        for n in grads:
            assert torch.equal(rgrads[n], grads[n]), (env, n)


def test_constructor_refusals_name_the_option():
    import vfs_amd
    for kw, word in ((dict(kernel_size=3), 'kernel_size'), (dict(predictor_plugin=dict(type='NonLocal2d')), 'predictor_plugin'),
                     (dict(conv_cfg=dict(type='Conv3d')), 'conv_cfg'), (dict(act_cfg=dict(type='LeakyReLU')), 'act_cfg'),
                     (dict(act_cfg=None), 'act_cfg')):
        with pytest.raises(NotImplementedError, match=word):
            vfs_amd.build_head(dict(type='DenseSimSiamHead', in_channels=64, **kw))
    with pytest.raises(KeyError):
        vfs_amd.build_head(dict(type='DenseSimSiamHead', in_channels=64, norm_cfg=dict(type='GN')))


def test_channel_counts_the_conv_kernels_do_not_take_are_refused(emu_backend):
    """the 1x1 convolution kernels take multiples of 64 channels: the head says so instead of launching"""
    import vfs_amd
    head = vfs_amd.build_head(dict(type='DenseSimSiamHead', **GOLDEN_HEAD))
    with pytest.raises(NotImplementedError, match='multiples of 64'):
        head.attach(emu_backend.eng)


@pytest.mark.parametrize('loss_feat', [dict(type='CosineSimLoss', pairwise=True), dict(type='CosineSimLoss', with_norm=False)])
def test_fused_step_refuses_other_loss_configs_and_head_loss_serves_them(backend, loss_feat):
    model = _mine(False, loss_feat=loss_feat).to(backend.dev).train()
    imgs = O.fill_tensor(IMGS, seed=11, scale=2.0).to(backend.dev)
    with pytest.raises(NotImplementedError, match='pairwise'):
        model.forward_train(imgs)
    kw = {k: v for k, v in loss_feat.items() if k != 'type'}
    p1, z1, p2, z2 = (O.fill_tensor([3, 16, 2, 5], 40 + i, scale=1.5) for i in range(4))
    mask = (O.fill_tensor([3, 10, 10], 50) > -0.2) if kw.get('pairwise') else None
    mine = model.img_head.loss(*(t.to(backend.dev) for t in (p1, z1, p2, z2)), mask12=None if mask is None else mask.to(backend.dev),
                               mask21=None if mask is None else mask.to(backend.dev), weight=0.5)['loss_feat']
    want = (O.cosine_sim_loss_general(p1, z2, mask, **kw) * 0.5 + O.cosine_sim_loss_general(p2, z1, mask, **kw) * 0.5) * 0.5
    assert relerr(mine.cpu(), want) < 1e-5


def test_frame_level_head_keeps_its_launches(backend, monkeypatch):
    """SimSiamHead's recorded step: its own loss entry points, nothing of the dense path"""
    monkeypatch.setenv('VFS_TAPE', '1')
    monkeypatch.setenv('VFS_GRAPHS', '0')
    model = _mine(True, head='SimSiamHead').to(backend.dev).train()
    imgs = O.fill_tensor(IMGS, seed=11, scale=2.0).to(backend.dev)
    for _ in range(3):      # two eager steps (the buffers settle), then the recording pass
        _step(model, imgs)
    fwd, bwd = [op[0] for op in model._gs.fwd.ops], [op[0] for op in model._gs.bwd.ops]
    assert 'cosine_loss_fwd' in fwd and 'avgpool_fwd' in fwd and fwd.index('cosine_loss_fwd') == fwd.index('loss_means') - 1
    assert 'cosine_loss_bwd' in bwd and bwd.index('cosine_loss_bwd') < bwd.index('avgpool_bwd')
    assert not [n for n in fwd + bwd if n is not None and n.startswith('dense_')]
