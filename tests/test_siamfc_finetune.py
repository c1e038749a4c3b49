"""SiamFCProbe with a partly unfrozen dilated backbone (cfg['backbone']['frozen_stages'] < 4; siamfc_tracker_base.py:131-144:
the optimizer holds the backbone too): one train step through the bf16 training path of both branches, the backbone gradients
against the torch oracle (O.ResNet + oracle/siamfc_oracle.py head and loss), the fp32 tracking executor after the step, and
the frozen probe's unchanged loss.  ResNet-18, batch 2, 120 / 255 pixel crops: GPU only (minutes on the emulator)."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import siamfc_oracle as SO
from oracle import vfs_oracle as O
from tests.test_emu_train_step import _freeze_like_reference, _l2rel

ARCH = dict(strides=(1, 2, 1, 1), dilations=(1, 1, 2, 4), out_indices=(3,))
MEAN = torch.tensor((123.675, 116.28, 103.53)).view(1, 3, 1, 1)
STD = torch.tensor((58.395, 57.12, 57.375)).view(1, 3, 1, 1)
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'siamfc_frozen_loss.npz')


def _skip_on_emu(backend):
    if backend.name == 'emu':
        pytest.skip('full ResNet-18 at 120 / 255 pixel crops: minutes on the emulator; runs on the GPU')


def _inputs():
    g = torch.Generator().manual_seed(0)
    return torch.rand(2, 3, 120, 120, generator=g) * 255, torch.rand(2, 3, 255, 255, generator=g) * 255


def _weights():
    ref = O.ResNet(18, zero_init_residual=False, **ARCH)
    O.fill_state_dict_(ref, seed=118)
    head = SO.SiamConvFC(512, 512, out_scale=0.001)
    O.fill_state_dict_(head, seed=21)
    return ref, head


def _probe(dev, frozen_stages, **cfg):
    import vfs_amd
    from vfs_amd.siamfc import DEFAULT_CFG
    cfg = dict(dict(out_channels=512, batch_size=2, exemplar_sz=120, instance_sz=255,
                    backbone=dict(DEFAULT_CFG['backbone'], frozen_stages=frozen_stages)), **cfg)
    probe = vfs_amd.SiamFCProbe(cfg, depth=18, device=dev)
    ref, head = _weights()
    probe.backbone.load_state_dict(ref.state_dict())
    probe.head.load_state_dict(head.state_dict())
    return probe


def _frames():
    frames = []
    for t in range(4):
        img = np.full((240, 320, 3), 60, np.uint8)
        img[100 + 3 * t:140 + 3 * t, 150 + 4 * t:190 + 4 * t] = 220
        frames.append(img)
    return frames


def test_finetune_step_updates_unfrozen_layers_only(backend):
    _skip_on_emu(backend)
    probe = _probe(backend.dev, 2)
    assert probe.finetune and probe.optimizer.param_groups[0]['weight_decay'] == probe.cfg['weight_decay']
    held = {id(p) for grp in probe.optimizer.param_groups for p in grp['params']}
    want = [p for p in list(probe.backbone.parameters()) + list(probe.head.parameters()) if p.requires_grad]
    assert held == {id(p) for p in want} and len(held) == 30 + 4      # layer3 / layer4: 10 convs + 10 BatchNorm affine pairs; the head
    before = {k: v.clone() for k, v in probe.backbone.state_dict().items()}
    hb = {k: v.clone() for k, v in probe.head.state_dict().items()}
    z, x = _inputs()
    loss = probe.train_step((z, x))
    assert np.isfinite(loss)
    assert not probe.backbone.training      # back in eval mode: everything else runs the fp32 executor
    for k, v in probe.backbone.state_dict().items():
        stat = 'running_' in k or 'num_batches_tracked' in k
        if stat or k.startswith(('conv1.', 'layer1.', 'layer2.')):
            assert torch.equal(v, before[k]), k      # frozen prefix, and EVERY running statistic (norm_eval)
        else:
            assert not torch.equal(v, before[k]), k      # layer3 / layer4 conv weights and BatchNorm affines
            assert torch.isfinite(v).all(), k
    for k, v in probe.head.state_dict().items():
        assert not torch.equal(v, hb[k]), k
    l2 = probe.train_step((z, x), backward=False)      # the no-grad fp32 feature pass, on the updated weights
    assert np.isfinite(l2)


@functools.lru_cache(maxsize=None)
def _oracle_grads(emulate):
    """backbone gradients of one step in the oracle: {branches: {name: grad}} for both branches and the exemplar branch alone"""
    ref, head = _weights()
    ref.train()
    _freeze_like_reference(ref, frozen_stages=2, norm_eval=True)
    for m in ref.modules():
        if hasattr(m, 'emulate_bf16'):
            m.emulate_bf16 = emulate
    z, x = _inputs()
    zn, xn = (z - MEAN) / STD, (x - MEAN) / STD
    if emulate:
        zn, xn = O.round_bf16(zn), O.round_bf16(xn)
    zf, xf = ref(zn), ref(xn)
    names = [n for n, p in ref.named_parameters() if p.requires_grad]
    params = [p for n, p in ref.named_parameters() if p.requires_grad]
    out = {}
    for key, xin in (('z', xf.detach()), ('zx', xf)):
        resp = head(zf, xin)
        labels = SO.create_labels(resp.size(), 16, 0, 8)
        loss = SO.focal_loss(resp, labels)
        grads = torch.autograd.grad(loss, params, retain_graph=True)
        out[key] = dict(zip(names, grads))
        out[key + '_loss'] = float(loss.detach())
    return out


@pytest.mark.parametrize('branches', ['zx', 'z'])
def test_finetune_backbone_gradients_match_oracle(backend, branches):
    """the whole backbone gradient of one step against fp32 autograd, the oracle's own bf16 emulation as the yardstick
    (test_dilated_frozen_backbone_matches_oracle): err_hip < max(2 err_emul, floor).  'z': the search branch's gradient
    stops at the head, so only the exemplar pass - the FIRST forward, whose context must survive the second - contributes"""
    _skip_on_emu(backend)
    probe = _probe(backend.dev, 2)
    loss = float(probe.finetune_loss_backward(_inputs(), branches=tuple(branches)).item())
    want, emul = _oracle_grads(False), _oracle_grads(True)
    assert abs(loss - want[branches + '_loss']) < 2e-2 * abs(want[branches + '_loss'])
    mine = dict(probe.backbone.named_parameters())
    keys = sorted(want[branches])
    assert keys and all(k.startswith(('layer3.', 'layer4.')) for k in keys)
    for n, p in mine.items():
        assert (p.grad is not None) == (n in want[branches]), n
    gm = torch.cat([mine[k].grad.cpu().flatten() for k in keys])
    gw = torch.cat([want[branches][k].flatten() for k in keys])
    ge = torch.cat([emul[branches][k].flatten() for k in keys])
    assert torch.isfinite(gm).all() and float(gw.norm()) > 0
    err_hip, err_emul = _l2rel(gm, gw), _l2rel(ge, gw)
    print(f'backbone gradient ({branches}): rel-L2 {err_hip:.3e}, emulation {err_emul:.3e}')
    for stage in ('layer3.', 'layer4.'):
        ks = [k for k in keys if k.startswith(stage)]
        a, b, c = (torch.cat([d[k].flatten() for k in ks]) for d in ({k: mine[k].grad.cpu() for k in ks}, want[branches], emul[branches]))
        print(f'  {stage} rel-L2 {_l2rel(a, b):.3e}, emulation {_l2rel(c, b):.3e}')
    assert err_hip < max(2.0 * err_emul, 2e-2), (err_hip, err_emul)


def test_tracking_after_finetune_step_sees_new_weights(backend):
    """step() bumps the params epoch: the fp32 executor behind features() / track() must refresh its folded weights"""
    _skip_on_emu(backend)
    stepped, fresh = _probe(backend.dev, 2, initial_lr=1e-2), _probe(backend.dev, 2, initial_lr=1e-2)
    z, x = _inputs()
    f0 = stepped.features(z).cpu()
    assert torch.equal(f0, fresh.features(z).cpu())
    b0 = stepped.track(_frames(), [151, 101, 40, 40])
    assert np.array_equal(b0, fresh.track(_frames(), [151, 101, 40, 40]))
    stepped.train_step((z, x))
    f1 = stepped.features(z).cpu()
    assert torch.isfinite(f1).all() and not torch.equal(f1, f0)
    # ... and they are the features of a FRESH probe holding the updated weights
    again = _probe(backend.dev, 2)
    again.backbone.load_state_dict(stepped.backbone.state_dict())
    assert torch.equal(again.features(z).cpu(), f1)
    b1 = stepped.track(_frames(), [151, 101, 40, 40])
    assert b1.shape == (4, 4) and np.isfinite(b1).all()
    assert not np.array_equal(b1, b0)
    assert np.array_equal(fresh.track(_frames(), [151, 101, 40, 40]), b0)


def test_frozen_probe_loss_bits_unchanged(backend):
    """frozen_stages=4 keeps its code path: the losses of two steps on fixed inputs, bit for bit what the commit before the
    fine-tuning path gave on an MI355X (tests/golden/siamfc_frozen_loss.npz)"""
    _skip_on_emu(backend)
    probe = _probe(backend.dev, 4)
    assert not probe.finetune
    held = {id(p) for grp in probe.optimizer.param_groups for p in grp['params']}
    assert held == {id(p) for p in probe.head.parameters()} and probe.optimizer.param_groups[0]['weight_decay'] == 0
    z, x = _inputs()
    losses = np.array([probe.train_step((z, x)), probe.train_step((z, x)), probe.train_step((z, x), backward=False)], np.float64)
    print('frozen probe losses:', [float(v).hex() for v in losses])
    assert np.array_equal(losses, np.load(GOLDEN)['losses'])
