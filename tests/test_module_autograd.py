"""Module-level autograd (vfs_amd/autograd.py): ResNet.forward, SimSiamHead.forward and DenseSimSiamHead.forward in train mode
carry a grad_fn and backward() runs the HIP backward - the reference's own loop, `x = backbone(imgs); z, p = head(x);
loss.backward()`.  ResNet-18, N = 2, 64 x 64 inputs (a few seconds on the emulator as well, so nothing here skips it)."""
import functools
import gc

import pytest
import torch

from oracle import vfs_oracle as O
from tests.dense_head_oracle import DenseHead
from tests.test_emu_train_step import _freeze_like_reference, _l2rel
from vfs_amd.engine import BF16

HEAD_KW = dict(in_channels=512, projection_mid_channels=512, projection_out_channels=512, predictor_mid_channels=128, predictor_out_channels=512)
STAGE_C = {0: 64, 1: 128, 2: 256, 3: 512}


@functools.lru_cache(maxsize=None)
def _ref_state(seed=118):
    ref = O.ResNet(18, zero_init_residual=False)
    O.fill_state_dict_(ref, seed=seed)
    return ref.state_dict()


def _net(dev, out_indices=(3,), seed=118, **kw):
    from vfs_amd.resnet import ResNet
    net = ResNet(18, out_indices=out_indices, zero_init_residual=False, **kw)
    net.load_state_dict(_ref_state(seed))
    return net.to(dev).train()


def _x(seed=11):
    return O.fill_tensor([2, 3, 64, 64], seed, scale=2.0)


def _cot(stage, seed):
    side = 64 // (4 * 2 ** stage)
    return O.fill_tensor([2, STAGE_C[stage], side, side], seed, scale=1.0)


def _nhwc(g):
    return g.permute(0, 2, 3, 1).contiguous().to(BF16)


def _zero_grads(mod):
    for p in mod.parameters():
        if p.requires_grad:
            p.grad = torch.zeros_like(p)


def _hand_backward(backend, net, x, grads):
    """the parent's path: forward_nhwc / backward_nhwc by hand, {stage: bf16 NHWC}"""
    eng, dev = backend.eng, backend.dev
    net.attach(eng)
    eng.pack_weights()
    N, _, H, W = x.shape
    x4 = eng.buf('backbone.x4', (N, H, W, 4), BF16, dev)
    eng.lib.imgs_to_nhwc4(x.to(dev).contiguous(), x4, N, 1, 1, H, W, W, eng.stream(dev))
    outs, ctx = net.forward_nhwc(eng, x4, N, H, W, 1, True)
    _zero_grads(net)
    net.backward_nhwc(eng, ctx, {s: g.to(dev) for s, g in grads.items()})
    eng.wgrad_join(dev)
    return outs


def _assert_same_grads(a, b):
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert pa.keys() == pb.keys()
    for n in pa:
        assert (pa[n].grad is None) == (pb[n].grad is None), n
        if pa[n].grad is not None:
            assert torch.equal(pa[n].grad, pb[n].grad), n


def test_train_mode_forward_is_differentiable(backend):
    """fails on the parent: no grad_fn there"""
    net = _net(backend.dev)
    y = net(_x().to(backend.dev))
    assert y.requires_grad and y.dtype == torch.float32 and tuple(y.shape) == (2, 512, 2, 2)
    y.float().pow(2).mean().backward()
    for g in (net.conv1.conv.weight.grad, net.layer4[1].conv2.bn.weight.grad):
        assert g is not None and torch.isfinite(g).all() and float(g.abs().sum()) > 0


def test_forward_bits_and_running_statistics(backend):
    a, b = _net(backend.dev), _net(backend.dev)
    x = _x().to(backend.dev)
    ya = a(x)
    with torch.no_grad():
        yb = b(x)
    assert ya.requires_grad and not yb.requires_grad and torch.equal(ya.detach(), yb)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert int(sa['layer4.1.conv2.bn.num_batches_tracked']) == 1
    # untouched: eval mode, and a fully frozen net in train mode
    assert not a.eval()(x).requires_grad
    for p in b.parameters():
        p.requires_grad = False
    assert not b.train()(x).requires_grad
    with pytest.raises(RuntimeError, match='ResNet.forward is the inference entry point'):
        a.train()(x.clone().requires_grad_())


@pytest.mark.parametrize('kw', [dict(), dict(frozen_stages=2, norm_eval=True)], ids=['plain', 'frozen2-norm_eval'])
def test_single_stage_backward_is_the_hand_driven_path(backend, kw):
    net, twin = _net(backend.dev, **kw), _net(backend.dev, **kw)
    G = _cot(3, 5)
    net(_x().to(backend.dev)).backward(G.to(backend.dev))
    _hand_backward(backend, twin, _x(), {3: _nhwc(G)})
    _assert_same_grads(net, twin)
    for n, p in net.named_parameters():
        frozen = bool(kw) and n.startswith(('conv1.', 'layer1.', 'layer2.'))
        assert (p.grad is None) == frozen, n
    assert float(net.layer3[0].conv1.conv.weight.grad.abs().sum()) > 0


def test_several_stages_exact_cases(backend):
    idx = (1, 3)
    G1, G3 = _cot(1, 6), _cot(3, 7)
    x = _x().to(backend.dev)
    # y1 alone == backward_nhwc(grads={1: ...}) on a twin; layers 3 and 4 are not walked: their gradients are the zeros that the
    # backward gives every trainable parameter without one (all-zero, not None)
    net, twin = _net(backend.dev, idx), _net(backend.dev, idx)
    y1, y3 = net(x)
    y1.backward(G1.to(backend.dev))
    _hand_backward(backend, twin, _x(), {1: _nhwc(G1)})
    _assert_same_grads(net, twin)
    for n, p in net.named_parameters():
        if n.startswith(('layer3.', 'layer4.')):
            assert p.grad is not None and not p.grad.any(), n
    assert float(net.layer2[1].conv2.conv.weight.grad.abs().sum()) > 0
    # an exact zero at the join changes nothing
    a, b = _net(backend.dev, idx), _net(backend.dev, idx)
    ya1, ya3 = a(x)
    torch.autograd.backward([ya1, ya3], [0 * G1.to(backend.dev), G3.to(backend.dev)])
    yb1, yb3 = b(x)
    yb3.backward(G3.to(backend.dev))
    _assert_same_grads(a, b)
    # ... and bf16 NHWC operands join in backward_nhwc too (vfs_bf16_add): a zero there changes nothing either
    c = _net(backend.dev, idx)
    _hand_backward(backend, c, _x(), {1: torch.zeros(2, 8, 8, 128, dtype=BF16), 3: _nhwc(G3)})
    _assert_same_grads(c, b)
    # a non-zero join, exactly: with a cotangent that is a bf16 value already, the fp32 join (vfs_nchw_f32_add_nhwc_bf16, through
    # autograd) and the bf16 join (vfs_bf16_add, by hand) round the same fp32 sum - every gradient behind the join has the same bits,
    # and they differ from the y3-only ones
    G1b = O.round_bf16(G1)
    d, e = _net(backend.dev, idx), _net(backend.dev, idx)
    yd1, yd3 = d(x)
    torch.autograd.backward([yd1, yd3], [G1b.to(backend.dev), G3.to(backend.dev)])
    _hand_backward(backend, e, _x(), {1: _nhwc(G1b), 3: _nhwc(G3)})
    _assert_same_grads(d, e)
    assert not torch.equal(d.layer2[0].conv1.conv.weight.grad, b.layer2[0].conv1.conv.weight.grad)
    assert torch.equal(d.layer3[0].conv1.conv.weight.grad, b.layer3[0].conv1.conv.weight.grad)      # in front of the join: G3 alone


@functools.lru_cache(maxsize=None)
def _oracle_two_stage_grads(emulate, norm_eval=False):
    ref = O.ResNet(18, zero_init_residual=False, out_indices=(1, 3))
    ref.load_state_dict(_ref_state())
    ref.train()
    _freeze_like_reference(ref, norm_eval=norm_eval)
    for m in ref.modules():
        if hasattr(m, 'emulate_bf16'):
            m.emulate_bf16 = emulate
    x = O.round_bf16(_x()) if emulate else _x()
    y1, y3 = ref(x)
    G1, G3 = _cot(1, 6), _cot(3, 7)
    torch.autograd.backward([y1, y3], [O.round_bf16(G1), O.round_bf16(G3)] if emulate else [G1, G3])
    return {n: p.grad.clone() for n, p in ref.named_parameters()}


@pytest.mark.parametrize('norm_eval', [False, True], ids=['batch-stats', 'norm_eval'])
def test_several_stages_against_the_oracle(backend, norm_eval):
    """both cotangents non-zero; the yardstick of tests/test_siamfc_finetune.py: err_hip < max(2 err_emul, 2e-2) in relative L2
    over all gradients and per stage, err_emul = the oracle's own bf16 emulation against its fp32 run.  With batch statistics a
    BatchNorm batch of this input is 8 values per channel at stage 3 and the emulation itself sits far from fp32 (a wide bar);
    norm_eval=True takes the batch statistics out - running statistics, fixed coefficients - and the emulation, and with it the
    bar on the join and on everything behind it, comes down to about a third (what is left is bf16 storage flipping ReLU masks
    on maps this small).  The join's VALUE is checked exactly in test_several_stages_exact_cases"""
    net = _net(backend.dev, (1, 3), norm_eval=norm_eval)
    y1, y3 = net(_x().to(backend.dev))
    torch.autograd.backward([y1, y3], [_cot(1, 6).to(backend.dev), _cot(3, 7).to(backend.dev)])
    want, emul = _oracle_two_stage_grads(False, norm_eval), _oracle_two_stage_grads(True, norm_eval)
    mine = {n: p.grad.cpu() for n, p in net.named_parameters()}
    assert mine.keys() == want.keys()
    for prefix in ('', 'conv1.', 'layer1.', 'layer2.', 'layer3.', 'layer4.'):
        ks = [k for k in sorted(want) if k.startswith(prefix)]
        gm, gw, ge = (torch.cat([d[k].flatten() for k in ks]) for d in (mine, want, emul))
        assert torch.isfinite(gm).all() and float(gw.norm()) > 0
        err_hip, err_emul = _l2rel(gm, gw), _l2rel(ge, gw)
        print(f'two-stage gradients ({"norm_eval" if norm_eval else "batch statistics"}) {prefix or "all"}: rel-L2 {err_hip:.3e}, emulation {err_emul:.3e}')
        assert err_hip < max(2.0 * err_emul, 2e-2), (prefix, err_hip, err_emul)


def test_two_live_passes_and_the_tag_pool(backend):
    from vfs_amd import autograd
    dev = backend.dev
    x1, x2, Ga, Gb = _x(11).to(dev), _x(12).to(dev), _cot(3, 8).to(dev), _cot(3, 9).to(dev)
    net, seq = _net(dev), _net(dev)
    a = net(x1)
    b = net(x2)
    torch.autograd.backward([a], [Ga])
    torch.autograd.backward([b], [Gb])
    seq(x1).backward(Ga)
    seq(x2).backward(Gb)
    # (forward x1, forward x2 leaves other running statistics than the interleaved order only through the order of the updates:
    # both nets saw x1 then x2)
    _assert_same_grads(net, seq)
    for k, v in net.state_dict().items():
        assert torch.equal(v, seq.state_dict()[k]), k
    with pytest.raises(RuntimeError, match='second time'):
        a.backward(Ga)
    assert autograd.LIVE_LIMIT == 4
    live = [net(x1) for _ in range(4)]
    with pytest.raises(RuntimeError, match='4 grad-mode forwards are alive'):
        net(x1)
    del live[0]
    gc.collect()
    y = net(x1)      # a tag came back with the collected context
    y.backward(Ga, retain_graph=True)
    with pytest.raises(RuntimeError, match='second time'):
        y.backward(Ga)
    del live, y
    gc.collect()
    assert len(autograd.live_pool(backend.eng, 'backbone').free) == 4


@pytest.mark.parametrize('kw', [dict(), dict(norm_eval=True)], ids=['plain', 'norm_eval'])
def test_two_instances_alive_at_once(backend, kw):
    """two nets of one class under one loss: the engine's buffers are keyed by name, so the second forward must take another tag
    (activations, masks, batch AND eval-mode BatchNorm coefficients of the first stay intact).  Bit for bit the sequential order."""
    dev = backend.dev
    x, Ga, Gb = _x().to(dev), _cot(3, 8).to(dev), _cot(3, 9).to(dev)
    n1, n2 = _net(dev, seed=118, **kw), _net(dev, seed=119, **kw)
    s1, s2 = _net(dev, seed=118, **kw), _net(dev, seed=119, **kw)
    a = n1(x)
    b = n2(x)
    assert not torch.equal(a.detach(), b.detach())
    torch.autograd.backward([a, b], [Ga, Gb])
    s1(x).backward(Ga)
    s2(x).backward(Gb)
    _assert_same_grads(n1, s1)
    _assert_same_grads(n2, s2)
    assert float(n1.layer1[0].conv1.conv.weight.grad.abs().sum()) > 0
    # the pool is the namespace's: four forwards over two instances exhaust it
    live = [n1(x), n2(x), n1(x), n2(x)]
    with pytest.raises(RuntimeError, match='4 grad-mode forwards are alive'):
        n2(x)
    del live
    gc.collect()


def test_two_head_instances_alive_at_once(backend):
    """SimSiamHead and DenseSimSiamHead share the 'img_head' buffer names: three heads alive under one backward"""
    dev = backend.dev
    (Gz, Gp), (Dz, Dp) = _head_cots(False), _head_cots(True)
    mk = lambda: (_head(dev, False, 21)[0], _head(dev, False, 22)[0], _head(dev, True, 23)[0])      # noqa: E731
    (h1, h2, hd), (t1, t2, td) = mk(), mk()
    x, xd = _feat(False).to(dev), _feat(True).to(dev)
    (z1, p1), (z2, p2), (zd, pd) = h1(x), h2(x), hd(xd)
    torch.autograd.backward([z1, p1, z2, p2, zd, pd], [c.to(dev) for c in (Gz, Gp, Gp, Gz, Dz, Dp)])
    for t, xx, cots in ((t1, x, (Gz, Gp)), (t2, x, (Gp, Gz)), (td, xd, (Dz, Dp))):
        torch.autograd.backward(list(t(xx)), [c.to(dev) for c in cots])
    for h, t in ((h1, t1), (h2, t2), (hd, td)):
        _assert_same_grads(h, t)


# ---------------------------------------------------------------------------------------------------------------- heads
def _head(dev, dense, seed=21):
    import vfs_amd
    kw = {k.replace('_fcs', '_convs'): v for k, v in HEAD_KW.items()} if dense else HEAD_KW
    head = vfs_amd.build_head(dict(type='DenseSimSiamHead' if dense else 'SimSiamHead', **kw))
    ref = DenseHead(**kw) if dense else O.SimSiamHead(**kw)
    O.fill_state_dict_(ref, seed=seed)
    head.load_state_dict(ref.state_dict())
    return head.to(dev).train(), ref.train()


def _feat(dense):
    return O.fill_tensor([4, 512, 4, 4] if dense else [4, 512, 2, 2], 31, scale=1.5)


def _head_cots(dense):
    shape = [4, 512, 4, 4] if dense else [4, 512]
    return O.fill_tensor(shape, 32, scale=1.0), O.fill_tensor(shape, 33, scale=1.0)


@pytest.mark.parametrize('dense', [False, True], ids=['SimSiamHead', 'DenseSimSiamHead'])
def test_head_p_cotangent_is_the_hand_driven_path(backend, dense):
    dev, eng = backend.dev, backend.eng
    head, _ = _head(dev, dense)
    twin, _ = _head(dev, dense)
    _, Gp = _head_cots(dense)
    x = _feat(dense).to(dev).requires_grad_()
    z, p = head(x)
    assert z.requires_grad and p.requires_grad and z.shape == p.shape == Gp.shape
    p.backward(Gp.to(dev))
    N, C, h, w = x.shape
    twin.attach(eng)
    eng.pack_weights()
    tz, tp, ctx = twin.forward_nhwc(eng, _nhwc(_feat(dense)).to(dev), N, h, w, C, 1, True)
    assert torch.equal(tz.float().cpu(), (z.permute(0, 2, 3, 1) if dense else z).detach().cpu())
    _zero_grads(twin)
    gfeat = twin.backward_nhwc(eng, ctx, (_nhwc(Gp) if dense else Gp.to(BF16)).to(dev))
    eng.wgrad_join(dev)
    _assert_same_grads(head, twin)
    want = torch.empty(N, C, h, w, device=dev)
    eng.lib.nhwc_bf16_to_nchw_f32(gfeat, want, N, h * w, C, eng.stream(dev))
    assert torch.equal(x.grad, want) and float(x.grad.abs().sum()) > 0
    assert torch.equal(want.cpu(), gfeat.float().cpu().permute(0, 3, 1, 2))


@pytest.mark.parametrize('dense', [False, True], ids=['SimSiamHead', 'DenseSimSiamHead'])
def test_head_z_and_p_cotangents_against_autograd(backend, dense):
    """cotangents on both outputs against fp32 torch autograd over the oracle's restatement of the layers; bars: gradients
    `mine <= 2.0 * emu + 5e-3` relative L2 with emu = the bf16-storage emulation against fp32 (tests/test_emu_train_step.py:90,
    tests/test_dense_head.py:130 and :138), a gradient that is exactly 0 in fp32 below 5e-3 (tests/test_emu_train_step.py:86)"""
    dev = backend.dev
    head, ref = _head(dev, dense)
    Gz, Gp = _head_cots(dense)
    x = _feat(dense).to(dev).requires_grad_()
    z, p = head(x)
    torch.autograd.backward([z, p], [Gz.to(dev), Gp.to(dev)])
    res = {}
    for emulate in (False, True):
        _, r = _head(torch.device('cpu'), dense)
        r.set_emulate_bf16(True) if (dense and emulate) else None
        if emulate and not dense:
            for m in r.modules():
                if hasattr(m, 'emulate_bf16'):
                    m.emulate_bf16 = True
        xr = (O.round_bf16(_feat(dense)) if emulate else _feat(dense)).requires_grad_()
        rz, rp = r(xr)
        torch.autograd.backward([rz, rp], [O.round_bf16(Gz), O.round_bf16(Gp)] if emulate else [Gz, Gp])
        res[emulate] = dict({n: q.grad for n, q in r.named_parameters()}, x=xr.grad, z=rz.detach(), p=rp.detach())
    mine = dict({n: q.grad.cpu() for n, q in head.named_parameters()}, x=x.grad.cpu())
    assert mine.keys() | {'z', 'p'} == res[False].keys()
    failed = []
    for n, g in mine.items():
        want, emu = res[False][n], res[True][n]
        assert torch.isfinite(g).all(), n
        if want.norm() < 1e-6:      # biases in front of a BatchNorm: exactly 0 in fp32
            assert g.norm() < 5e-3, (n, float(g.norm()))
            continue
        e_hip, e_emu = _l2rel(g, want), _l2rel(emu, want)
        print(f'{n}: rel-L2 {e_hip:.3e}, emulation {e_emu:.3e}')
        if not e_hip <= 2.0 * e_emu + 5e-3:
            failed.append((n, e_hip, e_emu))
    assert not failed, failed


@pytest.mark.parametrize('dense', [False, True], ids=['SimSiamHead', 'DenseSimSiamHead'])
def test_head_frozen_or_eval_layer_is_refused_by_name(backend, dense):
    head, _ = _head(backend.dev, dense)
    x = _feat(dense).to(backend.dev)
    bn = 'projection_convs.1.bn' if dense else 'projection_fcs.1'
    head.get_submodule(bn).eval()
    with pytest.raises(NotImplementedError, match=bn.replace('.', r'\.') + ': BatchNorm in eval mode'):
        head(x)
    head.train()
    w = 'predictor_convs.1.conv.weight' if dense else 'predictor_fcs.3.weight'
    head.get_parameter(w).requires_grad = False
    with pytest.raises(NotImplementedError, match=w.replace('.', r'\.') + ': requires_grad=False'):
        head(x)
    with torch.no_grad():      # the inference entry point stays open
        z, p = head(x)
    assert not z.requires_grad and torch.isfinite(p).all()


def test_z_detach_and_unused_outputs(backend):
    """z.detach() in user code yields no dz; a head whose p is unused trains its projector only"""
    head, _ = _head(backend.dev, False)
    twin, _ = _head(backend.dev, False)
    Gz, Gp = _head_cots(False)
    x = _feat(False).to(backend.dev)
    z, p = head(x)
    (p * Gp.to(backend.dev)).sum().add((z.detach() * Gz.to(backend.dev)).sum()).backward()
    z2, p2 = twin(x)
    p2.backward(Gp.to(backend.dev))
    _assert_same_grads(head, twin)
    third, _ = _head(backend.dev, False)
    z3, _ = third(x)
    z3.backward(Gz.to(backend.dev))
    assert not third.predictor_fcs[0].weight.grad.any() and float(third.projection_fcs[0].weight.grad.abs().sum()) > 0


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.gpu
def test_reference_loop_matches_the_fused_step(gpu_backend):
    """SimSiamBaseTracker's losses written with module calls (sim_siam_base_tracker.py:31-56) against the fused forward_train on
    the same weights and images: the loss within the 2e-2 relative bar of smoke(); every trainable parameter gets a finite
    gradient.  (Per-view BatchNorm statistics: the same mathematics, other launch shapes - no equal bits.)"""
    import os

    import vfs_amd
    dev = gpu_backend.dev
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = vfs_amd.Config.fromfile(os.path.join(repo, 'configs', 'vfs_r18.py'))
    ref = O.build_tracker(18)
    O.fill_state_dict_(ref, seed=3)
    models = []
    for _ in range(2):
        m = vfs_amd.build_model(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
        m.load_state_dict(ref.state_dict())
        models.append(m.to(dev).train())
    fused, loop = models
    imgs = O.fill_tensor([4, 2, 3, 1, 64, 64], seed=11, scale=2.0).to(dev)
    want = float(fused.train_step(dict(imgs=imgs, label=torch.zeros(4, 1)), None)['log_vars']['loss'])
    imgs1, imgs2 = imgs[:, 0, :, 0].contiguous(), imgs[:, 1, :, 0].contiguous()
    x1, x2 = loop.backbone(imgs1), loop.backbone(imgs2)
    (z1, p1), (z2, p2) = loop.img_head(x1), loop.img_head(x2)
    loss = sum(v.mean() for v in loop.img_head.loss(p1, z1, p2, z2).values())      # _parse_losses (base.py:103-108): the mean of each loss
    assert loss.requires_grad
    got = float(loss.detach())
    print(f'reference loop loss {got:.6f}, fused step {want:.6f}')
    assert abs(got - want) < 2e-2 * max(1.0, abs(want)), (got, want)
    loss.backward()
    for n, p in loop.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert float(loop.backbone.conv1.conv.weight.grad.abs().sum()) > 0 and float(loop.img_head.projection_fcs[0].weight.grad.abs().sum()) > 0
