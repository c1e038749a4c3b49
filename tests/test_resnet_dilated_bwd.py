"""Backward of a partly unfrozen DILATED backbone (ResNet.backward_nhwc -> Engine.conv_bwd_dilated) against the fp32 autograd
of the oracle ResNet: parameter gradients of the unfrozen convs and BatchNorm affines, no gradients below the frozen prefix.
norm_eval=True as the SiamFC probe's backbone: every BatchNorm on its running statistics.
backend=emu: host build through the fiber emulator; backend=gpu: libvfs_hip.so on the MI355X."""
import functools

import pytest
import torch

from oracle import vfs_oracle as O
from tests.emu_util import nhwc
from tests.test_emu_train_step import TOY_BARS, _freeze_like_reference, _l2rel, _nchw

ARCH = dict(num_stages=3, strides=(1, 2, 1), dilations=(1, 1, 2), out_indices=(2,))


def _oracle(depth, frozen, x, g, emulate):
    ref = O.ResNet(depth, zero_init_residual=False, **ARCH)
    O.fill_state_dict_(ref, seed=depth + 7)
    with torch.no_grad():      # damp the last BatchNorm of every block (tests/test_emu_train_step.py _filled): a conditioned net
        for m in ref.modules():
            if isinstance(m, O.BasicBlock):
                m.conv2.bn.weight.mul_(0.25)
            elif isinstance(m, O.Bottleneck):
                m.conv3.bn.weight.mul_(0.25)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    ref.train()
    _freeze_like_reference(ref, frozen_stages=frozen, norm_eval=True)
    for m in ref.modules():
        if hasattr(m, 'emulate_bf16'):
            m.emulate_bf16 = emulate
    out = ref(O.round_bf16(x))
    out.backward(g)
    return ref, sd, out.detach()


@functools.lru_cache(maxsize=None)
def _run(backend_name, depth, frozen):
    """one forward + backward of the engine and of the oracle (fp32 and with bf16 emulation), shared by the tests below"""
    import vfs_amd
    backend = _BACKENDS[backend_name]
    eng, dev = backend.eng, backend.dev
    N, H, W = 2, 32, 48
    x = O.fill_tensor([N, 3, H, W], seed=9, scale=2.0)
    cout = 256 * (1 if depth == 18 else 4)
    g = O.round_bf16(O.fill_tensor([N, cout, 4, 6], seed=21, scale=0.5))      # stride 8 at stage 3
    ref, sd, want_out = _oracle(depth, frozen, x, g, emulate=False)
    emu, _, _ = _oracle(depth, frozen, x, g, emulate=True)
    whole = {k: {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None} for k, m in (('fp32', ref), ('bf16', emu))}

    net = vfs_amd.ResNet(depth, frozen_stages=frozen, norm_eval=True, norm_cfg=dict(type='BN', requires_grad=True),
                         zero_init_residual=False, **ARCH)
    net.load_state_dict(sd)
    net.to(dev).train()
    for (n, p), (n2, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert n == n2 and p.requires_grad == q.requires_grad, n
        p.grad = torch.zeros_like(p) if p.requires_grad else None
    assert not any(m.training for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    dilated = [n for n, m in net.conv_modules() if m.conv.dilation[0] != 1]
    assert dilated and all(n.startswith('layer3.') for n in dilated)
    stats = {k: v.clone() for k, v in net.state_dict().items() if 'running' in k or 'num_batches' in k}

    net.attach(eng)
    eng.pack_weights()
    x4 = torch.empty(N, H, W, 4, dtype=torch.bfloat16, device=dev)
    eng.lib.imgs_to_nhwc4(x.to(dev).contiguous(), x4, N, 1, 1, H, W, W, eng.stream(dev))
    outs, ctx = net.forward_nhwc(eng, x4, N, H, W, 1, True)
    act, h, w, c = outs[2]
    assert (h, w, c) == (4, 6, cout)
    net.backward_nhwc(eng, ctx, {2: nhwc(g).to(dev)})
    eng.wgrad_join(dev)
    eng.flush_counters()
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    assert _l2rel(_nchw(act), want_out) < TOY_BARS['out_l2'] * 2      # (the forward is pinned elsewhere; a gross mismatch would void the rest)
    for k, v in net.state_dict().items():      # norm_eval: no running statistic moves
        if k in stats:
            assert torch.equal(v.cpu(), stats[k].cpu()), k
    names = [(ln, bi) for ln in net.res_layers for bi in range(len(getattr(net, ln)))]
    blocks = []
    for (ln, bi), bctx in zip(names, ctx['blocks']):
        gin = eng.bufs.get(f'backbone.{ln}.{bi}.conv1.gin')
        assert all(b is None for b in bctx['act_bn'])      # (no folded input BatchNorm at these sizes: `acts` are activations)
        nconv = len(bctx['raws'])
        gins = [eng.bufs.get(f'backbone.{ln}.{bi}.conv{k + 1}.gin') for k in range(nconv)]
        blocks.append(dict(name=(ln, bi), x=_nchw(bctx['x']), out=_nchw(bctx['out']), gin=None if gin is None else _nchw(gin),
                           acts=[_nchw(a) for a in bctx['acts']], gins=[None if t is None else _nchw(t) for t in gins]))
    grads = {n: (p.grad.cpu().clone() if p.grad is not None else None) for n, p in net.named_parameters()}
    return dict(ref=ref, emu=emu, whole=whole, grads=grads, blocks=blocks, g=g, names=names)


_BACKENDS = {}
CASES = [(18, 1), (50, 2)]


def _per_block(r, oracle):
    """the per-stage comparison of tests/test_emu_train_step.py (_every_stage), with its bars (TOY_BARS): every unfrozen oracle
    block, last to first, is fed the ENGINE'S OWN block input and incoming gradient; output, parameter gradients and the input
    gradient handed to the block below must agree.  -> the checks that missed their bar"""
    names, g_in, failed = r['names'], r['g'], []
    for blk in reversed(r['blocks']):
        ln, bi = blk['name']
        rblk = getattr(oracle, ln)[bi]
        if not any(q.requires_grad for q in rblk.parameters()):
            break
        oracle.zero_grad()
        xb = blk['x'].clone().requires_grad_(True)
        ob = rblk(xb)
        ob.backward(g_in)
        checks = [(f'{ln}.{bi}: out rel-L2', _l2rel(blk['out'], ob), TOY_BARS['out_l2'])]
        for n, q in rblk.named_parameters():
            checks.append((f'{ln}.{bi}.{n}.grad rel-L2', _l2rel(r['grads'][f'{ln}.{bi}.{n}'], q.grad), TOY_BARS['pgrad']))
        below = [q for (l2, b2) in names[:names.index((ln, bi))] for q in getattr(oracle, l2)[b2].parameters()]
        g_next = None
        if any(q.requires_grad for q in below):
            g_next = blk['gin']
            checks.append((f'{ln}.{bi}: input-gradient rel-L2', _l2rel(g_next, xb.grad), TOY_BARS['gin']))
        for name, val, bar in checks:
            print(f'{name}: {val:.3e} (bar {bar:g})')
            if not val < bar:
                failed.append((name, round(val, 4), bar))
        if g_next is None:
            break
        g_in = g_next
    return failed


@pytest.mark.parametrize('depth,frozen', CASES)
def test_dilated_backbone_no_gradient_below_frozen_prefix(backend, depth, frozen):
    _BACKENDS[backend.name] = backend
    r = _run(backend.name, depth, frozen)
    rp = dict(r['ref'].named_parameters())
    seen = 0
    for n, gm in r['grads'].items():
        if not rp[n].requires_grad:
            assert gm is None and n not in r['whole']['fp32'], n
        else:
            assert gm is not None and torch.isfinite(gm).all() and float(gm.abs().max()) > 0, n
            seen += n.startswith('layer3.1.')
    assert seen
    prefix = ['conv1.'] + [f'layer{i}.' for i in range(1, frozen + 1)]
    assert all(gm is None for n, gm in r['grads'].items() if any(n.startswith(p) for p in prefix))


def _per_unit_fp32(r):
    """every unfrozen conv -> BatchNorm unit of the fp32 oracle (O.ResNet's own ConvBN modules, no bf16 emulation), last to first,
    fed the ENGINE'S OWN input activation and the engine's own gradient at the unit's output: parameter gradients of the conv and
    the BatchNorm affine, and the input gradient the engine hands on.  -> the checks that missed their bar"""
    ref, names, failed = r['ref'], r['names'], []
    g_out = r['g']                                        # gradient at the output of the block in hand (the engine's, bf16)
    for blk in reversed(r['blocks']):
        ln, bi = blk['name']
        rblk = getattr(ref, ln)[bi]
        if not any(q.requires_grad for q in rblk.parameters()):
            break
        ref.zero_grad()
        units = [getattr(rblk, f'conv{k + 1}') for k in range(len(blk['gins']))]
        last = len(units) - 1
        below = [q for (l2, b2) in names[:names.index((ln, bi))] for q in getattr(ref, l2)[b2].parameters()]
        need_in = any(q.requires_grad for q in below)
        gm = g_out * (blk['out'] > 0)                     # through the join ReLU, with the ENGINE'S mask
        x0 = blk['x'].clone().requires_grad_(True)
        if rblk.downsample is not None:
            rblk.downsample.raw_bn(x0).backward(gm)
        checks = []
        for k in range(last, -1, -1):
            a_in = x0 if k == 0 else blk['acts'][k - 1].clone().requires_grad_(True)
            g_y = gm if k == last else blk['gins'][k + 1] * (blk['acts'][k] > 0)      # the unit's ReLU, the engine's mask again
            units[k].raw_bn(a_in).backward(g_y)
            if k > 0:
                checks.append((f'{ln}.{bi}.conv{k + 1}: input-gradient rel-L2', _l2rel(blk['gins'][k], a_in.grad), TOY_BARS['gin']))
        for n, q in rblk.named_parameters():
            checks.append((f'{ln}.{bi}.{n}.grad rel-L2', _l2rel(r['grads'][f'{ln}.{bi}.{n}'], q.grad), TOY_BARS['pgrad']))
        if need_in:      # conv1's dgrad + the identity branch (the masked block gradient itself, or the downsample unit's dgrad)
            want = x0.grad + (gm if rblk.downsample is None else 0.0)
            checks.append((f'{ln}.{bi}: input-gradient rel-L2', _l2rel(blk['gin'], want), TOY_BARS['gin']))
        for name, val, bar in checks:
            print(f'{name}: {val:.3e} (bar {bar:g})')
            if not val < bar:
                failed.append((name, round(val, 4), bar))
        if not need_in:
            break
        g_out = blk['gin']
    return failed


@pytest.mark.parametrize('depth,frozen', CASES)
def test_dilated_backbone_backward_matches_fp32_autograd(backend, depth, frozen):
    """parameter gradients of the unfrozen convs and BatchNorm affines (and the input gradients between them) against the
    autograd of the fp32 oracle, with the bars of the per-stage test (TOY_BARS: parameter gradients 4e-2, input gradients 3e-2).

    Cut at the ReLUs: every conv -> BatchNorm unit is compared on the engine's own input and on the engine's own gradient at
    its output, masked with the engine's own ReLU decision.  Reason: those bars were set for a reference that makes the engine's
    ReLU decisions (the bf16-emulating oracle of the per-stage test).  Against un-emulated fp32 a fraction f of activations within
    one bf16 rounding of zero takes the other branch of a ReLU, and each such element carries its whole gradient: the
    relative L2 error of everything behind that ReLU is sqrt(f), whatever the kernels do - f = 0.2-1 % at these 4 x 6 .. 8 x 12 maps
    gives 4-10 % (measured block by block through the ReLUs: up to 1.08e-1, on undilated layers as on dilated ones, and 6-7 % for
    the oracle's own bf16 emulation).  Between two ReLUs conv, BatchNorm (eval) and their gradients are linear in their operands,
    so there the fp32 result is the one correct answer up to bf16 rounding of the operands, and the bars apply as they stand.
    The ReLU decisions themselves are pinned by the two tests that follow (block by block against the bf16-emulating oracle; end
    to end against fp32 with the emulation as yardstick)."""
    _BACKENDS[backend.name] = backend
    failed = _per_unit_fp32(_run(backend.name, depth, frozen))
    assert not failed, failed


@pytest.mark.parametrize('depth,frozen', CASES)
def test_dilated_backbone_backward_matches_bf16_emulating_oracle(backend, depth, frozen):
    """the same comparison with the reference the per-stage test itself uses: the oracle with bf16-storage emulation"""
    _BACKENDS[backend.name] = backend
    failed = _per_block(_run(backend.name, depth, frozen), _run(backend.name, depth, frozen)['emu'])
    assert not failed, failed


@pytest.mark.parametrize('depth,frozen', CASES)
def test_dilated_backbone_whole_gradient_within_emulation_yardstick(backend, depth, frozen):
    """end to end: the whole parameter gradient against fp32 autograd, with the oracle's own bf16 emulation as the yardstick
    (as test_dilated_frozen_backbone_matches_oracle): err_hip < max(2 err_emul, floor)"""
    _BACKENDS[backend.name] = backend
    r = _run(backend.name, depth, frozen)
    keys = sorted(r['whole']['fp32'])
    mine = torch.cat([r['grads'][k].flatten() for k in keys])
    want = torch.cat([r['whole']['fp32'][k].flatten() for k in keys])
    emul = torch.cat([r['whole']['bf16'][k].flatten() for k in keys])
    err_hip, err_emul = _l2rel(mine, want), _l2rel(emul, want)
    print(f'whole gradient: rel-L2 {err_hip:.3e}, emulation {err_emul:.3e}')
    assert err_hip < max(2.0 * err_emul, 2e-2), (err_hip, err_emul)
