"""Label-propagation kernels vs the oracle's restatement of masked_attention_efficient /
post-processing on identical inputs.  backend=emu (CPU) / gpu (MI355X)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vfs_oracle as O
from tests.test_labelprop_exact import l2norm_rule, post_explained


def _bank(T, H, W, C, CO, seed):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(T, H * W, C, generator=g)
    # spatially smooth-ish features so the top-k is not pure noise
    feats = feats + 2.0 * torch.randn(1, 1, C, generator=g) + torch.linspace(0, 3, H * W)[None, :, None] * torch.randn(1, 1, C, generator=g)
    seg = torch.rand(T, H * W, CO, generator=g)
    return feats, seg


def run_labelprop_case(be, T, H, W, C, CO, radius, slots, qframe, topk=10, seed=0):
    lib = be.hostlib
    feats, seg = _bank(T, H, W, C, CO, seed)
    fb = torch.empty(T, H * W, C, dtype=torch.bfloat16)
    xin = feats.to(torch.bfloat16)
    lib.l2norm_rows(xin, fb, T * H * W, C, None)
    # every element: a bf16 neighbour of the float64 quotient, and the nearest one outside the kernel's fp32 error band
    l2norm_rule(xin.reshape(T * H * W, C), fb.reshape(T * H * W, C), f'l2norm {T}x{H}x{W}x{C}')
    out = torch.full((H * W, CO), float('nan'))
    ks = (ctypes.c_int * len(slots))(*slots)
    ws = torch.zeros(96 * H * W * 10 * 2)       # vfs_labelprop_workspace_bytes
    lib.labelprop(fb, seg, out, ws, ws.numel() * ws.element_size(), qframe, ks, len(slots), H, W, C, CO, radius, 0, topk, 0.07, None)
    # oracle on the SAME normalised bf16 features (normalize=False), reference tensor layout, fp64
    fn = fb.double()
    q = fn[qframe].t().reshape(1, C, H, W)
    k = torch.stack([fn[s].t().reshape(C, H, W) for s in slots], dim=1)[None]
    v = torch.stack([seg[s].t().reshape(CO, H, W) for s in slots], dim=1)[None].double()
    mask = O.spatial_neighbor_circle(H, W, 2 * radius) if radius > 0 else None
    ref = O.masked_attention_efficient(q, k, v, mask, 0.07, topk, normalize=False)
    ref = ref[0].reshape(CO, H * W).t().float()
    assert torch.isfinite(out).all()
    err = (out - ref).abs().max(dim=1)[0]
    bad = torch.nonzero(err > 2e-4).flatten()
    # A different fp32 summation order may legitimately swap the 10th and 11th candidate when they
    # are (nearly) tied -- torch.topk itself leaves ties unspecified.  Every query that differs
    # must be explained by such a near-tie in the exact (fp64) scores.
    assert len(bad) < 0.05 * H * W + 1, len(bad)
    if len(bad):
        kv = k[0].reshape(C, -1)                                   # [C, T*HW]
        sc = (kv.t() @ q[0].reshape(C, -1)[:, bad]) / 0.07         # [T*HW, nbad]
        if mask is not None:
            sc.masked_fill_(~mask[:, bad].repeat(len(slots), 1), float('-inf'))
        top = sc.topk(topk + 1, dim=0)[0]
        gap = top[topk - 1] - top[topk]
        assert (gap < 2e-4).all(), (float(gap.max()), int((gap >= 2e-4).sum()))
    return out


@pytest.mark.parametrize('case', [
    dict(T=6, H=12, W=16, C=64, CO=3, radius=4, slots=[0, 1, 2, 3, 4], qframe=5),
    dict(T=4, H=9, W=13, C=128, CO=5, radius=3, slots=[0, 0, 1, 2], qframe=3),       # duplicated first frame, ragged tiles
    dict(T=3, H=8, W=8, C=64, CO=2, radius=0, slots=[0, 1], qframe=2, topk=5),       # no spatial mask
    dict(T=3, H=20, W=28, C=64, CO=3, radius=6, slots=[0, 1], qframe=2),             # several 128-key blocks per window
])
def test_labelprop_matches_oracle(backend, case):
    run_labelprop_case(backend, **case)


@pytest.mark.gpu
@pytest.mark.parametrize('C,radius', [(256, 12), (1024, 18)])
def test_labelprop_davis_size(gpu_backend, C, radius):
    """DAVIS feature size 60x107 (480x854 / 8), R18 (C=256, r=12) and R50 (C=1024, r=18) settings,
    5 key frames incl. the duplicated first frame."""
    run_labelprop_case(gpu_backend, T=5, H=60, W=107, C=C, CO=4, radius=radius, slots=[0, 0, 1, 2, 3], qframe=4)


def test_seg_postprocess_and_onehot(backend):
    lib = backend.hostlib
    g = torch.Generator().manual_seed(1)
    H, W, CO, Ho, Wo = 12, 16, 4, 96, 128
    seg = torch.rand(H * W, CO, generator=g)
    seg[:, 3] = -seg[:, 3]            # a channel whose max is <= 0 stays un-normalised
    partial = torch.zeros(64 * CO * 2)
    lab = torch.zeros(Ho, Wo, dtype=torch.uint8)
    lib.seg_postprocess(seg, partial, lab, H, W, CO, Ho, Wo, None)
    want = O.seg_postprocess(seg.t().reshape(1, CO, H, W), (Ho, Wo))[0]
    # fp32 rounding can flip near-ties between channels and nothing else: every label that is not the float64 argmax must be such
    # a near-tie (tests/test_labelprop_exact.py, 3.), and the labels differ from the fp32 oracle's no more often than those occur
    off64, near = post_explained(seg.numpy(), H, W, Ho, Wo, lab.numpy(), 'seg_postprocess 12x16 -> 96x128')
    post_explained(seg.numpy(), H, W, Ho, Wo, want.numpy(), 'the fp32 oracle, 12x16 -> 96x128')
    mism = float((lab != want).float().mean())
    assert mism <= min(near, 1e-3), (mism, off64, near)
    labels = torch.randint(0, CO, (H * W,), generator=g).to(torch.uint8)
    oh = torch.zeros(H * W, CO)
    lib.onehot(labels, oh, H * W, CO, None)
    assert torch.equal(oh, F.one_hot(labels.long(), CO).float())


def test_forward_test_matches_reference_golden_labels(backend):
    """VanillaTracker.forward_test with test_cfg.precision='bf16' (the fast mode) vs the uint8 label maps captured from
    the REAL reference (tests/golden/forward_test_r18.npz: fp32 torch).  Features are bf16 here, so agreement is
    statistical (labels flip only where the top-2 classes are close); the default fp32 mode is held to 100 % in
    tests/test_exact_f32.py."""
    import os
    import vfs_amd
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'forward_test_r18.npz'))
    cfg = vfs_amd.Config.fromfile(os.path.join(os.path.dirname(os.path.dirname(__file__)), 'configs', 'vfs_r18.py'))
    tc = vfs_amd.ConfigDict(cfg.test_cfg)
    tc['neighbor_range'], tc['precede_frames'], tc['precision'] = 8, 3, 'bf16'      # the fast mode (fp32 default: test_exact_f32.py)
    bb = dict(cfg.model['backbone'])
    bb['out_indices'], bb['strides'] = tc['out_indices'], tc['strides']          # tools/test.py:129-133
    model = vfs_amd.build_model(dict(type='VanillaTracker', backbone=bb), train_cfg=None, test_cfg=tc)
    ref = O.VanillaTracker(18, dict(tc))
    O.fill_state_dict_(ref, seed=5)
    sd = {k: v for k, v in ref.state_dict().items()}
    missing = model.load_state_dict(sd, strict=False)
    assert not [k for k in missing.missing_keys if 'iteration' not in k]
    model.to(backend.dev).eval()
    T, H, W = 6, 96, 128
    imgs = O.fill_tensor([1, 1, 3, T, H, W], 41, scale=2.0)
    seg = torch.from_numpy(g['ref_seg'])[None]
    out = model(imgs.to(backend.dev), return_loss=False, ref_seg_map=seg, img_meta=[dict(original_shape=(H, W, 3))])
    assert isinstance(out, list) and out[0].shape == (T, H, W) and out[0].dtype == np.uint8
    want = g['seg_preds']
    assert (out[0][0] == want[0]).all()                      # frame 0: resized ground truth
    agree = (out[0] == want).mean()
    assert agree > 0.97, agree
    # ... and (near-)bit-exact against the oracle when it is fed the HIP path's own feature bank
    from vfs_amd.labelprop import extract_features
    bank, h, w, C = extract_features(model, backend.eng, imgs.reshape(1, 3, T, H, W).to(backend.dev), 10, precision='bf16')
    feats = bank.float().cpu().permute(2, 0, 1).reshape(1, C, T, h, w)
    lab = O.label_propagate(feats, g['ref_seg'], (H, W), precede_frames=3, topk=10, temperature=0.07,
                            neighbor_range=8, with_first=True, normalize=False)
    mism = (out[0] != lab).mean()
    assert mism < 2e-3, mism


def test_forward_test_all_blocks(backend):
    """test_cfg.all_blocks=True: the list holds ONE array [num_blocks, T, H, W] (vanilla_tracker.py:199-205);
    statistical agreement with the reference's fp32 labels per block, last block = the single-feature path"""
    import os
    import vfs_amd
    if backend.name == 'emu':
        pytest.skip('the bf16 all_blocks clip takes 20 s on the emulator; the GPU runs it (the fp32 all_blocks test covers the emulator)')
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'forward_test_r18_all_blocks.npz'))
    cfg = vfs_amd.Config.fromfile(os.path.join(os.path.dirname(os.path.dirname(__file__)), 'configs', 'vfs_r18.py'))
    tc = vfs_amd.ConfigDict(cfg.test_cfg)
    tc['neighbor_range'], tc['precede_frames'], tc['all_blocks'], tc['precision'] = 8, 3, True, 'bf16'
    bb = dict(cfg.model['backbone'])
    bb['out_indices'], bb['strides'] = tc['out_indices'], tc['strides']
    model = vfs_amd.build_model(dict(type='VanillaTracker', backbone=bb), train_cfg=None, test_cfg=tc)
    ref = O.VanillaTracker(18, dict(tc))
    O.fill_state_dict_(ref, seed=5)
    model.load_state_dict(ref.state_dict(), strict=False)
    model.to(backend.dev).eval()
    T, H, W = 6, 96, 128
    imgs = O.fill_tensor([1, 1, 3, T, H, W], 41, scale=2.0).to(backend.dev)
    seg = torch.from_numpy(g['ref_seg'])[None]
    meta = [dict(original_shape=(H, W, 3))]
    out = model(imgs, return_loss=False, ref_seg_map=seg, img_meta=meta)
    assert isinstance(out, list) and len(out) == 1 and out[0].shape == (2, T, H, W) and out[0].dtype == np.uint8
    for b in range(2):
        assert (out[0][b][0] == g['seg_preds'][b][0]).all()
        assert (out[0][b] == g['seg_preds'][b]).mean() > 0.97
    model.test_cfg['all_blocks'] = False
    single = model(imgs, return_loss=False, ref_seg_map=seg, img_meta=meta)
    assert np.array_equal(single[0], out[0][1])

