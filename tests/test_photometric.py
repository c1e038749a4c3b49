"""Photometric steps of the object-level configs (ColorJitter, RandomGrayScale, RandomGaussianBlur between Flip and
Normalize): host decisions vs the reference's own __call__s (tests/golden/photometric.npz), the two-launch kernel
vs tests/photometric_oracle.py bit-exact (backend = emu on the CPU / gpu), and the pipeline feeding train_step."""
import itertools
import os
import random

import numpy as np
import pytest
import torch

from oracle import pipeline_oracle as PO
from tests import photometric_oracle as PH
from vfs_amd.pipeline import GpuTrainPipeline, pack_photometric

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF_CFG = '/root/reference/configs'
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
F32 = lambda v: int(np.float32(v).view(np.int32))      # noqa: E731

COLOR_STEPS = [dict(type='ColorJitter', brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p=0.8, same_across_clip=False,
                    same_on_clip=False),
               dict(type='RandomGrayScale', p=0.2, same_across_clip=False, same_on_clip=False),
               dict(type='RandomGaussianBlur', p=0.5, same_across_clip=False, same_on_clip=False)]


def color_pipeline(cfg_pipeline, steps=COLOR_STEPS):
    """the shipped config's train_pipeline with the photometric steps inserted after Flip (as the object-level configs)"""
    tp = [dict(s) for s in cfg_pipeline]
    at = [s['type'] for s in tp].index('Flip') + 1
    return tp[:at] + [dict(s) for s in steps] + tp[at:]


def _frames(B, F, Hs, Ws, seed):
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, (B, F, Hs // 4 + 1, Ws // 4 + 1, 3), dtype=np.uint8)
    up = np.repeat(np.repeat(base, 4, axis=2), 4, axis=3)[:, :, :Hs, :Ws]
    return np.clip(up.astype(np.int64) + g.integers(-20, 21, up.shape), 0, 255).astype(np.uint8)


def _pipe(V, T, Ho, Wo, steps=COLOR_STEPS):
    return GpuTrainPipeline([dict(type='RandomResizedCrop', area_range=(0.2, 1.), same_across_clip=False, same_on_clip=False),
                             dict(type='Resize', scale=(Wo, Ho), keep_ratio=False),
                             dict(type='Flip', flip_ratio=0.5, same_across_clip=False, same_on_clip=False)] + list(steps) +
                            [dict(type='Normalize', mean=MEAN, std=STD, to_bgr=False),
                             dict(type='FormatShape', input_format='NCTHW')], V, T)


def oracle_pipeline(frames, boxes, flips, rows, out_hw, V, T, mean=MEAN, std=STD):
    B, F = frames.shape[:2]
    H, W = out_hw
    out = np.empty((B, V, 3, T, H, W), np.float32)
    for b in range(B):
        for f in range(F):
            left, top, right, bottom = boxes[b * F + f]
            img = PO.resize_bilinear_u8(frames[b, f, top:bottom, left:right], W, H)
            if flips[b * F + f]:
                img = np.ascontiguousarray(img[:, ::-1])
            img = PH.apply_packed(img, rows[b * F + f])
            out[b, f // T, :, f % T] = PO.normalize(img, mean, std).transpose(2, 0, 1)
    return out


def run_case(be, B, V, T, Hs, Ws, Ho, Wo, seed, rows=None, boxes=None, flips=None, frames=None):
    """the kernel on `be` vs the oracle, fp32 imgs and bf16 x4 bit for bit; rows=None: decisions sampled"""
    if frames is None:
        frames = _frames(B, V * T, Hs, Ws, seed)
    pipe = _pipe(V, T, Ho, Wo)
    np.random.seed(seed)
    random.seed(seed)
    from vfs_amd import _lib
    prev = _lib._LIB
    _lib.set_lib(be.lib)
    try:
        out = pipe(be.d(torch.from_numpy(frames)), boxes=boxes, flips=flips, photo=rows, want_x4=True)
        if be.dev.type == 'cuda':
            torch.cuda.synchronize()
    finally:
        _lib.set_lib(prev)
    want = oracle_pipeline(frames, out['boxes'], out['flips'], out['photo_rows'], (Ho, Wo), V, T)
    got = out['imgs'].cpu().numpy()
    assert got.shape == want.shape
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:4].tolist())
    Wp = Wo + (Wo & 1)
    x4 = torch.full((V * B * T, Ho, Wp, 4), 7.0, dtype=torch.bfloat16)
    be.hostlib.imgs_to_nhwc4(torch.from_numpy(want), x4, B, V, T, Ho, Wo, Wp, None)
    assert torch.equal(out['x4'].cpu().view(torch.int16), x4.view(torch.int16))
    return out


def _row(order=(), b=1.3, c=0.7, s=1.45, hue=231, gray=0, sigma=None):
    r = np.zeros(8, np.int32)
    r[0] = sum(op << (4 * k) for k, op in enumerate(order))
    r[1], r[2], r[3], r[4], r[5] = F32(b), F32(c), F32(s), hue, gray
    if sigma is not None:
        r[6], r[7] = PH.blur_weights(sigma)
    return r


def _full_boxes(n, Hs, Ws):
    return np.tile(np.asarray([[0, 0, Ws, Hs]], np.int32), (n, 1))


# ------------------------------------------------------------------------------------------------ decisions (CPU)

GOLD_PATH = os.path.join(HERE, 'golden', 'photometric.npz')
GOLD = np.load(GOLD_PATH) if os.path.exists(GOLD_PATH) else None
CASES = sorted({k.split('/')[0] for k in GOLD.files}) if GOLD is not None else []


def _gold_steps(case):
    soc, sac = (bool(v) for v in GOLD[case + '/same'])
    jb, jc, js, jh = (float(v) for v in GOLD[case + '/jitter_args'])
    jp, gp, bp = (float(v) for v in GOLD[case + '/probs'])
    return [dict(type='ColorJitter', brightness=jb, contrast=jc, saturation=js, hue=jh, p=jp, same_across_clip=sac, same_on_clip=soc),
            dict(type='RandomGrayScale', p=gp, same_across_clip=sac, same_on_clip=soc),
            dict(type='RandomGaussianBlur', p=bp, sigma_range=tuple(GOLD[case + '/sigma_range']), same_across_clip=sac,
                 same_on_clip=soc)]


@pytest.mark.parametrize('case', CASES)
def test_decisions_match_reference(case):
    """sample() draws the photometric decisions with the reference's RNG use: apply flags, jitter factors and order, blur
    sigma of every frame the reference's own ColorJitter / RandomGrayScale / RandomGaussianBlur __call__ applied them to"""
    hs, ws, nclips, clip_len, nsamp, seed = (int(v) for v in GOLD[case + '/meta'])
    nf = nclips * clip_len
    pipe = GpuTrainPipeline([dict(type='Resize', scale=(8, 8), keep_ratio=False)] + _gold_steps(case) +
                            [dict(type='Normalize', mean=MEAN, std=STD)], nclips, clip_len)
    np.random.seed(seed)
    random.seed(seed)
    got = [pipe.sample(nf, (hs, ws)) for _ in range(nsamp)]
    ph = {k: np.concatenate([g[2][k] for g in got]) for k in got[0][2]}
    for k in ('jitter', 'gray', 'blur'):
        assert np.array_equal(ph[k], GOLD[case + '/' + k]), k
    jit = ph['jitter'].astype(bool)
    assert np.array_equal(ph['factors'][jit], GOLD[case + '/factors'], equal_nan=True)
    assert np.array_equal(ph['order'][jit], GOLD[case + '/order'])
    assert np.array_equal(ph['sigma'][ph['blur'].astype(bool)], GOLD[case + '/sigma'])
    # the oracle's own restatement draws the same
    np.random.seed(seed)
    random.seed(seed)
    steps = _gold_steps(case)
    j, g, b = steps
    for s in range(nsamp):
        o = PH.sample_photometric(
            nf, clip_len, jitter=dict(ranges=PH.jitter_ranges(j['brightness'], j['contrast'], j['saturation'], j['hue']), p=j['p'],
                                      same_on_clip=j['same_on_clip'], same_across_clip=j['same_across_clip']),
            gray=dict(p=g['p'], same_on_clip=g['same_on_clip'], same_across_clip=g['same_across_clip']),
            blur=dict(p=b['p'], sigma_range=b['sigma_range'], same_on_clip=b['same_on_clip'], same_across_clip=b['same_across_clip']))
        sl = slice(s * nf, (s + 1) * nf)
        assert np.array_equal(o['jitter'], ph['jitter'][sl]) and np.array_equal(o['gray'], ph['gray'][sl])
        assert np.array_equal(o['blur'], ph['blur'][sl])
        assert np.array_equal(PH.pack_photometric(o), pack_photometric({k: v[sl] for k, v in ph.items()}))


@pytest.mark.parametrize('case', CASES)
def test_oracle_pixels_match_reference(case):
    """the oracle, driven by the packed rows of the golden decisions, reproduces the frames the reference's three
    __call__s produced (PIL arithmetic real; grey through the cv2 restatement)"""
    src, want = GOLD[case + '/src'], GOLD[case + '/out']
    rows = pack_photometric(dict(jitter=GOLD[case + '/jitter'], factors=GOLD[case + '/factors_all'], order=GOLD[case + '/order_all'],
                                 gray=GOLD[case + '/gray'], blur=GOLD[case + '/blur'], sigma=GOLD[case + '/sigma_all']))
    for i in range(len(src)):
        assert np.array_equal(PH.apply_packed(src[i], rows[i]), want[i]), i


def test_pipeline_position_rules():
    base = [dict(type='SampleFrames', clip_len=1, num_clips=8), dict(type='Clip2Frame', clip_len=4),
            dict(type='Resize', scale=(32, 24), keep_ratio=False), dict(type='Flip'),
            dict(type='Normalize', mean=MEAN, std=STD, to_bgr=False)]
    ok = GpuTrainPipeline(base[:4] + COLOR_STEPS + base[4:])
    assert ok.photometric and ok.jitter['p'] == 0.8 and ok.gray['p'] == 0.2 and ok.blur['sigma_range'] == (0.1, 0.2)
    for sub in ([0], [1], [2], [0, 2], [1, 2]):
        assert GpuTrainPipeline(base[:4] + [COLOR_STEPS[i] for i in sub] + base[4:]).photometric
    assert not GpuTrainPipeline(base).photometric
    assert GpuTrainPipeline(base[:4] + [dict(type='ColorJitter')] + base[4:]).jitter['ranges'] == [None] * 4
    bad = [base[:2] + COLOR_STEPS[:1] + base[2:],                          # before Resize
           base + COLOR_STEPS[2:],                                         # after Normalize
           base[:4] + COLOR_STEPS[1:2] + COLOR_STEPS[:1] + base[4:],       # out of order
           base[:4] + COLOR_STEPS[:1] * 2 + base[4:],                      # twice
           base[:4] + [dict(type='RandomGaussianBlur', sigma_range=(0.1, 2.0))] + base[4:]]     # box radius >= 1
    for b in bad:
        with pytest.raises(NotImplementedError):
            GpuTrainPipeline(b)
    with pytest.raises(ValueError):
        GpuTrainPipeline(base[:4] + [dict(type='ColorJitter', hue=0.6)] + base[4:])


@pytest.mark.parametrize('name', ['r18_sgd_cos_100e_r2_1xNx8_k400.py', 'r50_sgd_cos_100e_r5_1xNx2_k400.py'])
def test_reference_color_configs_build(name):
    path = os.path.join(REF_CFG, name)
    if not os.path.exists(path):
        pytest.skip('reference checkout not present')
    import vfs_amd
    cfg = vfs_amd.Config.fromfile(path)
    pipe = GpuTrainPipeline(cfg.train_pipeline)
    assert pipe.photometric and pipe.jitter is not None and pipe.gray is not None and pipe.blur is not None
    assert (pipe.num_clips, pipe.clip_len) == ((2, 4) if name.startswith('r18') else (2, 1))
    assert pipe.jitter['ranges'] == [[0.6, 1.4], [0.6, 1.4], [0.6, 1.4], [-0.1, 0.1]]
    b, f, ph = pipe.sample(pipe.num_clips * pipe.clip_len, (256, 340))
    assert b.shape == (pipe.num_clips * pipe.clip_len, 4) and set(ph) >= {'jitter', 'gray', 'blur'}


# ------------------------------------------------------------------------------------- kernel vs oracle (emu / gpu)

@pytest.mark.parametrize('op', ['brightness', 'contrast', 'saturation', 'hue', 'gray', 'blur'])
def test_kernel_single_op(backend, op):
    rows = {'brightness': _row([1]), 'contrast': _row([2]), 'saturation': _row([3]), 'hue': _row([4]),
            'gray': _row(gray=1), 'blur': _row(sigma=0.17)}[op]
    run_case(backend, 1, 2, 2, 30, 41, 21, 19, 5, rows=np.tile(rows, (4, 1)))


def test_kernel_contrast_positions(backend):
    """all jitter ops + grey + blur, contrast at each of the four positions (one frame each)"""
    orders = [[2, 1, 3, 4], [4, 2, 3, 1], [1, 3, 2, 4], [3, 4, 1, 2]]
    rows = np.stack([_row(o, gray=i % 2, sigma=0.12 + 0.02 * i) for i, o in enumerate(orders)])
    run_case(backend, 2, 2, 1, 26, 33, 18, 23, 7, rows=rows)


def test_kernel_all_orders(backend):
    """the 24 orders of the four jitter ops, one frame each"""
    rows = np.stack([_row(o, b=1.21, c=1.33, s=0.64, hue=25) for o in itertools.permutations([1, 2, 3, 4])])
    run_case(backend, 12, 2, 1, 14, 15, 9, 10, 8, rows=rows)


@pytest.mark.parametrize('Ho,Wo', [(1, 9), (9, 1), (1, 1), (37, 71), (17, 65)])
def test_kernel_blur_edges(backend, Ho, Wo):
    """one-pixel-wide / -high outputs, odd widths (x4 pad column) and several 64x16 tiles: the box passes' edge rule"""
    rows = np.stack([_row([2, 4], gray=1, sigma=0.2), _row(sigma=0.1), _row([3, 2], sigma=0.15), _row([1])])
    run_case(backend, 1, 2, 2, 40, 50, Ho, Wo, 11, rows=rows)


def test_kernel_sampled_decisions(backend):
    run_case(backend, 2, 2, 2, 36, 44, 20, 24, 13)


def test_kernel_flags_off_equals_plain(backend):
    """no photometric step on any frame: bit-identical to vfs_crop_resize_flip_norm"""
    from vfs_amd import _lib
    from vfs_amd.pipeline import GpuTrainPipeline as P
    B, V, T, Hs, Ws, Ho, Wo = 2, 2, 2, 33, 47, 17, 21
    frames = backend.d(torch.from_numpy(_frames(B, V * T, Hs, Ws, 17)))
    plain = P([dict(type='RandomResizedCrop', area_range=(0.2, 1.), same_across_clip=False, same_on_clip=False),
               dict(type='Resize', scale=(Wo, Ho), keep_ratio=False), dict(type='Flip', flip_ratio=0.5),
               dict(type='Normalize', mean=MEAN, std=STD, to_bgr=False)], V, T)
    color = _pipe(V, T, Ho, Wo)
    prev = _lib._LIB
    _lib.set_lib(backend.lib)
    try:
        np.random.seed(3)
        random.seed(3)
        a = plain(frames, want_x4=True)
        b = color(frames, boxes=a['boxes'], flips=a['flips'], photo=np.zeros((B * V * T, 8), np.int32), want_x4=True)
        c = color(frames, boxes=a['boxes'], flips=a['flips'], want_x4=True)      # explicit boxes, no photo: none applied
    finally:
        _lib.set_lib(prev)
    for o in (b, c):
        assert torch.equal(a['imgs'].cpu().view(torch.int32), o['imgs'].cpu().view(torch.int32))
        assert torch.equal(a['x4'].cpu().view(torch.int16), o['x4'].cpu().view(torch.int16))


def test_workspace_refused_when_small(emu_backend):
    lib = emu_backend.lib
    nb = torch.zeros(1, dtype=torch.int64)
    lib.crop_resize_flip_photo_norm_workspace_bytes(4, 8, 8, nb)
    assert int(nb) == 4 * 8 + 4 * 8 * 8 * 4
    src = torch.zeros(4, 8, 8, 3, dtype=torch.uint8)
    boxes = torch.tensor([[0, 0, 8, 8]] * 4, dtype=torch.int32)
    flips, rows = torch.zeros(4, dtype=torch.uint8), torch.zeros(4, 8, dtype=torch.int32)
    ws, imgs = torch.zeros(int(nb) - 1, dtype=torch.uint8), torch.zeros(1, 4, 3, 1, 8, 8)
    from vfs_amd._lib import VfsError
    with pytest.raises(VfsError):
        lib.crop_resize_flip_photo_norm(src, boxes, flips, rows, ws, ws.numel(), imgs, None, 1, 4, 1, 8, 8, 8, 8, 8, *MEAN, *STD, None)


# --------------------------------------------------------------------------------------------------------- GPU only

@pytest.mark.gpu
@pytest.mark.parametrize('V,T', [(2, 1), (2, 4)])
def test_kernel_full_size(gpu_backend, V, T):
    """baseline size: 340x256 frames -> 224x224, 8 pairs, R50 / R18 layouts, sampled decisions, every kind forced somewhere"""
    frames = _frames(8, V * T, 256, 340, 9)
    F = 8 * V * T
    pipe = _pipe(V, T, 224, 224)
    np.random.seed(9)
    random.seed(9)
    draws = [pipe.sample(V * T, (256, 340)) for _ in range(8)]
    boxes, flips = np.concatenate([d[0] for d in draws]), np.concatenate([d[1] for d in draws])
    rows = pack_photometric({k: np.concatenate([d[2][k] for d in draws]) for k in draws[0][2]})
    rows[:4] = [_row([2, 1, 3, 4], sigma=0.2), _row([4, 3, 1, 2], gray=1), _row([1, 4, 2]), _row(gray=1, sigma=0.1)]
    assert rows[:, 0].any() and rows[:, 5].any() and rows[:, 6].any() and (rows[:, 0] == 0).any() and F > 4
    run_case(gpu_backend, 8, V, T, 256, 340, 224, 224, 9, rows=rows, boxes=boxes, flips=flips, frames=frames)


def _color_cube():
    v = np.arange(256, dtype=np.uint8)
    return np.stack(np.meshgrid(v, v, v, indexing='ij'), -1).reshape(1, 1, 4096, 4096, 3)


@pytest.mark.gpu
def test_color_cube(gpu_backend):
    """one 4096x4096 frame holding every RGB value, full box, same-size resize (the identity): hue at several shifts,
    saturation, grey, each bit for bit against the oracle on all 2^24 colours"""
    frames = _color_cube()
    boxes, flips = _full_boxes(1, 4096, 4096), np.zeros(1, np.uint8)
    dev = gpu_backend.dev
    pipe = GpuTrainPipeline([dict(type='Resize', scale=(4096, 4096), keep_ratio=False), dict(type='ColorJitter', hue=0.5),
                             dict(type='RandomGrayScale'), dict(type='Normalize', mean=[0, 0, 0], std=[1, 1, 1])], 1, 1)
    ft = torch.from_numpy(frames).to(dev)
    img = frames[0, 0]
    rows = [_row([4], hue=h) for h in (0, 1, 25, 128, 231, 255)] + [_row([3], s=s) for s in (0.6, 1.4)]
    rows += [_row(gray=1), _row([1], b=1.37)]
    for row in rows:
        out = pipe(ft, boxes=boxes, flips=flips, photo=row[None])
        got = out['imgs'][0, 0, :, 0].permute(1, 2, 0).cpu().numpy()
        want = PH.apply_packed(img, row).astype(np.float32)
        assert np.array_equal(got, want), (row.tolist(), int((got != want).any(-1).sum()))


@pytest.mark.gpu
def test_runs_are_bit_identical(gpu_backend):
    frames = torch.from_numpy(_frames(8, 8, 256, 340, 4)).to(gpu_backend.dev)
    pipe = _pipe(2, 4, 224, 224)
    outs = []
    for _ in range(2):
        np.random.seed(4)
        random.seed(4)
        outs.append(pipe(frames, want_x4=True))
    torch.cuda.synchronize()
    assert np.array_equal(outs[0]['photo_rows'], outs[1]['photo_rows'])
    assert torch.equal(outs[0]['imgs'].view(torch.int32), outs[1]['imgs'].view(torch.int32))
    assert torch.equal(outs[0]['x4'].view(torch.int16), outs[1]['x4'].view(torch.int16))


@pytest.mark.gpu
def test_color_pipeline_feeds_train_step(gpu_backend):
    """the R18 config with the object-level photometric steps -> GpuTrainPipeline -> train_step: imgs equal the oracle's
    bit for bit and the step's loss is finite"""
    import vfs_amd
    cfg = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', 'vfs_r18.py'))
    tp = color_pipeline(cfg.train_pipeline)
    for s in tp:
        if s['type'] == 'Resize':
            s['scale'] = (64, 64)
    pipe = GpuTrainPipeline(tp)
    V, T = pipe.num_clips, pipe.clip_len
    assert (V, T) == (2, 4) and pipe.photometric
    B = 4
    frames = _frames(B, V * T, 72, 96, 21)
    np.random.seed(1)
    random.seed(1)
    out = pipe(torch.from_numpy(frames).to(gpu_backend.dev))
    rows = out['photo_rows']
    assert rows[:, 0].any() and rows[:, 6].any()
    want = oracle_pipeline(frames, out['boxes'], out['flips'], rows, (64, 64), V, T, pipe.mean, pipe.std)
    assert np.array_equal(out['imgs'].cpu().numpy().view(np.uint32), want.view(np.uint32))
    model = vfs_amd.build_model(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(gpu_backend.dev).train()
    res = model.train_step(dict(imgs=out['imgs'], label=torch.zeros(B, 1)), None)
    res['loss'].backward()
    assert np.isfinite(res['log_vars']['loss']) and res['num_samples'] == B
