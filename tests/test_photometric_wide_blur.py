"""RandomGaussianBlur at box radii of 1 and above (GpuTrainPipeline(max_blur_radius=R), vfs_crop_resize_flip_photo_norm_blur
and its _ragged form): the numpy restatement of PIL's extended box blur in clamped-index form vs PIL itself and vs frames PIL
produced (tests/golden/wide_blur.npz), the host's admission rules and decisions, and the kernel vs that restatement bit
for bit (backend = emu on the CPU / gpu)."""
import math
import os
import random

import numpy as np
import pytest
import torch

from oracle import pipeline_oracle as PO
from tests import photometric_oracle as PH
from vfs_amd import _lib
from vfs_amd.pipeline import GpuTrainPipeline, blur_weights, blur_weights_wide, pack_photometric

HERE = os.path.dirname(os.path.abspath(__file__))
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
F32 = lambda v: int(np.float32(v).view(np.int32))      # noqa: E731
GOLD = np.load(os.path.join(HERE, 'golden', 'wide_blur.npz'))
SIGMA_R3 = 3.9      # a sigma whose box radius has the integer part 3 (asserted in test_weights)


# ------------------------------------------------------------------------------------------------------- the oracle

def box_weights(sigma):
    """PIL GaussianBlur(radius=sigma): _gaussian_blur_radius(sigma, 3 passes) in fp32 -> (r, ww, fw) of ImagingLineBoxBlur8"""
    f32 = np.float32
    s2 = f32(f32(f32(sigma) * f32(sigma)) / f32(3))
    L = f32(math.sqrt(12.0 * float(s2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * s2)))
    a = f32(a / f32(f32(6) * f32(s2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    rad = f32(l + a)
    r = int(rad)
    ww = int(f32(f32(1 << 24) / f32(f32(2) * rad + f32(1))))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def box_pass(x, r, ww, fw, axis):
    """out[i] = (ww * sum_{|d| <= r} in[clamp(i+d)] + fw * (in[clamp(i-r-1)] + in[clamp(i+r+1)]) + 2^23) >> 24"""
    x = x.astype(np.int64)
    n = x.shape[axis]
    at = lambda d: np.take(x, np.clip(np.arange(n) + d, 0, n - 1), axis=axis)      # noqa: E731
    acc = ww * sum(at(d) for d in range(-r, r + 1)) + fw * (at(-r - 1) + at(r + 1)) + (1 << 23)
    assert acc.max() < 1 << 32
    return (acc >> 24).astype(np.uint8)


def box_blur(x, r, ww, fw):
    """three horizontal then three vertical passes on uint8 HxWxC, uint8 after every pass"""
    for axis in (1, 1, 1, 0, 0, 0):
        x = box_pass(x, r, ww, fw, axis)
    return x


def clamp_row(row, R):
    """what a launch of bound R makes of a row's blur words: r <= R, ww <= 2^24 / (2r + 1), fw <= (2^24 - (2r + 1) ww) / 2"""
    r = min((int(row[4]) >> 8) & 255, R)
    ww = min(int(row[6]) & 0xFFFFFFFF, (1 << 24) // (2 * r + 1))
    fw = min(int(row[7]) & 0xFFFFFFFF, ((1 << 24) - (2 * r + 1) * ww) // 2)
    return r, ww, fw


def oracle_pipeline(frames, boxes, flips, rows, out_hw, V, T, R):
    """frames: [B][F] arrays or a list of per-sample [F][Hs][Ws][3] arrays -> fp32 [B][V][3][T][H][W]"""
    B, F = len(frames), len(frames[0])
    H, W = out_hw
    out = np.empty((B, V, 3, T, H, W), np.float32)
    for b in range(B):
        for f in range(F):
            left, top, right, bottom = boxes[b * F + f]
            img = PO.resize_bilinear_u8(frames[b][f][top:bottom, left:right], W, H)
            if flips[b * F + f]:
                img = np.ascontiguousarray(img[:, ::-1])
            row = np.array(rows[b * F + f])
            r, ww, fw = clamp_row(row, R)
            row[6] = row[7] = 0
            img = PH.apply_packed(img, row)
            if ww:
                img = box_blur(img, r, ww, fw)
            out[b, f // T, :, f % T] = PO.normalize(img, MEAN, STD).transpose(2, 0, 1)
    return out


# ------------------------------------------------------------------------------------------------------- helpers

def _frames(B, F, Hs, Ws, seed):
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, (B, F, Hs // 4 + 1, Ws // 4 + 1, 3), dtype=np.uint8)
    up = np.repeat(np.repeat(base, 4, axis=2), 4, axis=3)[:, :, :Hs, :Ws]
    return np.clip(up.astype(np.int64) + g.integers(-20, 21, up.shape), 0, 255).astype(np.uint8)


def _steps(sigma_range=(0.1, 2.0)):
    return [dict(type='ColorJitter', brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p=0.8, same_across_clip=False,
                 same_on_clip=False),
            dict(type='RandomGrayScale', p=0.2, same_across_clip=False, same_on_clip=False),
            dict(type='RandomGaussianBlur', p=0.5, sigma_range=sigma_range, same_across_clip=False, same_on_clip=False)]


def _pipe(V, T, Ho, Wo, R, steps=None):
    steps = _steps((0.1, 0.2) if R == 0 else (0.1, 2.0) if R == 1 else (0.1, 3.0) if R == 2 else (0.1, SIGMA_R3)) if steps is None else steps
    return GpuTrainPipeline([dict(type='RandomResizedCrop', area_range=(0.2, 1.), same_across_clip=False, same_on_clip=False),
                             dict(type='Resize', scale=(Wo, Ho), keep_ratio=False),
                             dict(type='Flip', flip_ratio=0.5, same_across_clip=False, same_on_clip=False)] + steps +
                            [dict(type='Normalize', mean=MEAN, std=STD, to_bgr=False),
                             dict(type='FormatShape', input_format='NCTHW')], V, T, max_blur_radius=R)


def _row(order=(), b=1.3, c=0.7, s=1.45, hue=231, gray=0, sigma=None):
    r = np.zeros(8, np.int32)
    r[0] = sum(op << (4 * k) for k, op in enumerate(order))
    r[1], r[2], r[3], r[4], r[5] = F32(b), F32(c), F32(s), hue, gray
    if sigma is not None:
        rad, r[6], r[7] = box_weights(sigma)
        r[4] |= rad << 8
    return r


def _radius(row):
    return (int(row[4]) >> 8) & 255


class _Lib:
    """the backend's library in place of the product's for one with-block"""

    def __init__(self, be):
        self.be = be

    def __enter__(self):
        self.prev = _lib._LIB
        _lib.set_lib(self.be.lib)

    def __exit__(self, *exc):
        if self.be.dev.type == 'cuda':
            torch.cuda.synchronize()
        _lib.set_lib(self.prev)


def run_pipe(be, pipe, frames, **kw):
    """frames: numpy [B][F][Hs][Ws][3] or a list of per-sample arrays"""
    src = [be.d(torch.from_numpy(f)) for f in frames] if isinstance(frames, list) else be.d(torch.from_numpy(frames))
    with _Lib(be):
        out = pipe(src, want_x4=True, **kw)
    return out


def check(be, out, want):
    """fp32 imgs as uint32 and the bf16 x4 bit for bit"""
    got = out['imgs'].cpu().numpy()
    assert got.shape == want.shape
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:4].tolist())
    B, V, _, T, Ho, Wo = want.shape
    Wp = Wo + (Wo & 1)
    x4 = torch.full((V * B * T, Ho, Wp, 4), 7.0, dtype=torch.bfloat16)
    be.hostlib.imgs_to_nhwc4(torch.from_numpy(want), x4, B, V, T, Ho, Wo, Wp, None)
    assert torch.equal(out['x4'].cpu().view(torch.int16), x4.view(torch.int16))


def run_case(be, R, B, V, T, Hs, Ws, Ho, Wo, seed, rows=None):
    """GpuTrainPipeline(max_blur_radius=R) on `be` vs the oracle; rows=None: every decision sampled, else the rows with
    boxes and flips of the test's own (the pipeline samples all three when it gets no boxes)"""
    frames = _frames(B, V * T, Hs, Ws, seed)
    np.random.seed(seed)
    random.seed(seed)
    kw = {}
    if rows is not None:
        assert len(rows) == B * V * T
        boxes, flips = _decisions(B * V * T, Hs, Ws, seed)
        kw = dict(boxes=boxes, flips=flips, photo=rows)
    out = run_pipe(be, _pipe(V, T, Ho, Wo, R), frames, **kw)
    if rows is not None:
        assert np.array_equal(out['photo_rows'], rows)
    check(be, out, oracle_pipeline(frames, out['boxes'], out['flips'], out['photo_rows'], (Ho, Wo), V, T, R))
    return out


def call_entry(be, name, frames, boxes, flips, rows, Ho, Wo, V, T, R=None):
    """a uniform photometric C entry called directly (R=None: the entry without max_blur_radius) -> imgs, x4 as numpy bits"""
    B, F, Hs, Ws, _ = frames.shape
    Wp = Wo + (Wo & 1)
    nb = torch.zeros(1, dtype=torch.int64)
    be.lib.crop_resize_flip_photo_norm_workspace_bytes(B * F, Ho, Wo, nb)
    ws = torch.zeros(int(nb), dtype=torch.uint8)
    imgs = torch.zeros(B, V, 3, T, Ho, Wo)
    x4 = torch.zeros(V * B * T, Ho, Wp, 4, dtype=torch.bfloat16)
    extra = () if R is None else (R,)
    getattr(be.hostlib, name)(torch.from_numpy(frames), torch.from_numpy(np.ascontiguousarray(boxes, np.int32)),
                              torch.from_numpy(np.ascontiguousarray(flips, np.uint8)),
                              torch.from_numpy(np.ascontiguousarray(rows, np.int32)), ws, ws.numel(), imgs, x4, B, V, T, Hs, Ws,
                              Ho, Wo, Wp, *MEAN, *STD, *extra, None)
    return imgs.numpy().view(np.uint32), x4.view(torch.int16).numpy()


def _decisions(n, Hs, Ws, seed):
    g = np.random.default_rng(seed)
    boxes = []
    for _ in range(n):
        w, h = int(g.integers(Ws // 2, Ws + 1)), int(g.integers(Hs // 2, Hs + 1))
        x, y = int(g.integers(0, Ws - w + 1)), int(g.integers(0, Hs - h + 1))
        boxes.append((x, y, x + w, y + h))
    return np.asarray(boxes, np.int32), g.integers(0, 2, n).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- oracle vs PIL (CPU)

PIL_SIGMAS = (0.1, 0.2, 0.9, 1.0, 1.5, 2.0, 3.0, 5.0)
PIL_SIZES = ((224, 224), (17, 70), (5, 3), (2, 9), (1, 1))


def test_restatement_matches_pil():
    """the clamped-index form equals PIL.ImageFilter.GaussianBlur on every pixel: r = 0, 1, 2, 4, sizes below the window too"""
    pytest.importorskip('PIL')
    from PIL import Image, ImageFilter
    g = np.random.default_rng(5)
    assert sorted({box_weights(s)[0] for s in PIL_SIGMAS}) == [0, 1, 2, 4]
    for sigma in PIL_SIGMAS:
        for h, w in PIL_SIZES:
            x = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
            want = np.asarray(Image.fromarray(x).filter(ImageFilter.GaussianBlur(radius=sigma)), np.uint8)
            assert np.array_equal(box_blur(x, *box_weights(sigma)), want), (sigma, h, w)


def test_restatement_matches_golden():
    """the same against frames PIL produced when the fixture was made: fixed sigmas (r = 0..4) and the frames the
    reference's RandomGaussianBlur returned for sigma_range (0.1, 2.0)"""
    n = len({k.split('/')[1] for k in GOLD.files if k.startswith('pil/')})
    radii = set()
    for k in range(n):
        x, sigma = GOLD[f'pil/{k}/in'], float(GOLD[f'pil/{k}/sigma'])
        radii.add(box_weights(sigma)[0])
        assert np.array_equal(box_blur(x, *box_weights(sigma)), GOLD[f'pil/{k}/out']), (k, sigma, x.shape)
    assert radii == {0, 1, 2, 3, 4}
    for case in sorted({k.split('/')[1] for k in GOLD.files if k.startswith('draw/')}):
        src, out, blur, sigma = (GOLD[f'draw/{case}/{k}'] for k in ('src', 'out', 'blur', 'sigma'))
        assert {box_weights(s)[0] for s, b in zip(sigma, blur) if b} == {0, 1}
        for i in range(len(src)):
            want = box_blur(src[i], *box_weights(sigma[i])) if blur[i] else src[i]
            assert np.array_equal(want, out[i]), (case, i)


def test_weights():
    """blur_weights_wide = the oracle's (r, ww, fw); at r = 0 today's blur_weights; the sigmas the kernel tests use"""
    for sigma in PIL_SIGMAS + (SIGMA_R3, 0.17, 1.2345):
        r, ww, fw = box_weights(sigma)
        assert blur_weights_wide(sigma) == (r, ww, fw)
        assert (2 * r + 1) * ww + 2 * fw <= 1 << 24 and ww > 0 and fw >= 0
        if r == 0:
            assert blur_weights(sigma) == (ww, fw) == PH.blur_weights(sigma)
        else:
            with pytest.raises(NotImplementedError, match=f'max_blur_radius={r}' if r <= 3 else 'box radius'):
                blur_weights(sigma)
    assert [box_weights(s)[0] for s in (1.5, 2.0, 3.0, SIGMA_R3)] == [1, 1, 2, 3]


# ------------------------------------------------------------------------------------------------------ host (CPU)

def _cfg(sigma_range):
    return [dict(type='Resize', scale=(8, 8), keep_ratio=False), dict(type='RandomGaussianBlur', sigma_range=sigma_range),
            dict(type='Normalize', mean=MEAN, std=STD)]


def test_admission():
    with pytest.raises(NotImplementedError, match='max_blur_radius=1'):
        GpuTrainPipeline(_cfg((0.1, 2.0)), 2, 1)                                  # the default still refuses
    assert GpuTrainPipeline(_cfg((0.1, 0.2)), 2, 1).max_blur_radius == 0
    p = GpuTrainPipeline(_cfg((0.1, 2.0)), 2, 1, max_blur_radius=1)
    assert p.max_blur_radius == 1 and p.blur['sigma_range'] == (0.1, 2.0)
    with pytest.raises(NotImplementedError, match='max_blur_radius=1'):
        GpuTrainPipeline(_cfg((0.1, 3.0)), 2, 1, max_blur_radius=1)
    assert GpuTrainPipeline(_cfg((0.1, 3.0)), 2, 1, max_blur_radius=2).max_blur_radius == 2
    assert GpuTrainPipeline(_cfg((0.1, SIGMA_R3)), 2, 1, max_blur_radius=3).max_blur_radius == 3
    with pytest.raises(NotImplementedError):
        GpuTrainPipeline(_cfg((0.1, 5.0)), 2, 1, max_blur_radius=3)
    for bad in (4, -1, 1.5, None):
        with pytest.raises(ValueError, match='max_blur_radius'):
            GpuTrainPipeline(_cfg((0.1, 0.2)), 2, 1, max_blur_radius=bad)


def test_pack_photometric_radius():
    photo = dict(jitter=np.array([1, 0, 0], np.uint8), factors=np.array([[1.2, np.nan, np.nan, 0.1]] * 3), order=np.array([[4, 1, 0, 0]] * 3, np.int8),
                 gray=np.zeros(3, np.uint8), blur=np.array([1, 1, 0], np.uint8), sigma=np.array([2.0, 0.15, 3.0]))
    with pytest.raises(NotImplementedError):
        pack_photometric(photo)                                                    # today's behaviour by default
    rows = pack_photometric(photo, max_blur_radius=1)
    assert rows[0, 4] == (1 << 8 | 25) and rows[1, 4] == 0 and rows[2, 4] == 0 and not rows[2, 6]
    assert tuple(rows[0, 6:]) == box_weights(2.0)[1:] and tuple(rows[1, 6:]) == PH.blur_weights(0.15)
    photo['blur'][2] = 1
    with pytest.raises(NotImplementedError, match='frame 2'):
        pack_photometric(photo, max_blur_radius=1)
    assert _radius(pack_photometric(photo, max_blur_radius=2)[2]) == 2
    photo['sigma'][:] = 0.15                                                       # radii below 1: the same rows with and without the bound
    assert np.array_equal(pack_photometric(photo), pack_photometric(photo, max_blur_radius=3))
    assert np.array_equal(pack_photometric(photo), PH.pack_photometric(photo))


def test_caller_row_above_bound(emu_backend):
    be = emu_backend
    frames = _frames(1, 2, 12, 14, 3)
    boxes, flips = _decisions(2, 12, 14, 3)
    rows = np.stack([_row(sigma=2.0), _row(sigma=3.0)])
    with pytest.raises(ValueError, match='frame 1'):
        run_pipe(be, _pipe(2, 1, 6, 7, 1), frames, boxes=boxes, flips=flips, photo=rows)
    out = run_pipe(be, _pipe(2, 1, 6, 7, 2), frames, boxes=boxes, flips=flips, photo=rows)
    check(be, out, oracle_pipeline(frames, boxes, flips, rows, (6, 7), 2, 1, 2))


def test_c_entry_refuses_radius_bound(emu_backend):
    be = emu_backend
    frames = _frames(1, 2, 12, 14, 3)
    boxes, flips = _decisions(2, 12, 14, 3)
    rows = np.stack([_row(sigma=2.0), _row()])
    for R in (4, -1):
        with pytest.raises(_lib.VfsError, match='crop_resize_flip_photo_norm_blur: max_blur_radius outside 0..3'):
            call_entry(be, 'crop_resize_flip_photo_norm_blur', frames, boxes, flips, rows, 6, 7, 2, 1, R=R)
    src = torch.from_numpy(frames.reshape(-1))
    desc = torch.tensor([[0, 0, 12, 14]], dtype=torch.int32)
    ws, imgs = torch.zeros(1 << 12, dtype=torch.uint8), torch.zeros(1, 2, 3, 1, 6, 7)
    with pytest.raises(_lib.VfsError, match='crop_resize_flip_photo_norm_blur_ragged: max_blur_radius outside 0..3'):
        be.lib.crop_resize_flip_photo_norm_blur_ragged(src, src.numel(), desc, torch.from_numpy(boxes), torch.from_numpy(flips),
                                                       torch.from_numpy(rows), ws, ws.numel(), imgs, None, 1, 2, 1, 6, 7, 8, *MEAN, *STD, 4, None)


DRAWS = sorted({k.split('/')[1] for k in GOLD.files if k.startswith('draw/')})


@pytest.mark.parametrize('case', DRAWS)
def test_decisions_match_reference(case):
    """sample() with sigma_range (0.1, 2.0) draws what the reference's RandomGaussianBlur.__call__ drew: the apply flag from
    np.random and the sigma from random, once before the frame loop and again for every frame that does not share"""
    h, w, nclips, clip_len, nsamp, seed = (int(v) for v in GOLD[f'draw/{case}/meta'])
    soc, sac = (bool(v) for v in GOLD[f'draw/{case}/same'])
    nf = nclips * clip_len
    pipe = GpuTrainPipeline([dict(type='Resize', scale=(8, 8), keep_ratio=False),
                             dict(type='RandomGaussianBlur', p=float(GOLD[f'draw/{case}/p']), sigma_range=(0.1, 2.0), same_on_clip=soc,
                                  same_across_clip=sac), dict(type='Normalize', mean=MEAN, std=STD)], nclips, clip_len, max_blur_radius=1)
    np.random.seed(seed)
    random.seed(seed)
    got = [pipe.sample(nf, (h, w))[2] for _ in range(nsamp)]
    blur, sigma = np.concatenate([g['blur'] for g in got]), np.concatenate([g['sigma'] for g in got])
    on = GOLD[f'draw/{case}/blur'].astype(bool)
    assert np.array_equal(blur, GOLD[f'draw/{case}/blur'])
    assert np.array_equal(sigma[on], GOLD[f'draw/{case}/sigma'][on])
    rows = pack_photometric({k: np.concatenate([g[k] for g in got]) for k in got[0]}, max_blur_radius=1)
    assert {_radius(r) for r in rows[on]} == {0, 1}
    for i in range(len(rows)):      # and the packed rows drive the oracle to the frames the reference returned
        r, ww, fw = clamp_row(rows[i], 1)
        want = box_blur(GOLD[f'draw/{case}/src'][i], r, ww, fw) if ww else GOLD[f'draw/{case}/src'][i]
        assert np.array_equal(want, GOLD[f'draw/{case}/out'][i]), i


# ------------------------------------------------------------------------------------- kernel vs oracle (emu / gpu)

def test_kernel_radii(backend):
    """r = 1 (two sigmas), 2, 3 at max_blur_radius=3, 23x70: two column tiles, two row tiles"""
    rows = np.stack([_row(sigma=1.5), _row(sigma=2.0), _row(sigma=3.0), _row(sigma=SIGMA_R3)])
    assert [_radius(r) for r in rows] == [1, 1, 2, 3]
    run_case(backend, 3, 1, 2, 2, 40, 90, 23, 70, 5, rows=rows)


def test_kernel_mixed_radii(backend):
    """r = 0, 1, 3 and an unblurred frame in one launch; rows with r <= 1 give the same bits at R = 1 and R = 3"""
    rows = np.stack([_row(sigma=0.17), _row([1], sigma=2.0), _row(sigma=SIGMA_R3), _row([4, 3])])
    assert [_radius(r) for r in rows] == [0, 1, 3, 0] and rows[3, 6] == 0
    run_case(backend, 3, 1, 2, 2, 30, 41, 21, 67, 6, rows=rows)
    rows[2] = _row(gray=1, sigma=1.5)
    a = run_case(backend, 1, 1, 2, 2, 30, 41, 21, 67, 6, rows=rows)
    b = run_case(backend, 3, 1, 2, 2, 30, 41, 21, 67, 6, rows=rows)
    assert torch.equal(a['imgs'].cpu().view(torch.int32), b['imgs'].cpu().view(torch.int32))
    assert torch.equal(a['x4'].cpu().view(torch.int16), b['x4'].cpu().view(torch.int16))


@pytest.mark.parametrize('Ho,Wo', [(1, 1), (1, 9), (9, 1), (2, 5), (17, 65), (37, 71), (29, 77)])
def test_kernel_edges(backend, Ho, Wo):
    """outputs smaller than the window, one pixel wide / high, odd widths (x4 pad column), sizes that straddle the 64x16
    tile in both axes, and 29x77 = one tile plus the full halo of R = 3 (12) plus 1: a pass reads across a tile corner"""
    rows = np.stack([_row([2, 4], gray=1, sigma=SIGMA_R3), _row(sigma=1.5), _row([3, 2], sigma=3.0), _row([1], sigma=0.2)])
    assert [_radius(r) for r in rows] == [3, 1, 2, 0]
    run_case(backend, 3, 1, 2, 2, 40, 50, Ho, Wo, 11, rows=rows)


def test_kernel_with_other_steps(backend):
    """saturation, then contrast (its mean is the frame's after saturation), hue, brightness, grey, r = 2 blur: the blur reads
    photo_post's output in the halo too"""
    rows = np.stack([_row([3, 2, 4, 1], gray=1, sigma=3.0), _row([1, 2], sigma=3.0)])
    assert [_radius(r) for r in rows] == [2, 2]
    run_case(backend, 2, 1, 2, 1, 36, 80, 19, 70, 12, rows=rows)


def test_kernel_sampled_decisions(backend):
    out = run_case(backend, 1, 2, 2, 2, 36, 44, 20, 24, 24)
    assert {_radius(r) for r in out['photo_rows'] if r[6]} == {0, 1}


def test_ragged_equals_uniform(backend):
    """two samples of different source sizes, r = 1 and r = 2, through the ragged entry = each through the uniform one"""
    V, T, Ho, Wo, R = 2, 1, 18, 66, 2
    samples = [_frames(1, 2, 30, 41, 1)[0], _frames(1, 2, 25, 52, 2)[0]]
    dec = [_decisions(2, 30, 41, 1), _decisions(2, 25, 52, 2)]
    boxes, flips = np.concatenate([d[0] for d in dec]), np.concatenate([d[1] for d in dec])
    rows = np.stack([_row([2], sigma=2.0), _row(sigma=1.5), _row([1, 2], sigma=3.0), _row(gray=1, sigma=3.0)])
    assert [_radius(r) for r in rows] == [1, 1, 2, 2]
    pipe = _pipe(V, T, Ho, Wo, R)
    rag = run_pipe(backend, pipe, samples, boxes=boxes, flips=flips, photo=rows)
    check(backend, rag, oracle_pipeline(samples, boxes, flips, rows, (Ho, Wo), V, T, R))
    for b in range(2):
        uni = run_pipe(backend, pipe, samples[b][None], boxes=boxes[2 * b:2 * b + 2], flips=flips[2 * b:2 * b + 2], photo=rows[2 * b:2 * b + 2])
        assert torch.equal(uni['imgs'][0].cpu().view(torch.int32), rag['imgs'][b].cpu().view(torch.int32))
        assert torch.equal(uni['x4'].cpu().view(torch.int16), rag['x4'].cpu().view(torch.int16)[b::2])


def test_entries_used(emu_backend):
    """a pipeline with a bound calls the _blur entries with it, whatever the rows carry; without one, the entries of before"""
    calls = []

    class Rec:
        def __getattr__(self, name):
            fn = getattr(emu_backend.lib, name)

            def call(*a):
                calls.append((name, a))
                return fn(*a)
            return call
    frames = _frames(2, 2, 12, 14, 3)
    boxes, flips = _decisions(4, 12, 14, 3)
    prev = _lib._LIB
    _lib.set_lib(Rec())
    try:
        for R, rows in ((2, np.zeros((4, 8), np.int32)), (0, np.zeros((4, 8), np.int32))):
            pipe = _pipe(2, 1, 6, 7, R)
            pipe(torch.from_numpy(frames), boxes=boxes, flips=flips, photo=rows)
            pipe(list(torch.from_numpy(frames)), boxes=boxes, flips=flips, photo=rows)
    finally:
        _lib.set_lib(prev)
    names = [(n, a) for n, a in calls if 'workspace' not in n]
    assert [n for n, _ in names] == ['crop_resize_flip_photo_norm_blur', 'crop_resize_flip_photo_norm_blur_ragged',
                                     'crop_resize_flip_photo_norm', 'crop_resize_flip_photo_norm_ragged']
    assert names[0][1][-2] == 2 and names[1][1][-2] == 2


def test_row_guard(emu_backend):
    """malformed rows at R = 3: radius bits 200, and ww = fw = 2^24 at r = 3.  The launch finishes and computes what the
    clamped row says: r <= R, ww <= 2^24 / (2r + 1), fw <= (2^24 - (2r + 1) ww) / 2 (clamp_row)"""
    be = emu_backend
    V, T, Ho, Wo = 2, 1, 19, 70
    frames = _frames(1, 2, 30, 80, 14)
    boxes, flips = _decisions(2, 30, 80, 14)
    rows = np.stack([_row([1], sigma=SIGMA_R3), _row(sigma=SIGMA_R3)])
    rows[0, 4] = (200 << 8) | 17
    rows[1, 6] = rows[1, 7] = 1 << 24
    assert clamp_row(rows[0], 3) == box_weights(SIGMA_R3) and clamp_row(rows[1], 3) == (3, (1 << 24) // 7, 0)
    imgs, _ = call_entry(be, 'crop_resize_flip_photo_norm_blur', frames, boxes, flips, rows, Ho, Wo, V, T, R=3)
    want = oracle_pipeline(frames, boxes, flips, rows, (Ho, Wo), V, T, 3)
    assert np.array_equal(imgs, want.view(np.uint32))


def test_old_rows(backend):
    """rows without a radius through the new entry at R = 0 and R = 2 = the existing entry point's output, bit for bit; so
    is a row whose radius bits the existing entry ignores, at R = 0"""
    V, T, Ho, Wo = 2, 2, 21, 67
    frames = _frames(1, 4, 30, 41, 15)
    boxes, flips = _decisions(4, 30, 41, 15)
    rows = np.stack([_row([2, 4], gray=1, sigma=0.2), _row(sigma=0.1), _row([3, 2], sigma=0.15), _row([1])])
    assert all(_radius(r) == 0 for r in rows)
    old = call_entry(backend, 'crop_resize_flip_photo_norm', frames, boxes, flips, rows, Ho, Wo, V, T)
    assert np.array_equal(old[0], oracle_pipeline(frames, boxes, flips, rows, (Ho, Wo), V, T, 0).view(np.uint32))
    for R in (0, 2):
        new = call_entry(backend, 'crop_resize_flip_photo_norm_blur', frames, boxes, flips, rows, Ho, Wo, V, T, R=R)
        assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1]), R
    rows[1, 4] |= 2 << 8
    new = call_entry(backend, 'crop_resize_flip_photo_norm_blur', frames, boxes, flips, rows, Ho, Wo, V, T, R=0)
    again = call_entry(backend, 'crop_resize_flip_photo_norm', frames, boxes, flips, rows, Ho, Wo, V, T)
    assert np.array_equal(old[0], new[0]) and np.array_equal(old[0], again[0])


# --------------------------------------------------------------------------------------------------------- GPU only

@pytest.mark.gpu
def test_full_size(gpu_backend):
    """224x224 from 340x256 frames, V = 2, T = 4, decisions sampled with sigma_range (0.1, 2.0) at max_blur_radius=1: equal to
    the oracle and bit-identical on two runs"""
    be = gpu_backend
    B, V, T = 2, 2, 4
    frames = _frames(B, V * T, 256, 340, 9)
    pipe = _pipe(V, T, 224, 224, 1)
    outs = []
    for _ in range(2):
        np.random.seed(3)
        random.seed(3)
        outs.append(run_pipe(be, pipe, frames))
    rows = outs[0]['photo_rows']
    assert {_radius(r) for r in rows if r[6]} == {0, 1} and (rows[:, 6] == 0).any()
    assert np.array_equal(rows, outs[1]['photo_rows'])
    assert torch.equal(outs[0]['imgs'].view(torch.int32), outs[1]['imgs'].view(torch.int32))
    assert torch.equal(outs[0]['x4'].view(torch.int16), outs[1]['x4'].view(torch.int16))
    check(be, outs[0], oracle_pipeline(frames, outs[0]['boxes'], outs[0]['flips'], rows, (224, 224), V, T, 1))
