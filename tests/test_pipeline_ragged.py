"""Input pipeline on batches of mixed frame sizes (vfs_crop_resize_flip_norm_ragged / _photo_norm_ragged, pack_frames,
GpuTrainPipeline on a list of per-sample frames): the ragged launch equals, bit for bit, the uniform entry points run
sample by sample and the per-sample oracle; host packing, validation and RNG order; the descriptor guard (CPU
emulator only: nothing hands a bad table to a kernel on the GPU)."""
import os
import random

import numpy as np
import pytest
import torch

from oracle import pipeline_oracle as PO
from tests import photometric_oracle as PH
from vfs_amd import _lib
from vfs_amd.pipeline import GpuTrainPipeline, PackedFrames, pack_frames

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
SHAPE, ARG = -1, -3                                   # VFS_ERR_SHAPE, VFS_ERR_ARG
SIZES = [(5, 7), (33, 16), (1, 3), (12, 12)]          # (Hs, Ws) per sample
HO, WO = 9, 11                                        # odd width: x4 has a pad column
WP = WO + 1
F32 = lambda v: int(np.float32(v).view(np.int32))      # noqa: E731

COLOR_STEPS = [dict(type='ColorJitter', brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p=0.8, same_across_clip=False,
                    same_on_clip=False),
               dict(type='RandomGrayScale', p=0.2, same_across_clip=False, same_on_clip=False),
               dict(type='RandomGaussianBlur', p=0.5, same_across_clip=False, same_on_clip=False)]


def _pipe(V, T, Ho, Wo, color=False):
    return GpuTrainPipeline([dict(type='RandomResizedCrop', area_range=(0.2, 1.), same_across_clip=False, same_on_clip=False),
                             dict(type='Resize', scale=(Wo, Ho), keep_ratio=False),
                             dict(type='Flip', flip_ratio=0.5, same_across_clip=False, same_on_clip=False)] +
                            (COLOR_STEPS if color else []) +
                            [dict(type='Normalize', mean=MEAN, std=STD, to_bgr=False),
                             dict(type='FormatShape', input_format='NCTHW')], V, T)


def _sample(F, Hs, Ws, seed):
    """one decoded sample uint8 [F][Hs][Ws][3]: blocky content plus noise, so that crops and flips show"""
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, (F, Hs // 4 + 1, Ws // 4 + 1, 3), dtype=np.uint8)
    up = np.repeat(np.repeat(base, 4, axis=1), 4, axis=2)[:, :Hs, :Ws]
    return np.clip(up.astype(np.int64) + g.integers(-20, 21, up.shape), 0, 255).astype(np.uint8)


def _boxes(F, Hs, Ws):
    """full frame, one pixel wide, the bottom-right corner, one pixel high"""
    rows = [[0, 0, Ws, Hs], [Ws // 2, 0, Ws // 2 + 1, Hs], [max(Ws - 3, 0), max(Hs - 2, 0), Ws, Hs], [0, Hs // 2, Ws, Hs // 2 + 1]]
    return np.asarray(rows[:F], np.int32)


def _row(order=(), b=1.3, c=0.7, s=1.45, hue=231, gray=0, sigma=None):
    r = np.zeros(8, np.int32)
    r[0] = sum(op << (4 * k) for k, op in enumerate(order))
    r[1], r[2], r[3], r[4], r[5] = F32(b), F32(c), F32(s), hue, gray
    if sigma is not None:
        r[6], r[7] = PH.blur_weights(sigma)
    return r


def _photo_rows(n):
    """every jitter op, contrast first / in the middle / last (the per-frame luma sum), grey, blur, all-zero rows"""
    kinds = [_row([2, 1, 3, 4]), _row([1, 2, 4]), _row([4, 3, 1, 2]), _row([1]), np.zeros(8, np.int32), _row([3]), _row([4]),
             _row(gray=1), _row(sigma=0.15), _row([2], gray=1, sigma=0.15), np.zeros(8, np.int32), _row([3, 2, 1], sigma=0.15)]
    return np.stack([kinds[i % len(kinds)] for i in range(n)])


class Recorder:
    """stands in for the library: records the C entries a call goes through, forwards them to `lib` (None: no kernel runs)"""

    def __init__(self, lib=None):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name) if self.lib is not None else (lambda *a: 0)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


def _run(lib, pipe, frames, **kw):
    prev = _lib._LIB
    _lib.set_lib(lib)
    try:
        out = pipe(frames, **kw)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
    finally:
        _lib.set_lib(prev)
    return out


def _bits(out):
    return out['imgs'].cpu().numpy().view(np.uint32), out['x4'].cpu().view(torch.int16).numpy()


def _oracle_sample(frames, boxes, flips, rows, V, T, Ho, Wo, mean=MEAN, std=STD):
    """the reference's chain on ONE sample uint8 [F][Hs][Ws][3] -> fp32 [V][3][T][Ho][Wo]; rows=None: no photometric step"""
    if rows is None:
        return PO.train_pipeline(frames[None], boxes, flips, (Ho, Wo), mean, std, V, T)[0]
    out = np.empty((V, 3, T, Ho, Wo), np.float32)
    for f in range(V * T):
        left, top, right, bottom = boxes[f]
        img = PO.resize_bilinear_u8(frames[f, top:bottom, left:right], Wo, Ho)
        if flips[f]:
            img = np.ascontiguousarray(img[:, ::-1])
        out[f // T, :, f % T] = PO.normalize(PH.apply_packed(img, rows[f]), mean, std).transpose(2, 0, 1)
    return out


_CASES = {}


def _case(be, V, T, color):
    """the four samples of SIZES with explicit boxes, mixed flips (and hand-made photometric rows), through the UNIFORM entry
    points one sample at a time: the expected bits of the ragged launch.  Computed once per backend and shared."""
    key = (be.name, V, T, color)
    if key not in _CASES:
        F = V * T
        samples = [_sample(F, Hs, Ws, 100 + i) for i, (Hs, Ws) in enumerate(SIZES)]
        boxes = np.concatenate([_boxes(F, Hs, Ws) for Hs, Ws in SIZES])
        flips = (np.arange(len(SIZES) * F) % 3 != 1).astype(np.uint8)
        rows = _photo_rows(len(SIZES) * F) if color else None
        pipe = _pipe(V, T, HO, WO, color)
        per = []
        for b, s in enumerate(samples):
            sl = slice(b * F, (b + 1) * F)
            out = _run(be.lib, pipe, be.d(torch.from_numpy(s[None])), boxes=boxes[sl], flips=flips[sl],
                       photo=None if rows is None else rows[sl], want_x4=True)
            per.append(_bits(out))
        _CASES[key] = dict(samples=samples, boxes=boxes, flips=flips, rows=rows, per=per, pipe=pipe)
    return _CASES[key]


def _assert_sample(got_imgs, got_x4, b, B, V, T, want):
    """sample b of a batch of B: imgs[b] and the x4 frames (v, b, t) against the B = 1 result `want`"""
    wi, wx = want
    assert np.array_equal(got_imgs[b], wi[0]), f'imgs of sample {b}'
    gx = got_x4.reshape(V, B, T, HO, WP, 4)[:, b]
    assert np.array_equal(gx, wx.reshape(V, 1, T, HO, WP, 4)[:, 0]), f'x4 of sample {b}'


# ------------------------------------------------------------------------------ 1, 2: ragged == per-sample uniform

@pytest.mark.parametrize('V,T', [(1, 3), (2, 2)])
def test_ragged_equals_per_sample_plain(backend, V, T):
    """(V, T) = (1, 3): the samples after the first start at odd byte offsets"""
    c = _case(backend, V, T, False)
    B = len(SIZES)
    rec = Recorder(backend.lib)
    out = _run(rec, c['pipe'], [backend.d(torch.from_numpy(s)) for s in c['samples']], boxes=c['boxes'], flips=c['flips'], want_x4=True)
    assert [n for n, _ in rec.calls] == ['crop_resize_flip_norm_ragged']
    assert out['shapes'] == SIZES
    if (V, T) == (1, 3):
        assert any(o % 2 for o in np.cumsum([V * T * h * w * 3 for h, w in SIZES])[:-1])
    imgs, x4 = _bits(out)
    for b in range(B):
        _assert_sample(imgs, x4, b, B, V, T, c['per'][b])
    if (V, T) == (2, 2):       # and the oracle itself, sample by sample
        F = V * T
        for b in range(B):
            want = _oracle_sample(c['samples'][b], c['boxes'][b * F:(b + 1) * F], c['flips'][b * F:(b + 1) * F], None, V, T, HO, WO)
            assert np.array_equal(imgs[b], want.view(np.uint32)), b


@pytest.mark.parametrize('V,T', [(1, 3), (2, 2)])
def test_ragged_equals_per_sample_photometric(backend, V, T):
    c = _case(backend, V, T, True)
    B, F = len(SIZES), V * T
    rows = c['rows']
    orders = [[(int(r[0]) >> (4 * k)) & 15 for k in range(4)] for r in rows]
    assert {op for o in orders for op in o} == {0, 1, 2, 3, 4} and {o.index(2) for o in orders if 2 in o} >= {0, 1, 3}
    assert rows[:, 5].any() and rows[:, 6].any() and not rows[4].any()
    frames = [backend.d(torch.from_numpy(s)) for s in c['samples']]
    rec = Recorder(backend.lib)
    out = _run(rec, c['pipe'], frames, boxes=c['boxes'], flips=c['flips'], photo=rows, want_x4=True)
    assert [n for n, _ in rec.calls if 'workspace' not in n] == ['crop_resize_flip_photo_norm_ragged']
    imgs, x4 = _bits(out)
    for b in range(B):
        _assert_sample(imgs, x4, b, B, V, T, c['per'][b])
    if (V, T) == (2, 2):
        for b in range(B):
            sl = slice(b * F, (b + 1) * F)
            want = _oracle_sample(c['samples'][b], c['boxes'][sl], c['flips'][sl], rows[sl], V, T, HO, WO)
            assert np.array_equal(imgs[b], want.view(np.uint32)), b
    # rows all zero: the plain ragged entry's bits
    zero = _run(backend.lib, c['pipe'], frames, boxes=c['boxes'], flips=c['flips'], photo=np.zeros_like(rows), want_x4=True)
    plain = _run(backend.lib, _case(backend, V, T, False)['pipe'], frames, boxes=c['boxes'], flips=c['flips'], want_x4=True)
    for a, b in zip(_bits(zero), _bits(plain)):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------------------- 3: uniform sizes as a list

@pytest.mark.parametrize('color', [False, True], ids=['plain', 'color'])
def test_uniform_sizes_given_as_a_list(backend, color):
    B, V, T, Hs, Ws, Ho, Wo = 2, 2, 2, 40, 56, 24, 17
    pipe = _pipe(V, T, Ho, Wo, color)
    samples = [_sample(V * T, Hs, Ws, 7 + b) for b in range(B)]
    outs = []
    for frames in ([backend.d(torch.from_numpy(s)) for s in samples], backend.d(torch.from_numpy(np.stack(samples)))):
        np.random.seed(3)
        random.seed(3)
        outs.append(_run(backend.lib, pipe, frames, want_x4=True))
    lst, dense = outs
    assert np.array_equal(lst['boxes'], dense['boxes']) and np.array_equal(lst['flips'], dense['flips'])
    assert lst['shapes'] == dense['shapes'] == [(Hs, Ws)] * B
    if color:
        assert np.array_equal(lst['photo_rows'], dense['photo_rows']) and lst['photo_rows'].any()
    for a, b in zip(_bits(lst), _bits(dense)):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------------------------------- 4: RNG order

def _rng_state():
    return np.random.get_state(), random.getstate()


def _same_state(a, b):
    return a[0][0] == b[0][0] and np.array_equal(a[0][1], b[0][1]) and a[0][2:] == b[0][2:] and a[1] == b[1]


@pytest.mark.parametrize('color', [False, True], ids=['plain', 'color'])
def test_rng_order_is_sample_by_sample(color):
    """pipe(list) consumes np.random and random as B successive sample(F, shape_i) calls do (the reference's order for a
    batch), and nothing else touches them.  No kernel runs."""
    V, T = 2, 2
    shapes = [(30, 44), (52, 31), (17, 17)]
    pipe = _pipe(V, T, 8, 8, color)
    np.random.seed(11)
    random.seed(11)
    draws = [pipe.sample(V * T, s) for s in shapes]
    after = _rng_state()
    np.random.seed(11)
    random.seed(11)
    out = _run(Recorder(), pipe, [np.zeros((V * T, h, w, 3), np.uint8) for h, w in shapes])
    assert _same_state(_rng_state(), after)
    assert np.array_equal(out['boxes'], np.concatenate([d[0] for d in draws]))
    assert np.array_equal(out['flips'], np.concatenate([d[1] for d in draws]))
    assert len({tuple(b) for b in out['boxes']}) > 1 and out['shapes'] == shapes
    if color:
        for k in draws[0][2]:
            assert np.array_equal(out['photo'][k], np.concatenate([d[2][k] for d in draws]), equal_nan=True), k


# ------------------------------------------------------------------------------------------------- 5: pack_frames

def test_pack_frames_host_inputs():
    arrs = [_sample(3, Hs, Ws, 40 + i) for i, (Hs, Ws) in enumerate(SIZES)]
    want = np.concatenate([a.reshape(-1) for a in arrs])
    a = pack_frames(arrs)
    b = pack_frames([torch.from_numpy(x) for x in arrs])
    c = pack_frames([torch.from_numpy(x) if i % 2 else x for i, x in enumerate(arrs)])
    for p in (a, b, c):
        assert isinstance(p, PackedFrames) and p.buffer.dtype == torch.uint8 and p.buffer.dim() == 1
        assert np.array_equal(p.buffer.numpy(), want)
        assert p.shapes == SIZES and p.offsets == [0] + [int(v) for v in np.cumsum([x.size for x in arrs])[:-1]]
        assert all(isinstance(o, int) for o in p.offsets)
    # the caller's staging buffer is used when it is large enough, replaced when it is not
    big, small = torch.zeros(want.size + 64, dtype=torch.uint8), torch.zeros(want.size - 1, dtype=torch.uint8)
    p = pack_frames(arrs, pinned=big)
    assert p.buffer.data_ptr() == big.data_ptr() and np.array_equal(big.numpy()[:want.size], want) and p.buffer.numel() == want.size
    q = pack_frames(arrs, pinned=small)
    assert np.array_equal(q.buffer.numpy(), want) and not small.any()


def test_packed_frames_are_read_in_place():
    V, T = 1, 3
    packed = pack_frames([_sample(V * T, Hs, Ws, 50 + i) for i, (Hs, Ws) in enumerate(SIZES)])
    rec = Recorder()
    out = _run(rec, _pipe(V, T, HO, WO), packed)
    (name, args), = rec.calls
    assert name == 'crop_resize_flip_norm_ragged' and args[0] is packed.buffer and args[1] == packed.buffer.numel()
    desc = args[2].numpy().reshape(-1, 4)
    assert desc[:, 0].tolist() == packed.offsets and not desc[:, 1].any() and [tuple(r) for r in desc[:, 2:].tolist()] == SIZES
    assert out['shapes'] == SIZES and out['boxes'].shape == (len(SIZES) * V * T, 4)


@pytest.mark.gpu
def test_pack_frames_device(gpu_backend):
    dev = gpu_backend.dev
    arrs = [_sample(3, Hs, Ws, 40 + i) for i, (Hs, Ws) in enumerate(SIZES)]
    want = np.concatenate([a.reshape(-1) for a in arrs])
    host = pack_frames(arrs, device=dev)                                   # staged and uploaded
    ondev = pack_frames([torch.from_numpy(a).to(dev) for a in arrs])       # concatenated where they are
    pinned = torch.zeros(want.size + 64, dtype=torch.uint8).pin_memory()
    reuse = pack_frames([torch.from_numpy(a) for a in arrs], device=dev, pinned=pinned)
    torch.cuda.synchronize()
    for p in (host, ondev, reuse):
        assert p.buffer.device == dev and np.array_equal(p.buffer.cpu().numpy(), want)
        assert p.shapes == host.shapes == SIZES and p.offsets == host.offsets
    assert np.array_equal(pinned.numpy()[:want.size], want)
    rec = Recorder(gpu_backend.lib)
    _run(rec, _pipe(1, 3, HO, WO), ondev)
    assert rec.calls[0][1][0].data_ptr() == ondev.buffer.data_ptr()


# --------------------------------------------------------------------------------------------- 6: host validation

def test_host_validation_names_the_sample():
    V, T = 2, 2
    pipe = _pipe(V, T, HO, WO)
    good = [np.zeros((V * T, h, w, 3), np.uint8) for h, w in SIZES[:3]]

    def bad(i, arr):
        return good[:i] + [arr] + good[i + 1:]
    rec = Recorder()
    with pytest.raises(ValueError, match='sample 1'):
        _run(rec, pipe, bad(1, np.zeros((V * T + 1, 33, 16, 3), np.uint8)))                    # a wrong frame count
    with pytest.raises(ValueError, match='sample 2'):
        _run(rec, pipe, bad(2, np.zeros((V * T, 1, 3, 3), np.float32)))                        # a wrong dtype
    with pytest.raises(ValueError, match='sample 0'):
        _run(rec, pipe, bad(0, torch.zeros(V * T, 5, 7, 4, dtype=torch.uint8)))                # four channels
    with pytest.raises(ValueError, match='sample 1'):
        _run(rec, pipe, bad(1, torch.zeros(V * T, 33, 16, 3, dtype=torch.uint8, device='meta')))     # two devices
    packed = pack_frames(good)
    with pytest.raises(ValueError, match='sample 2'):                                          # an offset past the buffer
        _run(rec, pipe, PackedFrames(packed.buffer, packed.offsets[:2] + [packed.offsets[2] + 1], packed.shapes))
    with pytest.raises(ValueError, match='sample 0'):
        _run(rec, pipe, PackedFrames(packed.buffer, [-1] + packed.offsets[1:], packed.shapes))
    assert rec.calls == []          # refused before anything is uploaded or launched
    assert _run(rec, pipe, packed)['shapes'] == SIZES[:3] and len(rec.calls) == 1


# ------------------------------------------------------------------------- 7: descriptor guard (CPU emulator only)

BAD_ROWS = {'overrun': None,                                        # the sample's last byte lies behind src_bytes
            'Hs0': lambda off, Hs, Ws: (off, 0, Ws),
            'Ws-negative': lambda off, Hs, Ws: (off, Hs, -Ws),
            'offset-negative': lambda off, Hs, Ws: (-1, Hs, Ws),
            'offset-behind': lambda off, Hs, Ws: (1 << 40, Hs, Ws),
            'size-overflows': lambda off, Hs, Ws: (off, 0x7FFFFFFF, 0x7FFFFFFF)}


@pytest.mark.parametrize('color', [False, True], ids=['plain', 'color'])
@pytest.mark.parametrize('how', sorted(BAD_ROWS))
def test_descriptor_guard(emu_backend, how, color):
    """three samples, the second with a bad row: it reads nothing and gets zeros (imgs, x4 and its pad column), the other
    two keep the bits of the per-sample runs.  The memory behind src_bytes is 255: a read past the end would show."""
    V, T = 2, 2
    F, B = V * T, 3
    c = _case(emu_backend, V, T, color)
    order = [0, 2, 1]                               # sample 1 lies last in the buffer: cutting it short hurts nobody else
    offs, pos = {}, 1                               # an odd first offset
    for b in order:
        offs[b] = pos
        pos += c['samples'][b].size
    src_bytes = pos - 1 if how == 'overrun' else pos
    buf = np.full(pos + 4096, 255, np.uint8)
    for b in order:
        buf[offs[b]:offs[b] + c['samples'][b].size] = c['samples'][b].reshape(-1)
    buf[src_bytes:] = 255
    rows = [(offs[b],) + SIZES[b] for b in range(B)]
    if BAD_ROWS[how] is not None:
        rows[1] = BAD_ROWS[how](*rows[1])
    desc = torch.tensor([[(o & 0xFFFFFFFF) - ((o & 0x80000000) << 1), o >> 32, h, w] for o, h, w in rows], dtype=torch.int32)
    boxes, flips = torch.from_numpy(c['boxes'][:B * F].copy()), torch.from_numpy(c['flips'][:B * F].copy())
    imgs, x4 = torch.full((B, V, 3, T, HO, WO), 7.0), torch.full((V * B * T, HO, WP, 4), 7.0, dtype=torch.bfloat16)
    lib, src = emu_backend.lib, torch.from_numpy(buf)
    if color:
        nb = torch.zeros(1, dtype=torch.int64)
        lib.crop_resize_flip_photo_norm_workspace_bytes(B * F, HO, WO, nb)
        ws = torch.zeros(int(nb), dtype=torch.uint8)
        lib.crop_resize_flip_photo_norm_ragged(src, src_bytes, desc, boxes, flips, torch.from_numpy(c['rows'][:B * F].copy()), ws,
                                               ws.numel(), imgs, x4, B, V, T, HO, WO, WP, *MEAN, *STD, None)
    else:
        lib.crop_resize_flip_norm_ragged(src, src_bytes, desc, boxes, flips, imgs, x4, B, V, T, HO, WO, WP, *MEAN, *STD, None)
    gi, gx = imgs.numpy().view(np.uint32), x4.view(torch.int16).numpy()
    assert not gi[1].any(), 'imgs of the invalid sample'
    assert not gx.reshape(V, B, T, HO, WP, 4)[:, 1].any(), 'x4 of the invalid sample, pad column included'
    for b in (0, 2):
        _assert_sample(gi, gx, b, B, V, T, c['per'][b])


# --------------------------------------------------------------------------------------- 8: C argument checks

def _c_cases():
    P = torch.zeros(16384)
    norm = (123.675, 116.28, 103.53, 58.395, 57.12, 57.375, None)
    shape = (P, P, 1, 2, 1, 4, 4, 4)             # imgs, x4, B, V, T, Ho, Wo, Wp
    plain, photo = 'crop_resize_flip_norm_ragged', 'crop_resize_flip_photo_norm_ragged'
    cases = []
    for who, mid in ((plain, (P, P)), (photo, (P, P, P, P, 1 << 20))):        # boxes, flips(, photo, workspace, workspace_bytes)
        cases += [(f'{who}-null-src', who, (None, 64, P) + mid + shape + norm, ARG, f'{who}: null buffer'),
                  (f'{who}-null-srcdesc', who, (P, 64, None) + mid + shape + norm, ARG, f'{who}: null buffer'),
                  (f'{who}-src_bytes0', who, (P, 0, P) + mid + shape + norm, ARG, f'{who}: null buffer'),
                  (f'{who}-no-output', who, (P, 64, P) + mid + (None, None) + shape[2:] + norm, ARG, f'{who}: null buffer'),
                  (f'{who}-Wp', who, (P, 64, P) + mid + (None, P, 1, 2, 1, 4, 4, 3) + norm, SHAPE, f'{who}: Wp < Wo')]
    small = f'{photo}: workspace smaller than vfs_crop_resize_flip_photo_norm_workspace_bytes'
    cases += [(f'{photo}-workspace', photo, (P, 64, P, P, P, P, P, 8) + shape + norm, ARG, small),
              (f'{photo}-null-workspace', photo, (P, 64, P, P, P, P, None, 1 << 20) + shape + norm, ARG, small),
              (f'{photo}-null-photo', photo, (P, 64, P, P, P, None, P, 1 << 20) + shape + norm, ARG, f'{photo}: null buffer'),
              (f'{photo}-empty', photo, (P, 64, P, P, P, P, P, 1 << 20, P, P, 0, 2, 1, 4, 4, 4) + norm, SHAPE, f'{photo}: empty batch'),
              (f'{photo}-frames', photo, (P, 64, P, P, P, P, P, 1 << 40, P, P, 65536, 1, 1, 1, 1, 2) + norm, SHAPE,
               'photo pipeline: at most 65535 frames per launch'),
              (f'{plain}-empty', plain, (P, 64, P, P, P, P, P, 0, 2, 1, 4, 4, 4) + norm, SHAPE, 'pipeline: empty batch')]
    return [pytest.param(*c[1:], id=c[0]) for c in cases]


@pytest.mark.parametrize('name,args,code,message', _c_cases())
def test_c_argument_checks(emu_backend, name, args, code, message):
    """code and vfs_last_error() text of the uniform entry points' checks, under the ragged entry's name; each returns before
    anything is launched (the descriptor table is never read: the arguments point at zeros)"""
    lib = emu_backend.lib
    fn = lib.cfunc(name)
    assert len(args) == len(lib.protos['vfs_' + name][1]), 'the case does not match the prototype'
    rc = fn(*[a.data_ptr() if hasattr(a, 'data_ptr') else a for a in args])
    assert (rc, lib.last_error()) == (code, message)


# ---------------------------------------------------------------------------------------------------- 9, 10: GPU

K400 = [(256, 340), (256, 454), (340, 256), (256, 342)]


@pytest.mark.gpu
@pytest.mark.parametrize('color', [False, True], ids=['plain', 'color'])
def test_kinetics_sized_batch(gpu_backend, color):
    """B = 8 pairs at the sizes DecordDecode returns for Kinetics-400 -> 224x224, sampled decisions, one C call (one launch
    plain, two with the photometric steps), against the oracle sample by sample"""
    B, V, T = 8, 2, 1
    shapes = [K400[b % 4] for b in range(B)]
    samples = [_sample(V * T, h, w, 60 + b) for b, (h, w) in enumerate(shapes)]
    pipe = _pipe(V, T, 224, 224, color)
    np.random.seed(9)
    random.seed(9)
    rec = Recorder(gpu_backend.lib)
    out = _run(rec, pipe, samples, device=gpu_backend.dev, want_x4=True)
    assert [n for n, _ in rec.calls if 'workspace' not in n] == ['crop_resize_flip_photo_norm_ragged' if color else 'crop_resize_flip_norm_ragged']
    assert out['shapes'] == shapes
    rows = out['photo_rows'] if color else None
    if color:
        assert rows[:, 0].any() and rows[:, 6].any()
    imgs = out['imgs'].cpu().numpy().view(np.uint32)
    want = np.stack([_oracle_sample(samples[b], out['boxes'][b * 2:b * 2 + 2], out['flips'][b * 2:b * 2 + 2],
                                    None if rows is None else rows[b * 2:b * 2 + 2], V, T, 224, 224) for b in range(B)])
    bad = np.argwhere(imgs != want.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:4].tolist())
    x4 = torch.full((V * B * T, 224, 224, 4), 7.0, dtype=torch.bfloat16)
    gpu_backend.hostlib.imgs_to_nhwc4(torch.from_numpy(want), x4, B, V, T, 224, 224, 224, None)
    assert torch.equal(out['x4'].cpu().view(torch.int16), x4.view(torch.int16))


@pytest.mark.gpu
def test_mixed_sizes_feed_train_step(gpu_backend):
    """a mixed-size list -> GpuTrainPipeline (the shipped config's train_pipeline at 64x64) -> train_step: imgs equal the
    per-sample oracle bit for bit, the step gives a finite loss and the log vars of the oracle-fed step"""
    import vfs_amd
    cfg = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', 'vfs_r18.py'))
    tp = [dict(s) for s in cfg.train_pipeline]
    for s in tp:
        if s['type'] == 'Resize':
            s['scale'] = (64, 64)
    pipe = GpuTrainPipeline(tp)
    V, T = pipe.num_clips, pipe.clip_len
    assert (V, T) == (2, 4)
    shapes = [(72, 96), (96, 72), (80, 107), (64, 64)]
    B, F = len(shapes), V * T
    samples = [_sample(F, h, w, 21 + b) for b, (h, w) in enumerate(shapes)]
    np.random.seed(1)
    random.seed(1)
    out = pipe(samples, device=gpu_backend.dev)
    want = np.stack([_oracle_sample(samples[b], out['boxes'][b * F:(b + 1) * F], out['flips'][b * F:(b + 1) * F], None, V, T, 64, 64,
                                    pipe.mean, pipe.std) for b in range(B)])
    assert np.array_equal(out['imgs'].cpu().numpy().view(np.uint32), want.view(np.uint32))
    model = vfs_amd.build_model(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(gpu_backend.dev).train()
    res = model.train_step(dict(imgs=out['imgs'], label=torch.zeros(B, 1)), None)
    res['loss'].backward()
    assert np.isfinite(res['log_vars']['loss']) and res['num_samples'] == B
    res2 = model.train_step(dict(imgs=torch.from_numpy(want).to(gpu_backend.dev), label=torch.zeros(B, 1)), None)
    assert res2['log_vars'].keys() == res['log_vars'].keys()
