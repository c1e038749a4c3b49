"""SiamFC probe, tracking loop on the device (csrc/siamfc_track.hip; SiamFCProbe(device_loop=True)): the search crops, the cubic
up-sampling of the responses and the peak search against the host loop of vfs_amd/siamfc.py (crop_and_resize, resize_cubic and
the numpy tail of SiamFCProbe.update), which is the yardstick - the reference's own loop needs cv2.  backend=emu (CPU) / gpu."""
import numpy as np
import pytest
import torch

from vfs_amd import siamfc as SF
from vfs_amd._lib import VfsError

U = 2.0 ** -24      # unit round-off of fp32
UP = 272
SCALE_FACTORS = SF.DEFAULT_CFG['scale_step'] ** np.linspace(-1, 1, 3)
PENALTY = np.array([SF.DEFAULT_CFG['scale_penalty'], 1.0, SF.DEFAULT_CFG['scale_penalty']], np.float32)
WI = SF.DEFAULT_CFG['window_influence']


def _hann():
    h = np.outer(np.hanning(UP), np.hanning(UP))      # SiamFCProbe.init
    return h / h.sum()


# ---------------------------------------------------------------------------------------------
# 1. crops
# ---------------------------------------------------------------------------------------------
def _frame(h=240, w=320, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _device_crops(backend, frame, center, sizes, out_size, avg):
    params = np.stack([SF.crop_params(frame.shape, center, s, out_size, avg) for s in sizes])
    out = torch.full((len(sizes), 3, out_size, out_size), -1.0)
    backend.hostlib.siamfc_crops(torch.from_numpy(frame), params.ctypes.data, out, frame.shape[0], frame.shape[1], len(sizes), out_size, None)
    return out.numpy(), params


def _host_crops(frame, center, sizes, out_size, avg):
    return np.stack([np.asarray(SF.crop_and_resize(frame, center, s, out_size, avg), dtype=np.float32) for s in sizes]).transpose(0, 3, 1, 2)


CROP_CASES = {      # (centre (y, x), box size) on a 240 x 320 frame; every case runs at the three scale factors of the probe
    'inside': ((120.0, 160.0), 80.0),
    'inside_fractional': ((97.3, 201.8), 61.7),
    'left': ((120.0, 20.0), 100.0),
    'right': ((120.0, 310.0), 100.0),
    'top': ((10.0, 160.0), 100.0),
    'bottom': ((235.0, 160.0), 100.0),
    'top_left': ((5.0, 5.0), 90.0),
    'bottom_right': ((236.5, 317.5), 75.0),
    'larger_than_image': ((120.0, 160.0), 700.0),
    'size_below_2': ((100.0, 100.0), 0.5),
    'size_below_2_at_the_corner': ((0.2, 0.4), 1.0),
    'outside_right': ((120.0, 500.0), 60.0),
    'outside_below': ((400.0, 160.0), 60.0),
    'outside_above_left': ((-100.0, -100.0), 50.0),
    'touching_from_outside': ((120.0, -30.0), 60.0),
}


@pytest.mark.parametrize('out_size', [255, 120])
def test_crops_equal_host_bytes(backend, out_size):
    """vfs_siamfc_crops == crop_and_resize, every byte, three scale factors per launch: boxes inside the frame, across each
    border and two at once, larger than the frame, size < 2 (clamped to 2), and fully outside (zeros)."""
    frame = _frame()
    avg = np.mean(frame, axis=(0, 1))
    seen_fill = seen_zero = seen_resized = False
    for name, (center, size) in CROP_CASES.items():
        sizes = [size * f for f in SCALE_FACTORS]
        got, params = _device_crops(backend, frame, center, sizes, out_size, avg)
        want = _host_crops(frame, center, sizes, out_size, avg)
        assert got.shape == want.shape, name
        assert np.array_equal(got, want), (name, out_size, int((got != want).sum()), float(np.abs(got - want).max()))
        seen_zero |= not params[:, 0].any()
        seen_fill |= bool((params[:, 0] == 1).any() and (params[:, 7:9] > 0).any())
        seen_resized |= bool((params[:, 0] == 1).any() and (params[:, 3] != params[:, 5]).any())
    assert seen_zero and seen_fill and seen_resized      # the cases reach the three branches of the kernel


def test_crops_one_scale_and_refusals(backend):
    """S = 1 (the exemplar crop of init()); a parameter row whose patch or target rectangle leaves its array is refused by the
    launcher instead of being read out of bounds"""
    frame = _frame(96, 128, seed=3)
    avg = np.mean(frame, axis=(0, 1))
    got, params = _device_crops(backend, frame, (40.0, 100.0), [70.0], 120, avg)
    assert np.array_equal(got, _host_crops(frame, (40.0, 100.0), [70.0], 120, avg))
    out = torch.zeros(1, 3, 120, 120)
    for col, val in ((1, 100), (2, -1), (4, 97), (5, 121), (7, 120), (8, -1)):
        bad = params.copy()
        bad[0, col] = val
        with pytest.raises(VfsError):
            backend.hostlib.siamfc_crops(torch.from_numpy(frame), bad.ctypes.data, out, 96, 128, 1, 120, None)


# ---------------------------------------------------------------------------------------------
# 2. up-sampling
# ---------------------------------------------------------------------------------------------
def _responses(seed, magnitude, r=17):
    return (np.random.default_rng(seed).standard_normal((3, r, r)) * magnitude).astype(np.float32)


def _key_decode(keys):
    """scale_max of vfs_siamfc_upsample (include/vfs_hip.h) -> (maximum, flat index)"""
    k = keys.numpy().view(np.uint64)
    u = (k >> np.uint64(32)).astype(np.uint32)
    bits = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7fffffff), ~u).astype(np.uint32)
    return bits.view(np.float32), (np.uint32(0xffffffff) - (k & np.uint64(0xffffffff)).astype(np.uint32)).astype(np.int64)


def _device_upsample(backend, resp, penalty):
    S, r = resp.shape[0], resp.shape[-1]
    idx, w = SF._cubic_taps(r, UP)
    up = torch.zeros(S, UP, UP)
    keys = torch.full((S,), -1, dtype=torch.int64)      # stale keys of an earlier frame must not survive
    backend.hostlib.siamfc_upsample(torch.from_numpy(resp), torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(w),
                                    torch.from_numpy(np.asarray(penalty, np.float32)), up, keys, S, r, UP, None)
    return up, keys


MAGNITUDES = [1.0, 1e-3, 3e-5, 40.0]      # out_scale = 0.001 puts trained responses in the 1e-3 .. 1e-5 range


@pytest.mark.parametrize('magnitude', MAGNITUDES)
def test_upsample_matches_resize_cubic(backend, magnitude):
    """vfs_siamfc_upsample against resize_cubic, [3,17,17] -> [3,272,272]:  max|diff| <= 32 u max|a|,  u = 2^-24.

    Each pass is four fp32 products and three adds: relative error gamma_4 ~ 4u on a sum whose absolute terms add up to at most
    sum|w| * max|input|, and sum|w| <= 1.375 for the Keys kernel with A = -0.75 (reached at t = 0.5).  The horizontal pass
    therefore returns values bounded by 1.375 max|a| with error <= 4u * 1.375 max|a| = 5.5u max|a|; the vertical pass amplifies
    that by 1.375 (7.6u) and adds 4u * 1.375 * 1.375 max|a| = 7.6u of its own: each implementation is within ~15.1u max|a| of
    the exact cubic (whose values are bounded by 1.89 max|a|), two implementations within 32u max|a| of each other.
    Observed, emulator and MI355X: the difference is exactly 0 for every magnitude - the kernel's ((p0 + p1) + p2) + p3 is the
    order in which numpy sums four elements.

    The penalty is one more fp32 multiplication of the same value (exact against the kernel's own unpenalised output), and
    scale_max is the maximum of the kernel's own penalised map at its lowest flat index."""
    a = _responses(11, magnitude)
    got, _ = _device_upsample(backend, a, np.ones(3))
    want = np.stack([SF.resize_cubic(m, UP, UP) for m in a])
    diff = float(np.abs(got.numpy().astype(np.float64) - want).max())
    bound = 32 * U * float(np.abs(a).max())
    print(f'upsample magnitude {magnitude:g}: max|diff| {diff:.3e} (bound {bound:.3e}), bit-equal: {np.array_equal(got.numpy(), want)}')
    assert diff <= bound
    pen, keys = _device_upsample(backend, a, PENALTY)
    assert np.array_equal(pen.numpy(), got.numpy() * PENALTY[:, None, None])
    val, idx = _key_decode(keys)
    flat = pen.numpy().reshape(3, -1)
    assert np.array_equal(val, flat.max(1)) and np.array_equal(idx, flat.argmax(1))


def test_upsample_lowest_index_of_equal_maxima(backend):
    """a constant map: every up-sampled value is the maximum, the key must name flat index 0; 18 x 18 maps (what the dilated
    backbone yields for 255 / 120 pixel crops) go through the same kernel"""
    a = np.full((2, 18, 18), 0.25, np.float32)
    a[1] = _responses(5, 1.0, r=18)[0]
    up, keys = _device_upsample(backend, a, np.ones(2))
    val, idx = _key_decode(keys)
    flat = up.numpy().reshape(2, -1)
    assert np.array_equal(val, flat.max(1)) and np.array_equal(idx, flat.argmax(1))
    assert np.array_equal(up.numpy(), np.stack([SF.resize_cubic(m, UP, UP) for m in a]))


# ---------------------------------------------------------------------------------------------
# 3. peak
# ---------------------------------------------------------------------------------------------
def _host_upsampled(resp):
    """SiamFCProbe.update: the up-sampled, penalised maps"""
    up = np.stack([SF.resize_cubic(u, UP, UP) for u in resp])
    n = len(resp)
    up[:n // 2] *= SF.DEFAULT_CFG['scale_penalty']
    up[n // 2 + 1:] *= SF.DEFAULT_CFG['scale_penalty']
    return up


def _host_blend(up_s, hann):
    """SiamFCProbe.update on the chosen scale: the blended map whose argmax is the new location, and the intermediates the
    tolerance is built from"""
    response = up_s.copy()
    response -= response.min()
    y = response.copy()
    den = response.sum() + 1e-16
    response /= den
    return (1 - WI) * response + WI * hann, y, float(den)


def _peak_tolerance(resp, up_s, y, den, blended):
    """How far below the host's maximum the host's blended map may be at the device's argmax.

    eps  = 32u max|a| + 2u max|U|: the up-sampling bound of test_upsample_matches_resize_cubic, plus the rounding of the penalty
           multiplication on either side (U: the host's penalised map, D: the device's; |U - D| <= eps elementwise)
    Y = fl(U - min U):   |min D - min U| <= eps, so dY = 2 eps + 2u (max Y + 2 eps)
    den = fl(sum Y) + 1e-16: the host sums in fp32 pairwise (error <= 64u sum Y, generous for numpy's 128-element blocks of 8
           partial sums and log2(n / 128) levels), the device in fp64 rounded once (u sum Y), one more rounding for the 1e-16:
           dden = n dY + 66u den + 2u den
    Q = fl(Y / den):     dQ = dY / den_lo + max Y * dden / (den * den_lo) + 2u max Q',  den_lo = den - dden > 0,
                                                                                       max Q' = (max Y + dY) / den_lo
    B = fl((1 - wi) Q) + wi hann (fp64): dB = (1 - wi) dQ + 2u (1 - wi) max Q' + 2^-50 max B
    The device returns the argmax of its own map B':  B(loc') >= B'(loc') - dB >= B'(loc*) - dB >= B(loc*) - 2 dB  ->  tol = 2 dB."""
    n = up_s.size
    eps = 32 * U * float(np.abs(resp).max()) + 2 * U * float(np.abs(up_s).max())
    ymax = float(y.max())
    dy = 2 * eps + 2 * U * (ymax + 2 * eps)
    dden = n * dy + 68 * U * den
    den_lo = den - dden
    assert den_lo > 0, 'degenerate map: the tolerance formula needs a positive denominator'
    qmax = (ymax + dy) / den_lo
    dq = dy / den_lo + ymax * dden / (den * den_lo) + 2 * U * qmax
    db = (1 - WI) * dq + 2 * U * (1 - WI) * qmax + 2.0 ** -50 * float(blended.max())
    return 2 * db


def _device_peak(backend, resp):
    up, keys = _device_upsample(backend, resp, PENALTY)
    rec = torch.full((4,), -1, dtype=torch.int32)
    backend.hostlib.siamfc_peak(up, keys, torch.from_numpy(_hann()), rec, resp.shape[0], UP, float(np.float32(1 - WI)), float(WI), None)
    assert int(rec[3]) == 0
    return tuple(int(v) for v in rec[:3])


def check_peak(resp, triple, hann):
    """the near-argmax criteria for a device triple on raw responses `resp` [S,r,r]; -> the host's own triple"""
    sid, row, col = triple
    up = _host_upsampled(resp)
    hm = np.amax(up, axis=(1, 2))
    assert 0 <= sid < len(resp) and 0 <= row < UP and 0 <= col < UP
    assert hm[sid] >= hm.max() - 32 * U * float(np.abs(resp).max()), (triple, hm)
    blended, y, den = _host_blend(up[sid], hann)
    tol = _peak_tolerance(resp, up[sid], y, den, blended)
    assert tol < 1e-3 * (blended.max() - blended.min()), 'the tolerance must stay a small fraction of the map'
    assert blended[row, col] >= blended.max() - tol, (triple, float(blended[row, col]), float(blended.max()), tol)
    hsid = int(np.argmax(hm))
    hloc = np.unravel_index(_host_blend(up[hsid], hann)[0].argmax(), (UP, UP))
    return hsid, int(hloc[0]), int(hloc[1])


def _planted(seed, magnitude, scale, cell):
    a = _responses(seed, 0.05 * magnitude)
    a[scale, cell[0], cell[1]] = magnitude
    return a


def test_peak_near_argmax_of_host_map(backend):
    """vfs_siamfc_upsample + vfs_siamfc_peak against the numpy tail of SiamFCProbe.update on the same raw responses.

    scale_id:  host penalised maximum at the device's scale >= best host maximum - 32u max|a|
    (row, col): host blended map (for the device's scale) at the device's location >= its maximum - tol, tol computed by
                _peak_tolerance from the host's intermediates (formula in its docstring; no tuned constant)
    planted peak / exact tie between two scales (identical maps at scales 0 and 2, both penalised: the lower index wins, as
    np.argmax): the triple equals the host's exactly.
    Observed: every triple equals the host's, 12 of 12 (emulator and MI355X)."""
    hann = _hann()
    equal = total = 0
    for magnitude in MAGNITUDES:
        for seed in (21, 22):
            resp = _responses(seed, magnitude)
            triple = _device_peak(backend, resp)
            host = check_peak(resp, triple, hann)
            equal += triple == host
            total += 1
    exact = [_planted(31, 1e-3, 2, (4, 12)), _planted(32, 1.0, 0, (15, 1)), _planted(33, 3e-5, 1, (8, 8))]
    tie = _planted(34, 1e-3, 0, (6, 9))
    tie[2] = tie[0]
    tie[1] *= 0.5
    for resp in exact + [tie]:
        triple = _device_peak(backend, resp)
        host = check_peak(resp, triple, hann)
        assert triple == host, (triple, host)
        equal += 1
        total += 1
    assert _device_peak(backend, tie)[0] == 0
    print(f'peak: {equal} of {total} triples equal the host loop\'s exactly')


def test_peak_tie_goes_to_lowest_flat_index(backend):
    """two equal maxima of the blended map: the Hann window is symmetric under transposition (an outer product of one vector),
    so equal values at (r, c) and (c, r) tie exactly; the winner is the lower flat index, as np.argmax"""
    hann = _hann()
    assert np.array_equal(hann, hann.T)
    up = np.random.default_rng(41).random((3, UP, UP)).astype(np.float32) * 0.1
    up[1, 100, 180] = up[1, 180, 100] = 1.0
    keys = np.zeros(3, np.uint64)
    for s in range(3):      # the key format of include/vfs_hip.h (positive floats: bits | 0x80000000)
        flat = up[s].reshape(-1)
        keys[s] = (np.uint64(flat.max().view(np.uint32) | np.uint32(0x80000000)) << np.uint64(32)) | np.uint64(0xffffffff - int(flat.argmax()))
    rec = torch.full((4,), -1, dtype=torch.int32)
    backend.hostlib.siamfc_peak(torch.from_numpy(up), torch.from_numpy(keys.view(np.int64)), torch.from_numpy(hann), rec, 3, UP,
                                float(np.float32(1 - WI)), float(WI), None)
    blended = _host_blend(up[1], hann)[0]
    assert blended[100, 180] == blended[180, 100] == blended.max()
    assert rec.tolist() == [1, 100, 180, 0]


# ---------------------------------------------------------------------------------------------
# 4. the loop
# ---------------------------------------------------------------------------------------------
def _sequence(frames=7):
    """a textured 40 x 40 target that moves (3, 4) pixels per frame over a textured background"""
    rng = np.random.default_rng(51)
    coarse = rng.integers(30, 140, (30, 40, 3)).astype(np.float64)
    bg = np.kron(coarse, np.ones((8, 8, 1))) + rng.integers(-12, 13, (240, 320, 3))
    tcoarse = rng.integers(150, 255, (5, 5, 3)).astype(np.float64)
    target = np.kron(tcoarse, np.ones((8, 8, 1))) + rng.integers(-10, 11, (40, 40, 3))
    out = []
    for t in range(frames):
        img = bg.copy()
        img[100 + 3 * t:140 + 3 * t, 150 + 4 * t:190 + 4 * t] = target
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out, [151, 101, 40, 40]


def _probes(dev):
    import vfs_amd
    from oracle import vfs_oracle as O
    cfg = dict(out_channels=512, batch_size=2, exemplar_sz=120, instance_sz=255)
    torch.manual_seed(7)      # the head's initial weights: every pair of probes gets the same
    host = vfs_amd.SiamFCProbe(cfg, depth=18, device=dev)
    ref = O.ResNet(18, strides=(1, 2, 1, 1), dilations=(1, 1, 2, 4), out_indices=(3,), zero_init_residual=False)
    O.fill_state_dict_(ref, seed=118)
    host.backbone.load_state_dict(ref.state_dict())
    device = vfs_amd.SiamFCProbe(cfg, depth=18, device=dev, backbone=host.backbone, device_loop=True)
    device.head.load_state_dict(host.head.state_dict())
    return host, device


def _spy(probe):
    seen = []
    inner = probe._apply_peak

    def apply_peak(scale_id, loc):
        seen.append((int(scale_id), int(loc[0]), int(loc[1])))
        return inner(scale_id, loc)
    probe._apply_peak = apply_peak
    return seen


def test_device_loop_against_host_loop(backend):
    """SiamFCProbe(device_loop=True) on a ResNet-18 probe, 7 frames of a moving textured target.

    teacher-forced: with the host probe's state copied in before every frame, the device loop's search crops equal the host's
        bytes and its triple meets the criteria of test_peak_near_argmax_of_host_map on the responses it was computed from
    free-running: track() returns [T,4] float64, finite, frame 0 the input box; up to the first frame whose triple differs
        from the host loop's, the boxes are identical
    buffer reuse: the per-frame buffers keep their addresses and the allocator's counters do not grow over frames 2..T
    Observed on the MI355X: 6 of 6 teacher-forced triples equal the numpy tail's, 6 of 6 free-running frames equal the host loop's."""
    if backend.name == 'emu':
        pytest.skip('full ResNet-18 at 120 / 255 pixel crops: minutes on the emulator; runs on the GPU')
    frames, box = _sequence()
    hann = _hann()
    host, device = _probes(backend.dev)
    assert host.device_loop is False and device.device_loop is True
    host.init(frames[0], box)
    device.init(frames[0], box)
    c = host.cfg
    z = SF.crop_and_resize(frames[0], host.center, host.z_sz, c['exemplar_sz'], host.avg_color)
    assert np.array_equal(device._dl['z'].cpu().numpy()[0], np.asarray(z, np.float32).transpose(2, 0, 1))
    equal = 0
    for img in frames[1:]:
        device.center, device.target_sz = host.center.copy(), host.target_sz.copy()
        device.z_sz, device.x_sz = host.z_sz, host.x_sz
        x = np.stack([SF.crop_and_resize(img, host.center, host.x_sz * f, c['instance_sz'], host.avg_color) for f in host.scale_factors])
        device.update(img)
        assert np.array_equal(device._dl['x'].cpu().numpy(), x.astype(np.float32).transpose(0, 3, 1, 2))
        resp = device._dl['responses'].squeeze(1).cpu().numpy()
        equal += check_peak(resp, device.last_peak, hann) == device.last_peak
        host.update(img)
    print(f'teacher-forced: {equal} of {len(frames) - 1} triples equal the numpy tail\'s on the same responses')

    host, device = _probes(backend.dev)
    hseen, dseen = _spy(host), _spy(device)
    hboxes = host.track(frames, box)
    torch.cuda.synchronize()
    device.init(frames[0], box)
    dboxes, stats, ptrs = [np.asarray(box, dtype=np.float64)], [], []
    for img in frames[1:]:
        dboxes.append(device.update(img))
        stats.append((torch.cuda.memory_allocated(), torch.cuda.memory_reserved()))
        ptrs.append({k: v.data_ptr() for k, v in device._dl.items() if isinstance(v, torch.Tensor) and k != 'responses'})
    for s, p in zip(stats[1:], ptrs[1:]):
        assert s[0] <= stats[0][0] and s[1] <= stats[0][1], stats
        assert p == ptrs[0]
    dboxes = np.stack(dboxes)
    host2, device2 = _probes(backend.dev)
    tboxes = device2.track(frames, box)
    assert tboxes.shape == (len(frames), 4) and tboxes.dtype == np.float64 and np.isfinite(tboxes).all()
    assert np.array_equal(tboxes[0], np.asarray(box, dtype=np.float64))
    same = 0
    for t in range(1, len(frames)):
        if hseen[:t] != dseen[:t]:
            break
        assert np.array_equal(hboxes[t], dboxes[t]), (t, hboxes[t], dboxes[t])
        same += 1
    print(f'free-running: {same} of {len(frames) - 1} frames with every triple so far equal to the host loop\'s; '
          f'a second device run repeats the boxes bit for bit: {np.array_equal(tboxes, dboxes)}')
