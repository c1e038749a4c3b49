"""SiamFC probe, a batch of sequences with the tracker state on the device (csrc/siamfc_track.hip: vfs_siamfc_batch_crops /
_upsample / _peak; SiamFCProbe.track_batch).  The yardsticks are the host functions of vfs_amd/siamfc.py (crop_and_resize,
SiamFCProbe._apply_peak), the single-sequence kernels (vfs_siamfc_upsample / _peak) and SiamFCProbe(device_loop=True).track();
every comparison is exact.  backend=emu (CPU) / gpu."""
import numpy as np
import pytest
import torch

import tests.test_siamfc_track as T
from vfs_amd import siamfc as SF
from vfs_amd._lib import VfsError

SCALE_FACTORS = T.SCALE_FACTORS
WI = T.WI
STATUS_STATE, STATUS_GEOMETRY, STATUS_ROWS = 1, 2, 4      # include/vfs_hip.h


def _pack(frames):
    """the frames back to back (256-byte aligned) in one uint8 buffer -> buffer, offsets"""
    offs, end = [], 0
    for f in frames:
        offs.append(end)
        end += (f.size + 255) // 256 * 256
    buf = np.full(end, 77, np.uint8)
    for o, f in zip(offs, frames):
        buf[o:o + f.size] = f.reshape(-1)
    return torch.from_numpy(buf), torch.tensor(offs, dtype=torch.int64)


def _slots(frames, centers, z_szs, x_szs, active):
    """state fp64 [N][8] and meta int32 [N][8] as track_batch uploads them (row 0, status 0)"""
    N = len(frames)
    state, meta = torch.zeros(N, 8, dtype=torch.float64), torch.zeros(N, 8, dtype=torch.int32)
    for n, f in enumerate(frames):
        state[n] = torch.tensor([centers[n][0], centers[n][1], 30.0, 40.0, z_szs[n], x_szs[n], 0.0, 0.0], dtype=torch.float64)
        fill = np.clip(np.rint(np.mean(f, axis=(0, 1))), 0, 255)
        meta[n] = torch.tensor([active[n], f.shape[0], f.shape[1], fill[0], fill[1], fill[2], 0, 0], dtype=torch.int32)
    return state, meta


def _batch_crops(backend, frames, state, meta, factors, out_size, use_z=0):
    buf, offs = _pack(frames)
    N, S = len(frames), len(factors)
    out = torch.full((S, N, 3, out_size, out_size), -1.0)
    backend.hostlib.siamfc_batch_crops(buf, offs, state, meta, torch.tensor(factors, dtype=torch.float64), out, N, S, out_size, use_z, None)
    return out.numpy()


def _host_crop(frame, center, size, out_size):
    return np.asarray(SF.crop_and_resize(frame, center, size, out_size, np.mean(frame, axis=(0, 1))), dtype=np.float32).transpose(2, 0, 1)


# ---------------------------------------------------------------------------------------------
# 1. crops
# ---------------------------------------------------------------------------------------------
CROP_FRAMES = [T._frame(96, 128, seed=1), T._frame(72, 80, seed=2), T._frame(120, 64, seed=3)]
CROP_CENTERS = [(np.float32(47.6), np.float32(66.3)), (np.float32(5.5), np.float32(4.25)), (np.float32(300.0), np.float32(-200.0))]
CROP_X_SZ = [float(np.float32(41.7)), 50.3 * 1.0148, float(np.float32(30.0))]      # float32 values (after init) and a float64 one (after a step)
CROP_Z_SZ = [float(np.float32(19.6)), 23.7, float(np.float32(14.1))]


@pytest.mark.parametrize('out_size', [63, 31])
def test_batch_crops_equal_host_bytes(backend, out_size):
    """vfs_siamfc_batch_crops, N = 3 slots with frames of three sizes, S = 3: out[s][n] == crop_and_resize(frame_n, center_n,
    x_sz_n * f_s, out_size, avg_n) in CHW, every byte - a box inside its frame, one across two borders (average-colour
    padding), one wholly outside (zeros).  With one slot inactive its crops are zeros, its state / meta bytes are unchanged and
    the other slots' crops are what they were.  One use_z launch (S = 1, size = z_sz)."""
    factors = [float(f) for f in SCALE_FACTORS]
    state, meta = _slots(CROP_FRAMES, CROP_CENTERS, CROP_Z_SZ, CROP_X_SZ, [1, 1, 1])
    state0, meta0 = state.clone(), meta.clone()
    got = _batch_crops(backend, CROP_FRAMES, state, meta, factors, out_size)
    kinds = set()
    for n, frame in enumerate(CROP_FRAMES):
        for s, f in enumerate(factors):
            want = _host_crop(frame, CROP_CENTERS[n], CROP_X_SZ[n] * f, out_size)
            assert np.array_equal(got[s, n], want), (n, s, int((got[s, n] != want).sum()))
            p = SF.crop_params(frame.shape, CROP_CENTERS[n], CROP_X_SZ[n] * f, out_size, np.mean(frame, axis=(0, 1)))
            kinds.add('zeros' if not p[0] else 'padded_twice' if p[7] > 0 and p[8] > 0 else 'inside' if p[5] == p[6] == out_size else 'other')
    assert {'zeros', 'padded_twice', 'inside'} <= kinds
    assert torch.equal(state, state0) and torch.equal(meta, meta0)      # no status bit, nothing else written

    state, meta = _slots(CROP_FRAMES, CROP_CENTERS, CROP_Z_SZ, CROP_X_SZ, [1, 0, 1])
    state[1, 6:] = torch.tensor([123.0, -7.0], dtype=torch.float64)
    state0, meta0 = state.clone(), meta.clone()
    part = _batch_crops(backend, CROP_FRAMES, state, meta, factors, out_size)
    assert not part[:, 1].any() and np.array_equal(part[:, 0], got[:, 0]) and np.array_equal(part[:, 2], got[:, 2])
    assert torch.equal(state, state0) and torch.equal(meta, meta0)

    state, meta = _slots(CROP_FRAMES, CROP_CENTERS, CROP_Z_SZ, CROP_X_SZ, [1, 1, 1])
    z = _batch_crops(backend, CROP_FRAMES, state, meta, [1.0], out_size, use_z=1)
    for n, frame in enumerate(CROP_FRAMES):
        assert np.array_equal(z[0, n], _host_crop(frame, CROP_CENTERS[n], CROP_Z_SZ[n], out_size)), n
    assert z[0, 0].any() and z[0, 1].any()


# ---------------------------------------------------------------------------------------------
# 2. up-sampling + peak + state
# ---------------------------------------------------------------------------------------------
def _host_probe(r, box, frame):
    """a host-loop SiamFCProbe (its state and _apply_peak are the yardstick; the backbone is never used for them)"""
    p = SF.SiamFCProbe(dict(extra_conv=False, response_sz=r), backbone=torch.nn.Identity(), device='cpu')
    p.init(frame, box)
    return p


def _probe_state(p):
    return [float(p.center[0]), float(p.center[1]), float(p.target_sz[0]), float(p.target_sz[1]), float(p.z_sz), float(p.x_sz)]


def _single_record(backend, resp, up_sz, hann):
    """vfs_siamfc_upsample + vfs_siamfc_peak on one slot's maps [S,r,r]"""
    S, r = resp.shape[0], resp.shape[-1]
    idx, w = SF._cubic_taps(r, up_sz)
    up = torch.zeros(S, up_sz, up_sz)
    keys = torch.full((S,), -1, dtype=torch.int64)
    backend.hostlib.siamfc_upsample(torch.from_numpy(resp), torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(w),
                                    torch.from_numpy(T.PENALTY), up, keys, S, r, up_sz, None)
    rec = torch.full((4,), -1, dtype=torch.int32)
    backend.hostlib.siamfc_peak(up, keys, torch.from_numpy(hann), rec, S, up_sz, float(np.float32(1 - WI)), float(WI), None)
    return rec.tolist(), up.numpy(), keys.numpy()


def _batch_step(backend, resp, up_sz, hann, state, meta, boxes, records):
    """one vfs_siamfc_batch_upsample + vfs_siamfc_batch_peak on resp [S][N][r][r]; state, meta, boxes, records in place"""
    S, N, r = resp.shape[0], resp.shape[1], resp.shape[-1]
    idx, w = SF._cubic_taps(r, up_sz)
    up = torch.zeros(S, N, up_sz, up_sz)
    keys = torch.full((N, S), -1, dtype=torch.int64)
    backend.hostlib.siamfc_batch_upsample(torch.from_numpy(resp), torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(w),
                                          torch.from_numpy(T.PENALTY), up, keys, N, S, r, up_sz, None)
    c = SF.DEFAULT_CFG
    backend.hostlib.siamfc_batch_peak(up, keys, torch.from_numpy(hann), torch.from_numpy(np.ascontiguousarray(SCALE_FACTORS)), state, meta,
                                      boxes, records, boxes.shape[0], N, S, up_sz, float(np.float32(1 - WI)), float(WI),
                                      float(c['total_stride']), float(c['response_up']), float(c['instance_sz']), float(c['scale_lr']), None)
    return up.numpy(), keys.numpy()


def _hann(up_sz):
    h = np.outer(np.hanning(up_sz), np.hanning(up_sz))
    return h / h.sum()


def _slot_responses(step, r):
    """three slots' maps [3][S,r,r]: random; the same map at scales 0 and 2 (both penalised: the lower index wins); constant
    maps (the maximum of a map repeats inside it)"""
    a = T._responses(60 + step, 1e-3, r)
    tie = T._responses(70 + step, 1e-3, r)
    tie[0, r // 3, r // 2] = 5e-3
    tie[2] = tie[0]
    tie[1] *= 0.5
    flat = np.stack([np.full((r, r), v, np.float32) for v in (0.2, 0.25, 0.2)])
    return [a, tie, flat]


@pytest.mark.parametrize('r,steps', [(17, 1), (5, 3)], ids=['r17_up272', 'r5_up80_three_steps'])
def test_batch_peak_and_state_equal_single_kernels_and_host(backend, r, steps):
    """N = 4 (three active slots, one inactive), S = 3.  Per step and slot: records[row] == the triple of vfs_siamfc_upsample +
    vfs_siamfc_peak on that slot's three maps alone (the up-sampled maps and maxima too); the state == a host SiamFCProbe's
    center, target_sz, z_sz, x_sz after _apply_peak(scale_id, (row, col)) from the same start, widened, with ==; boxes[row] ==
    the method's return value.  Three consecutive steps cover z_sz / x_sz turning from float32 into float64 and the row
    counter.  Ties across scales and inside a map go to the lowest index.  The inactive slot keeps every word."""
    up_sz = 16 * r
    hann = _hann(up_sz)
    frame = T._frame(96, 128, seed=4)
    start = [[31, 21, 40, 30], [50.5, 30.25, 21, 33], [11, 12, 57.5, 19.25]]
    probes = [_host_probe(r, b, frame) for b in start]
    assert all(isinstance(p.x_sz, np.float32) for p in probes)
    N, S, rows_cap = 4, 3, 4 * 8
    state, meta = torch.zeros(N, 8, dtype=torch.float64), torch.zeros(N, 8, dtype=torch.int32)
    order = [0, 1, 3]      # slot 2 is the inactive one
    for p, n in zip(probes, order):
        state[n, :6] = torch.tensor(_probe_state(p), dtype=torch.float64)
        meta[n] = torch.tensor([1, 96, 128, 1, 2, 3, 8 * n + 1, 0], dtype=torch.int32)
    state[2] = torch.arange(8, dtype=torch.float64) + 0.5
    meta[2] = torch.tensor([0, 96, 128, 9, 9, 9, 17, 0], dtype=torch.int32)
    boxes, records = torch.full((rows_cap, 4), -5.0, dtype=torch.float64), torch.full((rows_cap, 4), -5, dtype=torch.int32)
    for step in range(steps):
        maps = _slot_responses(step, r)
        resp = np.zeros((S, N, r, r), np.float32)
        for m, n in zip(maps, order):
            resp[:, n] = m
        resp[:, 2] = T._responses(99, 1.0, r)
        up, keys = _batch_step(backend, resp, up_sz, hann, state, meta, boxes, records)
        for p, m, n in zip(probes, maps, order):
            rec, sup, skeys = _single_record(backend, m, up_sz, hann)
            row = 8 * n + 1 + step
            assert records[row].tolist() == rec, (step, n)
            assert np.array_equal(up[:, n], sup) and np.array_equal(keys[n], skeys)
            box = p._apply_peak(rec[0], (rec[1], rec[2]))
            assert box.dtype == np.float32
            assert state[n, :6].tolist() == _probe_state(p), (step, n)
            assert boxes[row].tolist() == [float(v) for v in box], (step, n)
            assert meta[n].tolist() == [1, 96, 128, 1, 2, 3, row + 1, 0]
            if step == 0:
                assert isinstance(p.x_sz, np.float64) and isinstance(p.z_sz, np.float64)
        assert records[8 * order[1] + 1 + step, 0] == 0      # the same map at scales 0 and 2: the lower one
        assert records[8 * order[2] + 1 + step, 0] == 1
        flat_up = up[1, order[2]].reshape(-1)        # a flat map: its maximum repeats inside the map, the key names the first one
        val, idx = T._key_decode(torch.from_numpy(keys[order[2]]))
        assert (flat_up == flat_up.max()).sum() > 1 and val[1] == flat_up.max() and idx[1] == int(np.argmax(flat_up))
    assert state[2].tolist() == [i + 0.5 for i in range(8)] and meta[2].tolist() == [0, 96, 128, 9, 9, 9, 17, 0]
    written = sorted(8 * n + 1 + k for n in order for k in range(steps))
    rest = [i for i in range(rows_cap) if i not in written]
    assert (boxes[rest] == -5.0).all() and (records[rest] == -5).all()


def test_batch_peak_out_of_rows(backend):
    """row == rows_cap: nothing of that slot is written but its status bit, and the neighbours advance as if it were alone"""
    r, up_sz = 5, 80
    hann = _hann(up_sz)
    frame = T._frame(96, 128, seed=4)
    probes = [_host_probe(r, b, frame) for b in ([31, 21, 40, 30], [50.5, 30.25, 21, 33], [11, 12, 57.5, 19.25])]
    N, S, rows_cap = 3, 3, 6
    state, meta = torch.zeros(N, 8, dtype=torch.float64), torch.zeros(N, 8, dtype=torch.int32)
    for n, p in enumerate(probes):
        state[n, :6] = torch.tensor(_probe_state(p), dtype=torch.float64)
        meta[n] = torch.tensor([1, 96, 128, 1, 2, 3, (2, rows_cap, 5)[n], 0], dtype=torch.int32)
    state0 = state.clone()
    boxes, records = torch.full((rows_cap, 4), -5.0, dtype=torch.float64), torch.full((rows_cap, 4), -5, dtype=torch.int32)
    maps = _slot_responses(0, r)
    _batch_step(backend, np.stack(maps, 1), up_sz, hann, state, meta, boxes, records)
    assert torch.equal(state[1], state0[1]) and meta[1].tolist() == [1, 96, 128, 1, 2, 3, rows_cap, STATUS_ROWS]
    for n in (0, 2):
        rec, _, _ = _single_record(backend, maps[n], up_sz, hann)
        row = (2, rows_cap, 5)[n]
        box = probes[n]._apply_peak(rec[0], (rec[1], rec[2]))
        assert records[row].tolist() == rec and boxes[row].tolist() == [float(v) for v in box]
        assert state[n, :6].tolist() == _probe_state(probes[n]) and meta[n].tolist() == [1, 96, 128, 1, 2, 3, row + 1, 0]
    assert (records[[0, 1, 3, 4]] == -5).all() and (boxes[[0, 1, 3, 4]] == -5.0).all()


# ---------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------
def _valid_args(dev):
    """small valid argument lists of the three entry points (device tensors: an argument is refused before anything is read)"""
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)      # noqa: E731
    N, S, r, up, out = 2, 3, 5, 80, 31
    crops = dict(frames=z(4096, dtype=torch.uint8), frame_off=z(N + 1, dtype=torch.int64), state=z(N + 1, 8, dtype=torch.float64),
                 meta=z(N + 1, 8, dtype=torch.int32), factors=z(S + 1, dtype=torch.float64), out=z(S, N, 3, out, out), N=N, S=S, out_size=out,
                 use_z=0, stream=None)
    upsample = dict(responses=z(S, N, r, r), tap_idx=z(up + 1, 4, dtype=torch.int32), tap_w=z(up + 1, 4), penalty=z(S), up_out=z(S, N, up, up),
                    scale_max=z(N * S + 1, dtype=torch.int64), N=N, S=S, r=r, up=up, stream=None)
    peak = dict(up_in=z(S, N, up, up), scale_max=z(N * S + 1, dtype=torch.int64), hann=z(up * up + 1, dtype=torch.float64),
                factors=z(S + 1, dtype=torch.float64), state=z(N + 1, 8, dtype=torch.float64), meta=z(N + 1, 8, dtype=torch.int32),
                boxes=z(9, 4, dtype=torch.float64), records=z(9, 4, dtype=torch.int32), rows_cap=8, N=N, S=S, up=up, one_minus_wi=0.8,
                window_influence=0.2, total_stride=8.0, response_up=16.0, instance_sz=255.0, scale_lr=0.59, stream=None)
    return dict(siamfc_batch_crops=crops, siamfc_batch_upsample=upsample, siamfc_batch_peak=peak)


def _shift(nbytes):
    """the same buffer, its address moved by nbytes (misaligned)"""
    return lambda t: t.reshape(-1).view(torch.uint8)[nbytes:]


REFUSALS = [(e, k, None) for e, ks in (('siamfc_batch_crops', ('frames', 'frame_off', 'state', 'meta', 'factors', 'out')),
                                       ('siamfc_batch_upsample', ('responses', 'tap_idx', 'tap_w', 'penalty', 'up_out', 'scale_max')),
                                       ('siamfc_batch_peak', ('up_in', 'scale_max', 'hann', 'factors', 'state', 'meta', 'boxes', 'records')))
            for k in ks]
REFUSALS += [('siamfc_batch_crops', k, _shift(4)) for k in ('frame_off', 'state', 'factors')] + [('siamfc_batch_crops', 'meta', _shift(2))]
REFUSALS += [('siamfc_batch_upsample', k, _shift(8)) for k in ('tap_idx', 'tap_w')] + [('siamfc_batch_upsample', 'scale_max', _shift(4))]
REFUSALS += [('siamfc_batch_peak', k, _shift(4)) for k in ('scale_max', 'hann', 'factors', 'state', 'boxes')]
REFUSALS += [('siamfc_batch_peak', 'meta', _shift(2)), ('siamfc_batch_peak', 'records', _shift(8))]
for _e in ('siamfc_batch_crops', 'siamfc_batch_upsample', 'siamfc_batch_peak'):
    REFUSALS += [(_e, 'N', 0), (_e, 'N', 65), (_e, 'S', 0), (_e, 'S', 9)]
REFUSALS += [('siamfc_batch_crops', 'out_size', 0), ('siamfc_batch_crops', 'out_size', 4097), ('siamfc_batch_crops', 'use_z', 2),
             ('siamfc_batch_crops', 'use_z', 1),      # with S = 3
             ('siamfc_batch_upsample', 'r', 0), ('siamfc_batch_upsample', 'r', 33), ('siamfc_batch_upsample', 'r', 70000),
             ('siamfc_batch_upsample', 'up', 0), ('siamfc_batch_upsample', 'up', 4097),
             ('siamfc_batch_peak', 'up', 0), ('siamfc_batch_peak', 'up', 4097), ('siamfc_batch_peak', 'rows_cap', 0),
             ('siamfc_batch_peak', 'rows_cap', 2 ** 31)]


def _refusal_id(case):
    e, k, v = case
    return f'{e[13:]}-{k}-' + ('null' if v is None else 'misaligned' if callable(v) else str(v))


@pytest.mark.parametrize('case', REFUSALS, ids=_refusal_id)
def test_batch_refusals(backend, case):
    """every argument check of the three entry points: VfsError, before any launch (the outputs keep their bytes); the valid
    argument list the case is derived from is accepted"""
    entry, key, val = case
    args = _valid_args(backend.dev)[entry]
    outs = [t for k, t in args.items() if k in ('out', 'up_out', 'state', 'meta', 'boxes', 'records')]
    for t in outs:
        t.fill_(3)
    bad = dict(args)
    bad[key] = val(args[key]) if callable(val) else val
    with pytest.raises(VfsError):
        getattr(backend.lib, entry)(*bad.values())
    if backend.dev.type == 'cuda':
        torch.cuda.synchronize()
    assert all(bool((t == 3).all()) for t in outs)


def test_batch_valid_arguments_accepted(backend):
    """the argument lists the refusals start from do launch (all slots inactive: zeros out, nothing else written)"""
    for entry, args in _valid_args(backend.dev).items():
        getattr(backend.lib, entry)(*args.values())
    if backend.dev.type == 'cuda':
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# 4. poisoned state (emulator only: a GPU is no place to find out that a guard is missing)
# ---------------------------------------------------------------------------------------------
def test_batch_crops_poisoned_state(emu_backend):
    """a slot whose state holds NaN and one with x_sz = 1e300 (and an infinite centre): zero crops and the status bit, never an
    address; the healthy neighbours' crops are what they are without the poison"""
    frames = [T._frame(48, 64, seed=s) for s in (5, 6, 7, 8)]
    centers = [(np.float32(20.0), np.float32(30.0))] * 4
    factors = [float(f) for f in SCALE_FACTORS]
    state, meta = _slots(frames, centers, [10.0] * 4, [24.0] * 4, [1, 1, 1, 1])
    clean = _batch_crops(emu_backend, frames, state.clone(), meta.clone(), factors, 31)
    assert clean[:, 2].any()
    state[0, 1] = float('nan')
    state[1, 5] = 1e300
    state[3, 0] = float('inf')
    got = _batch_crops(emu_backend, frames, state, meta, factors, 31)
    assert not got[:, 0].any() and not got[:, 1].any() and not got[:, 3].any()
    assert np.array_equal(got[:, 2], clean[:, 2])
    for s, f in enumerate(factors):
        assert np.array_equal(got[s, 2], _host_crop(frames[2], centers[2], 24.0 * f, 31))
    assert meta[:, 7].tolist() == [STATUS_STATE, STATUS_STATE, 0, STATUS_STATE]
    state, meta = _slots(frames, centers, [float('nan')] * 4, [24.0] * 4, [1, 1, 1, 1])      # use_z reads z_sz
    z = _batch_crops(emu_backend, frames, state, meta, [1.0], 31, use_z=1)
    assert not z.any() and meta[:, 7].tolist() == [STATUS_STATE] * 4
    state, meta = _slots(frames, centers, [10.0] * 4, [24.0] * 4, [1, 1, 1, 1])
    meta[1, 1] = 0                   # a frame without rows
    meta[2, 2] = 1 << 20             # a width that no frame has
    got = _batch_crops(emu_backend, frames, state, meta, factors, 31)
    assert not got[:, 1].any() and not got[:, 2].any() and np.array_equal(got[:, 0], clean[:, 0])
    assert meta[:, 7].tolist() == [0, STATUS_STATE, STATUS_STATE, 0]


# ---------------------------------------------------------------------------------------------
# 5. the loop
# ---------------------------------------------------------------------------------------------
def _sequences():
    """three sequences in the style of test_siamfc_track._sequence: lengths 4, 6, 7, two frame sizes"""
    a, box_a = T._sequence(7)
    small = [np.ascontiguousarray(f[40:232, 60:316]) for f in T._sequence(6)[0]]      # 192 x 256: the same scene, cut
    return [a[:4], small, a], [box_a, [box_a[0] - 60, box_a[1] - 40, 40, 40], box_a]


def test_track_batch_against_device_loop(backend, monkeypatch):
    """SiamFCProbe.track_batch on a ResNet-18 probe: three sequences of 4, 6 and 7 frames in two frame sizes, batch=2 (one slot
    is refilled).

    per-image bits: features() and the head give a search crop the same bits in the batched pass (6 maps, 2 exemplars) as in
        the single-sequence pass (3 maps, 1 exemplar) - asserted on one frame's crops
    boxes: track_batch == SiamFCProbe(device_loop=True).track() for each sequence, every box, with ==; frame 0 is the input
        box, everything finite float64
    no per-frame read-back: the calls of Tensor.item / .tolist / .cpu / .numpy and torch.cuda.synchronize during track_batch
        are as many with every sequence twice as long
    buffers: the per-call buffers keep their addresses over the frame steps"""
    if backend.name == 'emu':
        pytest.skip('full ResNet-18 at 120 / 255 pixel crops: minutes on the emulator; runs on the GPU')
    seqs, boxes = _sequences()
    assert [len(q) for q in seqs] == [4, 6, 7] and len({q[0].shape for q in seqs}) == 2
    _, probe = T._probes(backend.dev)
    lib = backend.eng.lib
    inner = lib.siamfc_batch_peak
    ptrs = []

    def spy(*args):
        ptrs.append({k: v.data_ptr() for k, v in probe._bl.items() if isinstance(v, torch.Tensor) and k != 'responses'})
        return inner(*args)
    monkeypatch.setitem(lib.__dict__, 'siamfc_batch_peak', spy)
    got = probe.track_batch(seqs, boxes, batch=2)
    monkeypatch.setitem(lib.__dict__, 'siamfc_batch_peak', inner)
    assert len(ptrs) == 3 + 6 and all(p == ptrs[0] for p in ptrs)      # slot 0: 3 steps, then the 7-frame sequence's 6; slot 1: 5

    x = probe._bl['x'].clone()      # the last step's crops [S * 2]: slot 0 holds the 7-frame sequence, slot 1 is inactive (zeros)
    bank = probe._bl['bank'].clone()
    assert x.view(3, 2, -1)[:, 0].any()
    f6, f3 = probe.features(x), probe.features(x.view(3, 2, *x.shape[1:])[:, 0].contiguous())
    assert torch.equal(f6.view(3, 2, *f6.shape[1:])[:, 0], f3), 'features(): an image\'s bits depend on the batch it is in (6 vs 3)'
    r6, r3 = probe.head(bank, f6), probe.head(bank[0:1].contiguous(), f3)
    assert torch.equal(r6.view(3, 2, *r6.shape[1:])[:, 0], r3), 'head (1x1 conv + vfs_xcorr_fwd): bits depend on the batch (6 vs 3 maps)'

    for i, (q, box) in enumerate(zip(seqs, boxes)):
        _, single = T._probes(backend.dev)
        want = single.track(q, box)
        assert got[i].shape == (len(q), 4) and got[i].dtype == np.float64 and np.isfinite(got[i]).all()
        assert np.array_equal(got[i][0], np.asarray(box, dtype=np.float64))
        assert np.array_equal(got[i], want), (i, np.abs(got[i] - want).max())
        assert probe.last_batch_records[i].shape == (len(q) - 1, 3)

    counts = {}

    def counted(owner, name):
        fn = getattr(owner, name)

        def wrapper(*a, **k):
            counts[name] = counts.get(name, 0) + 1
            return fn(*a, **k)
        monkeypatch.setattr(owner, name, wrapper)
    for name in ('item', 'tolist', 'cpu', 'numpy'):
        counted(torch.Tensor, name)
    counted(torch.cuda, 'synchronize')
    probe.track_batch(seqs, boxes, batch=2)
    once = dict(counts)
    counts.clear()
    twice = probe.track_batch([list(q) + list(q) for q in seqs], boxes, batch=2)
    assert counts == once, (once, counts)
    monkeypatch.undo()
    assert [len(t) for t in twice] == [8, 12, 14]
    for t, g, q in zip(twice, got, seqs):
        assert np.array_equal(t[:len(q)], g)      # the first half is the same run
