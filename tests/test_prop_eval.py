"""JHMDB pose (PCK) and VIP parts (mIoU) evaluation: the numpy oracle (tests/prop_eval_oracle.py) against numbers recorded
from the reference's own functions (tests/golden/prop_eval.npz), the three HIP kernels of csrc/propeval.hip through the C ABI
bit for bit against the oracle (emulator and GPU), the host evaluators against oracle and golden, and both paths end to end
through VanillaTracker.forward_test.

Coordinates are compared bit for bit with the REFERENCE only on maps whose topk + 1 largest values are distinct (np.argsort
leaves ties open; the golden generator asserts it, share of maps left out: 0).  On the reference's symmetric Gaussian the
selected set is unambiguous and only the float64 summation order is open: five products below 2^11 summed in any order differ
by less than 5 * 2^-53 * 2^11 ~ 1e-12, compared at 1e-9 pixels.  Kernel against oracle is bit for bit everywhere, ties
included: both follow the stated rule (larger value first, then the lower flat index)."""
import contextlib
import os

import numpy as np
import pytest
import torch

from oracle import vfs_oracle as VO
from tests import prop_eval_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, 'tests', 'golden')
TOPK = 5


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(G, 'prop_eval.npz'))


@contextlib.contextmanager
def use_lib(backend):
    """vfs_amd.prop_eval binds the library through vfs_amd._lib.get_lib(): point it at the backend's for the test"""
    from vfs_amd._lib import get_lib, set_lib
    try:
        prev = get_lib()
    except Exception:
        prev = None
    set_lib(backend.lib)
    try:
        yield
    finally:
        set_lib(prev)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def coord_maps(golden, i):
    seed, T, K, H, W = (int(v) for v in golden['coord/cases'][i])
    return O.seeded_maps(seed, T, K, H, W, [tuple(z) for z in golden[f'coord/{i}/zero']], [tuple(z) for z in golden[f'coord/{i}/sparse']])


def pck_inputs(golden):
    results, gts = [], []
    for i, (seed, T, H, W, T_gt) in enumerate(golden['pck/cases']):
        results.append(O.seeded_maps(int(seed), int(T), 15, int(H), int(W), [tuple(z) for z in golden[f'pck/{i}/zero']]))
        gts.append(golden[f'pck/{i}/gt'])
        assert gts[-1].shape == (2, 15, int(T_gt))
    return results, gts


def label_inputs(golden):
    pairs = [O.seeded_labels(int(seed), int(T), int(H), int(W)) for seed, T, H, W in golden['label/cases']]
    return [p for p, _ in pairs], [g for _, g in pairs]


# ---- 1. oracle == golden (the reference's own functions) ----------------------------------------------------------------
def test_oracle_heatmaps_equal_reference(golden):
    xy = golden['pose/xy']
    for i, (H, W, sigma) in enumerate(golden['pose/cases']):
        got = O.pose_heatmaps(xy, int(sigma), int(H), int(W))
        assert same_bits(got, golden[f'pose/{i}/map']), (i, H, W, sigma)
    # the cases cover: an untouched map (fully outside), a clipped patch, a whole patch
    m = golden['pose/0/map']
    nz = (m.reshape(len(m), -1) != 0).sum(1)
    assert (nz == 0).any() and (nz == 13 * 13).any() and ((nz > 0) & (nz < 13 * 13)).any()


def test_oracle_coordinates_equal_reference(golden):
    for i in range(len(golden['coord/cases'])):
        maps = coord_maps(golden, i)
        assert same_bits(O.heatmap_coords(maps, TOPK), golden[f'coord/{i}/coords']), i
        assert (golden[f'coord/{i}/coords'] == -1).any()         # the all-zero maps
    sym = O.pose_heatmaps(golden['coord/sym/xy'], 2, 24, 32)[None]
    got, want = O.heatmap_coords(sym, TOPK), golden['coord/sym/coords']
    assert np.abs(got - want).max() <= 1e-9
    # ... and the peak is where it was drawn: five fp32 weights (relative error 2^-24 each) times coordinates below 32
    assert np.abs(got[:, :, 0] - golden['coord/sym/xy']).max() <= 5 * 32 * 2.0**-24


def test_oracle_miou_equals_reference(golden):
    preds, gts = label_inputs(golden)
    frames = [(p, g) for P, Gt in zip(preds, gts) for p, g in zip(P, Gt)]
    total = np.zeros((20, 3), np.int64)
    for f, (p, g) in enumerate(frames):
        c = O.label_counts(p, g, 20, 255)
        want = golden['label/per_frame'][f]                          # intersect, union, pred, label
        assert np.array_equal(c[:, 0], want[0]) and np.array_equal(c[:, 1], want[2]) and np.array_equal(c[:, 2], want[3])
        assert np.array_equal(c[:, 1] + c[:, 2] - c[:, 0], want[1])
        total += c
    t = golden['label/total']
    assert np.array_equal(total[:, 0], t[0]) and np.array_equal(total[:, 1], t[2]) and np.array_equal(total[:, 2], t[3])
    all_acc, acc, iou = O.metrics_from_counts(total)
    assert all_acc == golden['label/all_acc']
    assert same_bits(acc, golden['label/acc']) and same_bits(iou, golden['label/iou'])
    assert np.isnan(iou[7]) and np.isnan(acc[7])                     # class 7 occurs in neither map: NaN, skipped by nanmean
    summary, per_class, counts = O.vip_evaluate(preds, gts)
    assert list(golden['label/summary_keys']) == ['mIoU', 'mAcc', 'aAcc']
    for k, v in zip(golden['label/summary_keys'], golden['label/summary_values']):
        assert summary[str(k)] == v, (k, summary[str(k)], v)
    # np.histogram's closed last bin: a 2 x 2 map of 20s against itself counts in class 19
    tiny = np.full((2, 2), 20, np.uint8)
    c = O.label_counts(tiny, tiny, 20, 255)
    want = golden['label/closed_bin']
    assert c[19].tolist() == [4, 4, 4] and c.sum() == 12
    assert np.array_equal(c[:, 0], want[0]) and np.array_equal(c[:, 1], want[2]) and np.array_equal(c[:, 2], want[3])


def test_oracle_pck_equals_reference(golden):
    results, gts = pck_inputs(golden)
    got = O.pck_evaluate(results, gts, TOPK)
    assert list(got) == [str(k) for k in golden['pck/keys']] == [f'PCK@{a}' for a in O.PCK_RANGES]
    for k, v in zip(golden['pck/keys'], golden['pck/values']):
        assert got[str(k)] == v, (k, got[str(k)], v)
    d = np.split(golden['pck/compute_in'], np.cumsum(golden['pck/compute_split'])[:-1])
    for a, want in zip(O.PCK_RANGES, golden['pck/compute_out']):
        assert np.array_equal(O.compute_pck(d, a), want)
    with pytest.raises(ZeroDivisionError):
        O.compute_pck([np.zeros((0, 0))], 0.1)


# ---- 2. kernels == oracle, bit for bit ----------------------------------------------------------------------------------
def run_topk(backend, maps, topk, offset=0):
    """maps [N][HW] numpy; `offset` floats of padding in front so that map 0 starts off a 16-byte boundary"""
    from vfs_amd import prop_eval as PE
    N, HW = maps.shape
    buf = torch.zeros(N * HW + 4, dtype=torch.float32)
    buf[offset:offset + N * HW] = torch.from_numpy(maps.reshape(-1))
    dev = buf.to(backend.dev)[offset:offset + N * HW].view(N, 1, HW)
    with use_lib(backend):
        return PE.heatmap_topk(dev, topk, backend.dev)


def check_topk(backend, maps, topk, offset=0):
    vals, idx, minv, flags = run_topk(backend, maps, topk, offset)
    wv, wi, wm, wf = O.heatmap_topk(maps, topk)
    assert np.array_equal(idx, wi), (idx, wi)
    assert same_bits(vals, wv) and np.array_equal(minv, wm) and np.array_equal(flags, wf)


# one workgroup covers 1024 elements per step (256 lanes x 16 bytes), four steps per unrolled iteration
TOPK_SIZES = [(3, 5), (2, 8), (3, 1000), (2, 1024), (3, 1025), (3, 24 * 32), (3, 37 * 53), (2, 4096), (3, 4099), (2, 9001)]


@pytest.mark.parametrize('N,HW,topk', [(n, hw, k) for n, hw in TOPK_SIZES for k in (1, 5, 8) if hw >= k])
def test_topk_kernel_bit_exact(backend, N, HW, topk):
    rng = np.random.RandomState(HW * 10 + topk)
    maps = rng.rand(N, HW).astype(np.float32)
    maps[N - 1] = np.floor(maps[N - 1] * 16) / 16          # a map of 17 distinct values: ties everywhere
    for offset in (0, 1, 3):                               # odd HW moves the later maps off the boundary as well
        check_topk(backend, maps, topk, offset)


def test_topk_tie_rule_zero_and_single_maps(backend):
    HW = 2500
    maps = np.zeros((6, HW), np.float32)
    base = np.random.RandomState(1).rand(HW).astype(np.float32) * 0.5
    # ties inside the top 5: the same largest value at three places, in different lanes and waves
    maps[0] = base
    maps[0, [2400, 7, 1030]] = 0.9
    # ties across the boundary: 4 distinct leaders, then the 5th value at four places - the LOWEST index is taken
    maps[1] = base
    maps[1, [10, 20, 30, 40]] = [0.95, 0.94, 0.93, 0.92]
    maps[1, [2222, 1500, 333, 1501]] = 0.8
    # all zero; one non-zero pixel; negative zeros count as zero; one negative value (minimum)
    maps[3, 1234] = 0.25
    maps[4, ::2] = -0.0
    maps[5] = base
    maps[5, 77] = -3.0
    for topk in (1, 5, 8):
        for offset in (0, 2):
            check_topk(backend, maps, topk, offset)
    vals, idx, minv, flags = run_topk(backend, maps, 5)
    assert set(idx[0, 2:]) == {7, 1030, 2400} and idx[0, 2:].tolist() == [2400, 1030, 7]      # ascending rank: the lowest index last
    assert idx[1].tolist() == [333, 40, 30, 20, 10]
    assert idx[2].tolist() == [4, 3, 2, 1, 0] and flags.tolist() == [0, 0, 1, 0, 1, 0]
    assert idx[3, 4] == 1234 and idx[3, :4].tolist() == [3, 2, 1, 0]
    assert minv[5] == -3.0 and minv[2] == 0.0


def test_topk_nan_flag_and_shape_errors(backend):
    from vfs_amd._lib import VfsError
    from vfs_amd import prop_eval as PE
    maps = np.random.RandomState(2).rand(3, 1100).astype(np.float32)
    maps[1, 1000] = np.nan
    vals, idx, minv, flags = run_topk(backend, maps, 5)
    wv, wi, wm, wf = O.heatmap_topk(maps, 5)
    assert flags.tolist() == wf.tolist() == [0, O.TOPK_NAN, 0]                  # bad data, not a bad call
    assert np.array_equal(idx[[0, 2]], wi[[0, 2]]) and same_bits(vals[[0, 2]], wv[[0, 2]])
    # -inf never ranks (the empty slots of a lane's list hold -inf): flagged like a NaN, the other maps untouched
    inf_maps = maps.copy()
    inf_maps[1] = -np.inf
    inf_maps[1, :3] = [0.5, 0.25, 0.125]
    inf_maps[2, 17] = -np.inf
    vals, idx, minv, flags = run_topk(backend, inf_maps, 5)
    wv, wi, wm, wf = O.heatmap_topk(inf_maps, 5)
    assert flags.tolist() == wf.tolist() == [0, O.TOPK_NEG_INF, O.TOPK_NEG_INF]
    assert np.array_equal(idx[0], wi[0]) and same_bits(vals[0], wv[0]) and minv[1] == -np.inf and minv[2] == -np.inf
    both = inf_maps.copy()
    both[2, 18] = np.nan
    assert run_topk(backend, both, 5)[3].tolist() == O.heatmap_topk(both, 5)[3].tolist() == [0, 4, 6]
    dev = backend.dev
    with use_lib(backend):
        with pytest.raises(ValueError, match='infinity'):
            PE.heatmap_coords(torch.from_numpy(inf_maps.reshape(3, 1, 25, 44)).to(dev), 5, dev)
    t = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)       # noqa: E731
    args = lambda N, H, W, k: (t(N, H * W), t(N, 8), t(N, 8, dt=torch.int32), t(N), t(N, dt=torch.int32), N, H, W, k, None)   # noqa: E731
    with pytest.raises(VfsError, match='topk'):
        backend.lib.heatmap_topk(*args(2, 1, 4, 5))                              # H*W < topk
    for k in (0, 9):
        with pytest.raises(VfsError, match='topk 1..8'):
            backend.lib.heatmap_topk(*args(2, 4, 4, k))
    with pytest.raises(VfsError, match='null'):
        backend.lib.heatmap_topk(None, t(1, 8), t(1, 8, dt=torch.int32), t(1), t(1, dt=torch.int32), 1, 4, 4, 5, None)
    with use_lib(backend):
        with pytest.raises(ValueError, match='NaN'):
            PE.heatmap_coords(torch.from_numpy(maps.reshape(3, 1, 25, 44)).to(dev), 5, dev)
        neg = maps.copy()
        neg[1, 1000] = -1.0
        with pytest.raises(ValueError, match='negative'):
            PE.heatmap_coords(torch.from_numpy(neg.reshape(3, 1, 25, 44)).to(dev), 5, dev)
        with pytest.raises(NotImplementedError, match='1..8'):
            PE.heatmap_coords(neg.reshape(3, 1, 25, 44), 9, dev)
        with pytest.raises(ValueError, match='fewer'):
            PE.heatmap_coords(neg.reshape(3, 275, 2, 2), 5, dev)


@pytest.mark.parametrize('n', [1, 15, 16, 17, 4097, 24 * 32 * 3, 37 * 53 * 2 + 1])
def test_label_counts_kernel_bit_exact(backend, n):
    from vfs_amd import prop_eval as PE
    pred, gt = O.seeded_labels(n, 2, 37, 64)
    pred, gt = pred.reshape(-1)[:n], gt.reshape(-1)[:n]
    dev = backend.dev
    with use_lib(backend):
        c = PE.label_counts(pred, gt, 20, 255, device=dev)
        assert c.dtype == torch.int64 and np.array_equal(c.cpu().numpy(), O.label_counts(pred, gt, 20, 255))
        # accumulation onto the buffer; maps that start off a 16-byte boundary; no ignore index; fewer classes than labels
        want = O.label_counts(pred, gt, 20, 255) + O.label_counts(pred[1:], gt[1:], 20, None)
        tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        c2 = PE.label_counts(tp[1:], tg[1:], 20, None, out=c)
        assert c2 is c and np.array_equal(c.cpu().numpy(), want)
        for nc, ign in [(1, 0), (7, 3), (256, 255), (255, None)]:
            got = PE.label_counts(tp, tg, nc, ign, device=dev).cpu().numpy()
            assert np.array_equal(got, O.label_counts(pred, gt, nc, ign)), (nc, ign)


def test_label_counts_closed_last_bin_and_errors(backend):
    from vfs_amd._lib import VfsError
    from vfs_amd import prop_eval as PE
    dev = backend.dev
    tiny = np.full((2, 2), 20, np.uint8)
    with use_lib(backend):
        c = PE.label_counts(tiny, tiny, 20, 255, device=dev).cpu().numpy()
        assert c[19].tolist() == [4, 4, 4] and c.sum() == 12
        with pytest.raises(NotImplementedError, match='256'):
            PE.label_counts(tiny, tiny, 257, 255, device=dev)
        with pytest.raises(ValueError, match='shape'):
            PE.label_counts(tiny, tiny[:1], 20, 255, device=dev)
    z = torch.zeros(16, dtype=torch.uint8, device=dev)
    out = torch.zeros(20, 3, dtype=torch.int64, device=dev)
    with pytest.raises(VfsError, match='classes'):
        backend.lib.label_counts(z, z, out, 16, 0, 255, None)
    with pytest.raises(VfsError, match='ignore_index'):
        backend.lib.label_counts(z, z, out, 16, 20, 256, None)
    with pytest.raises(VfsError, match='null'):
        backend.lib.label_counts(z, None, out, 16, 20, 255, None)


def test_pose_heatmaps_kernel_equals_oracle_and_reference(backend, golden):
    from vfs_amd import prop_eval as PE
    xy = golden['pose/xy']
    with use_lib(backend):
        for i, (H, W, sigma) in enumerate(golden['pose/cases']):
            out = PE.pose_heatmaps(xy, int(sigma), int(H), int(W), backend.dev)
            assert out.shape == (1, xy.shape[1], H, W) and out.dtype == torch.float32
            got = out[0].cpu().numpy()
            assert same_bits(got, O.pose_heatmaps(xy, int(sigma), int(H), int(W)))
            assert same_bits(got, golden[f'pose/{i}/map'])
        with pytest.raises(ValueError, match='sigma'):
            PE.pose_heatmaps(xy, 0.7, 24, 32, backend.dev)
        with pytest.raises(ValueError, match='pose_coord'):
            PE.pose_heatmaps(xy.T, 2, 24, 32, backend.dev)


# ---- 3. evaluators == oracle evaluators == golden dicts -----------------------------------------------------------------
def test_heatmap_coords_equals_oracle_and_reference(backend, golden):
    from vfs_amd import prop_eval as PE
    with use_lib(backend):
        for i in range(len(golden['coord/cases'])):
            maps = coord_maps(golden, i)
            got = PE.heatmap_coords(torch.from_numpy(maps).to(backend.dev), TOPK, backend.dev)
            assert got.dtype == np.float64 and same_bits(got, O.heatmap_coords(maps, TOPK))
            assert same_bits(got, golden[f'coord/{i}/coords'])
        sym = O.pose_heatmaps(golden['coord/sym/xy'], 2, 24, 32)[None]
        got = PE.heatmap_coords(sym, TOPK, backend.dev)
        assert same_bits(got, O.heatmap_coords(sym, TOPK))
        assert np.abs(got - golden['coord/sym/coords']).max() <= 1e-9


def test_jhmdb_evaluator_matches_oracle_and_reference(backend, golden, tmp_path):
    import vfs_amd
    results, gts = pck_inputs(golden)
    want = O.pck_evaluate(results, gts, TOPK)
    with use_lib(backend):
        ev = vfs_amd.JHMDBEvaluator(gts, device=backend.dev)
        got = ev.evaluate(results, metrics='pck')
        with pytest.raises(KeyError):
            ev.evaluate(results, metrics='pkc')
        feat = ev.evaluate([[r, r] for r in results], metrics=['pck'])
        # results as save_np paths and as device tensors
        paths = []
        for i, r in enumerate(results):
            paths.append(str(tmp_path / f'{i}.npy'))
            np.save(paths[-1], r)
        got_paths = ev.evaluate(paths)
        got_dev = ev.evaluate([torch.from_numpy(r).to(backend.dev) for r in results])
        # a key point that is never visible: ZeroDivisionError, as the reference
        dead = [r.copy() for r in results]
        for r in dead:
            r[:, 3] = 0
        with pytest.raises(ZeroDivisionError):
            ev.evaluate(dead)
    assert list(got) == [f'PCK@{a}' for a in O.PCK_RANGES]
    for k, v in zip(golden['pck/keys'], golden['pck/values']):
        k = str(k)
        assert abs(got[k] - want[k]) < 1e-12 and abs(got[k] - v) < 1e-12, (k, got[k], want[k], v)
        assert got_paths[k] == got[k] and got_dev[k] == got[k]
    assert list(feat) == [str(k) for k in golden['pck/feat_keys']]
    for k, v in zip(golden['pck/feat_keys'], golden['pck/feat_values']):
        assert abs(feat[str(k)] - v) < 1e-12
    assert 0 < got['PCK@0.1'] < got['PCK@0.5'] < 100


def test_vip_evaluator_matches_oracle_and_reference(backend, golden, tmp_path):
    import vfs_amd
    from vfs_amd import davis_eval as DE
    preds, gts = label_inputs(golden)
    want, want_cls, want_counts = O.vip_evaluate(preds, gts)
    with use_lib(backend):
        ev = vfs_amd.VIPEvaluator(gts, device=backend.dev)
        got = ev.evaluate(preds, metrics='mIoU', output_dir=str(tmp_path))
        assert np.array_equal(ev.counts, want_counts)
        for k in ('IoU', 'Acc'):
            assert np.array_equal(ev.per_class[k], want_cls[k], equal_nan=True)
        with pytest.raises(KeyError):
            ev.evaluate(preds, metrics='mDice')
        feat = ev.evaluate([np.stack([p, g]) for p, g in zip(preds, gts)])          # [num_feats][T][H][W] per video
        dev_res = ev.evaluate([torch.from_numpy(p).to(backend.dev) for p in preds])
        feat_dev = ev.evaluate([torch.from_numpy(np.stack([p, g])).to(backend.dev) for p, g in zip(preds, gts)])     # 4-D tensors
        assert feat_dev == feat
        with pytest.raises(NotImplementedError, match='256'):
            vfs_amd.VIPEvaluator(gts, num_classes=300)
    assert list(got) == ['mIoU', 'mAcc', 'aAcc']
    for k, v in zip(golden['label/summary_keys'], golden['label/summary_values']):
        k = str(k)
        assert abs(got[k] - want[k]) < 1e-12 and abs(got[k] - v) < 1e-12, (k, got[k], want[k], v)
        assert dev_res[k] == got[k]
    assert list(feat) == [f'feat_{i}.{k}' for i in (0, 1) for k in ('mIoU', 'mAcc', 'aAcc')]
    assert feat['feat_0.mIoU'] == got['mIoU'] and feat['feat_1.mIoU'] == 1.0 and feat['feat_1.aAcc'] == 1.0
    back = DE.load_palette_pngs(os.path.join(str(tmp_path), ev.names[1]))              # the palette PNGs of the predictions
    assert np.array_equal(back, preds[1])


# ---- 4. end to end through forward_test ---------------------------------------------------------------------------------
def _model(dev, depth=18, **over):
    import vfs_amd
    cfg = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', f'vfs_r{depth}.py'))
    tc = vfs_amd.ConfigDict(cfg.test_cfg)
    tc['neighbor_range'], tc['precede_frames'] = 8, 3
    tc.update(over)
    bb = dict(cfg.model['backbone'])
    bb['out_indices'], bb['strides'] = tc['out_indices'], tc['strides']
    model = vfs_amd.build_model(dict(type='VanillaTracker', backbone=bb), train_cfg=None, test_cfg=tc)
    ref = VO.VanillaTracker(depth, dict(tc))
    VO.fill_state_dict_(ref, seed=5)
    ref.eval()
    missing = model.load_state_dict(ref.state_dict(), strict=False)
    assert not [k for k in missing.missing_keys if 'iteration' not in k]
    return model.to(dev).eval()


def _small_clip(T=3):
    """a 48 x 64 crop of a seeded clip (6 x 8 feature map): runs on the CPU emulator as well"""
    imgs = VO.fill_tensor([1, 1, 3, 6, 96, 128], 41, scale=2.0)
    return imgs[:, :, :, :T, 16:64, 24:88].contiguous(), (48, 64)


def test_end_to_end_pose_propagation_pck(backend):
    import vfs_amd
    model = _model(backend.dev)
    imgs, (H, W) = _small_clip(3)
    rng = np.random.RandomState(9)
    pose = np.stack([rng.uniform(4, W - 4, 15), rng.uniform(4, H - 4, 15)])
    pose[:, 5] = [W + 40, H + 40]                                       # one key point outside the frame: never visible ...
    gt = np.stack([pose + rng.normal(0, 1.5, pose.shape) * t for t in range(4)], axis=-1)      # [2][15][4]: longer than the clip
    with use_lib(backend):
        hm = vfs_amd.pose_heatmaps(pose, 2, H, W, backend.dev)
        assert hm.shape == (1, 15, H, W)
        out = model(imgs.to(backend.dev), return_loss=False, ref_seg_map=hm, img_meta=[dict(original_shape=(H, W, 3))])
        maps = out[0]
        assert maps.shape == (3, 15, H, W) and maps.dtype == np.float32
        assert np.array_equal(maps[0], hm[0].cpu().numpy())              # frame 0: the drawn maps themselves (same size)
        ev = vfs_amd.JHMDBEvaluator([gt], device=backend.dev)
        with pytest.raises(ZeroDivisionError):                           # ... as in the reference
            ev.evaluate([maps])
        maps = maps.copy()
        maps[1, 5, 10, 10] = 1.0                                         # make it visible once
        got = ev.evaluate([maps])
        coords = vfs_amd.heatmap_coords(maps, TOPK, backend.dev)
    assert same_bits(coords, O.heatmap_coords(maps, TOPK))
    # frame 0: the top-5 mean of a drawn Gaussian is its centre, int()-truncated from the key point: less than a pixel away
    assert np.abs(coords[:, np.arange(15) != 5, 0] - pose[:, np.arange(15) != 5]).max() < 1.0
    want = O.pck_evaluate([maps], [gt], TOPK)
    for k in want:
        assert abs(got[k] - want[k]) < 1e-12, (k, got[k], want[k])
    assert got['PCK@0.5'] > 0


def test_end_to_end_part_propagation_miou(backend):
    import vfs_amd
    model = _model(backend.dev)
    imgs, (H, W) = _small_clip(3)
    _, seg = O.seeded_labels(4, 1, H, W, num_classes=6, ignore_index=None, absent=(4,))
    gt = np.repeat(seg, 3, axis=0)
    gt[1:, ::7, ::5] = 255                                               # ignored pixels in the later frames
    with use_lib(backend):
        out = model(imgs.to(backend.dev), return_loss=False, ref_seg_map=torch.from_numpy(seg[0])[None],
                    img_meta=[dict(original_shape=(H, W, 3))])
        assert out[0].shape == (3, H, W) and out[0].dtype == np.uint8
        ev = vfs_amd.VIPEvaluator([gt], num_classes=6, device=backend.dev)
        got = ev.evaluate(out)
    want, want_cls, want_counts = O.vip_evaluate(out, [gt], 6, 255)
    assert np.array_equal(ev.counts, want_counts) and np.isnan(ev.per_class['IoU'][4])
    for k in want:
        assert abs(got[k] - want[k]) < 1e-12, (k, got[k], want[k])
    assert got['aAcc'] > 1 / 3                                           # frame 0 is the given map


# ---- 5. full sizes (GPU only) --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_topk_jhmdb_size_bit_exact(gpu_backend):
    """40 frames x 15 key points x 240 x 320: every map against the oracle, ties included (every other map is quantised)"""
    from vfs_amd import prop_eval as PE
    T, K, H, W = 40, 15, 240, 320
    maps = np.random.RandomState(77).rand(T, K, H, W).astype(np.float32)
    maps[::2] = np.floor(maps[::2] * 4096) / 4096
    maps[3, 4] = 0
    maps[5, 6] *= (maps[5, 6] > 0.9999)
    with use_lib(gpu_backend):
        vals, idx, minv, flags = PE.heatmap_topk(torch.from_numpy(maps).to(gpu_backend.dev), TOPK)
        coords = PE.heatmap_coords(torch.from_numpy(maps).to(gpu_backend.dev), TOPK)
    wv, wi, wm, wf = O.heatmap_topk(maps.reshape(T * K, H * W), TOPK)
    assert np.array_equal(idx.reshape(T * K, TOPK), wi) and same_bits(vals.reshape(T * K, TOPK), wv)
    assert np.array_equal(minv.reshape(-1), wm) and np.array_equal(flags.reshape(-1), wf) and flags[3, 4] == 1
    assert same_bits(coords, O.heatmap_coords(maps, TOPK))


@pytest.mark.gpu
def test_label_counts_vip_size_bit_exact(gpu_backend):
    """8 frames of 720 x 1280, 20 classes, 5 % ignored"""
    from vfs_amd import prop_eval as PE
    pred, gt = O.seeded_labels(88, 8, 720, 1280, ignore_frac=0.05)
    with use_lib(gpu_backend):
        c = PE.label_counts(torch.from_numpy(pred).to(gpu_backend.dev), torch.from_numpy(gt).to(gpu_backend.dev), 20, 255)
        ev = PE.VIPEvaluator([gt[:4], gt[4:]], device=gpu_backend.dev)
        got = ev.evaluate([pred[:4], pred[4:]])
    want = O.label_counts(pred, gt, 20, 255)
    assert np.array_equal(c.cpu().numpy(), want) and np.array_equal(ev.counts, want)
    summary, _, _ = O.vip_evaluate([pred], [gt])
    for k in summary:
        assert abs(got[k] - summary[k]) < 1e-12
