#!/usr/bin/env python3
"""Golden key-point heat maps, coordinates, PCK and mIoU numbers from the REAL reference functions, run in the build
container only (numpy 2 / scipy; `np.float = float` restores the alias the reference still uses):

* `draw_label_map` (mmaction/datasets/pipelines/loading.py:1074-1101), imported from its file
* `JHMDBDataset.img2coord`, `.compute_pck`, `.pck_evaluate`, `.evaluate` (datasets/jhmdb_dataset.py), the class imported from
  its file with a stub parent; `pck_evaluate` reads joint_positions.mat files that scipy.io.savemat writes to a temporary tree
* `intersect_and_union`, `total_intersect_and_union`, `mean_iou` (core/evaluation/iou.py), imported from its file
* `VIPDataset.vip_evaluate` (datasets/vip_dataset.py) on PNG files in a temporary tree, for the rounding of the summary

Stand-ins for what is absent here: `mmcv` (gen_golden.install_mmcv_standin, plus `imread` = PIL and `fileio.FileClient`),
`terminaltables.AsciiTable` (printing only), `mmaction.utils` (add_prefix; terminal_is_available = False), the parent
class RawframeDataset (holds `video_infos` only).

RESTATED here, not driven through the reference: the dozen lines of RawFrameDecode's pose_coord branch around
draw_label_map (loading.py:1055-1069: the loop over key points and the single-pixel case for sigma <= 0) - the class
reads frames from disk first.

Inputs are seeded (tests/prop_eval_oracle.py: seeded_maps / seeded_labels), so the file stores seeds, integers and outputs.
For every map recorded for a bit-for-bit coordinate comparison the generator ASSERTS that its topk + 1 largest values
are pairwise distinct or the map is all zero (np.argsort leaves ties open); the share of maps left out is 0.

Usage: python tests/golden/gen_prop_eval_golden.py   (writes tests/golden/prop_eval.npz)"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import scipy.io as sio
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from gen_golden import REF, install_mmcv_standin  # noqa: E402
from tests.prop_eval_oracle import seeded_labels, seeded_maps  # noqa: E402

TOPK = 5
# (seed, T, K, H, W, zero maps, sparse maps)
COORD_CASES = [(11, 3, 15, 24, 32, ((1, 4),), ((0, 2), (2, 9))), (12, 2, 15, 37, 53, ((0, 0), (1, 14)), ((1, 7),))]
# key points [2][K] on a 24 x 32 and a 37 x 53 map: inside, fractional, straddling each border and corner, negative
# fractional corners (int() truncates towards zero), fully outside in every direction, just outside (br < 0 / ul >= size)
POSE_XY = np.array([[16, 10.25, 0.5, 31.2, 15.0, 14.7, -1.5, 33.9, 1.5, -6.9, -7.5, 38.5, 16.0, 16.0, 200.0, -0.5, 31.99, 29.0],
                    [12, 7.75, 11.0, 12.0, 0.2, 23.4, -2.5, 25.1, 1.5, 5.0, 5.0, 12.0, -7.5, 30.5, 12.0, -0.5, 23.99, 36.5]])
POSE_CASES = [(24, 32, 2), (24, 32, 1), (24, 32, 0), (37, 53, 4), (37, 53, 0)]
# (seed, T, H, W) per video; 20 classes, ignore 255, class 7 absent from both maps
LABEL_CASES = [(21, 3, 24, 32), (22, 2, 37, 53)]
# PCK: (seed, T_result, H, W, zero maps, T_gt)
PCK_CASES = [(31, 4, 24, 32, ((1, 3), (2, 3)), 4), (32, 5, 37, 53, ((0, 0),), 3)]


def import_reference():
    install_mmcv_standin()
    np.float = float
    mmcv = sys.modules['mmcv']
    mmcv.imread = lambda path, flag='color', channel_order='bgr', backend=None: np.array(Image.open(path))
    fileio = types.ModuleType('mmcv.fileio')
    fileio.FileClient = mmcv.FileClient
    sys.modules['mmcv.fileio'] = mmcv.fileio = fileio
    tt = types.ModuleType('terminaltables')
    tt.AsciiTable = type('AsciiTable', (), {'__init__': lambda self, data: setattr(self, 'table', '')})
    sys.modules['terminaltables'] = tt
    sys.path.insert(0, REF)
    for name in ['mmaction', 'mmaction.core', 'mmaction.core.evaluation', 'mmaction.datasets', 'mmaction.datasets.pipelines']:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, *name.split('.'))]
        sys.modules[name] = m
    utils = types.ModuleType('mmaction.utils')
    utils.add_prefix = lambda inputs, prefix: {f'{prefix}.{k}': v for k, v in inputs.items()}
    utils.terminal_is_available = lambda: False
    utils.get_random_string = utils.get_shm_dir = utils.get_thread_id = lambda *a, **k: None
    sys.modules['mmaction.utils'] = utils
    parent = types.ModuleType('mmaction.datasets.rawframe_dataset')

    class RawframeDataset:
        def __init__(self, *a, **k):
            pass

        def __len__(self):
            return len(self.video_infos)
    parent.RawframeDataset = RawframeDataset
    sys.modules['mmaction.datasets.rawframe_dataset'] = parent
    iou = importlib.import_module('mmaction.core.evaluation.iou')
    jhmdb = importlib.import_module('mmaction.datasets.jhmdb_dataset')
    vip = importlib.import_module('mmaction.datasets.vip_dataset')
    loading = importlib.import_module('mmaction.datasets.pipelines.loading')
    return iou, jhmdb.JHMDBDataset, vip.VIPDataset, loading.draw_label_map


def pose_map(draw_label_map, pose_coord, sigma, H, W):
    """RESTATED loop of loading.py:1055-1069 around the reference's draw_label_map -> float64 [K][H][W]"""
    num_poses = pose_coord.shape[1]
    out = np.zeros((H, W, num_poses), dtype=float)
    for j in range(num_poses):
        if sigma > 0:
            draw_label_map(out[:, :, j], pose_coord[:, j], sigma)
        else:
            tx, ty = int(pose_coord[0, j]), int(pose_coord[1, j])
            if 0 <= tx < W and 0 <= ty < H:
                out[ty, tx, j] = 1.0
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def assert_tie_free(maps, topk):
    flat = maps.reshape(-1, maps.shape[-2] * maps.shape[-1])
    for m in flat:
        top = np.sort(m)[-(topk + 1):]
        assert not m.any() or len(np.unique(top)) == topk + 1, 'a recorded map has a tie among its topk + 1 largest values'


def main():
    iou, JHMDBDataset, VIPDataset, draw_label_map = import_reference()
    out = {}

    # ---- heat maps
    out['pose/xy'] = POSE_XY
    out['pose/cases'] = np.asarray(POSE_CASES, np.int64)
    for i, (H, W, sigma) in enumerate(POSE_CASES):
        hm = pose_map(draw_label_map, POSE_XY, sigma, H, W)
        out[f'pose/{i}/map'] = hm.astype(np.float32)          # the float64 map rounded to fp32
        print('pose', (H, W, sigma), 'non-zero key points', int((hm.reshape(len(hm), -1).max(1) > 0).sum()), 'of', len(hm))

    # ---- coordinates (img2coord)
    jh = object.__new__(JHMDBDataset)
    out['coord/cases'] = np.asarray([c[:5] for c in COORD_CASES], np.int64)
    for i, (seed, T, K, H, W, zero, sparse) in enumerate(COORD_CASES):
        maps = seeded_maps(seed, T, K, H, W, zero, sparse)
        assert_tie_free(maps, TOPK)
        out[f'coord/{i}/zero'] = np.asarray(zero, np.int64).reshape(-1, 2)
        out[f'coord/{i}/sparse'] = np.asarray(sparse, np.int64).reshape(-1, 2)
        with np.errstate(invalid='ignore', divide='ignore'):
            out[f'coord/{i}/coords'] = jh.img2coord(maps, topk=TOPK)
    # the reference's own symmetric Gaussian: four equal neighbours of the peak, the 6th value strictly smaller - the selected
    # SET is unambiguous, the float64 summation order is not (compared at 1e-9 pixels)
    sym_xy = np.stack([np.linspace(8, 24, 15).round(), np.linspace(7, 17, 15).round()])
    sym = pose_map(draw_label_map, sym_xy, 2, 24, 32).astype(np.float32)[None]
    for m in sym[0]:
        top = np.sort(m.reshape(-1))[-6:]
        assert top[5] > top[4] == top[1] > top[0]
    out['coord/sym/xy'] = sym_xy
    out['coord/sym/coords'] = jh.img2coord(sym, topk=TOPK)

    # ---- PCK (pck_evaluate / evaluate on joint_positions.mat files)
    out['pck/cases'] = np.asarray([(c[0], c[1], c[2], c[3], c[5]) for c in PCK_CASES], np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        results, infos = [], []
        rng = np.random.RandomState(5)
        for i, (seed, T, H, W, zero, T_gt) in enumerate(PCK_CASES):
            maps = seeded_maps(seed, T, 15, H, W, zero)
            assert_tie_free(maps, TOPK)
            with np.errstate(invalid='ignore', divide='ignore'):
                pred = jh.img2coord(maps, topk=TOPK)
            gt = np.round(pred[..., :T_gt] + rng.normal(0, 2.5, (2, 15, T_gt)), 2)     # ground truth near the predictions
            frame_dir = os.path.join(tmp, 'data', 'Frames', f'v{i}')
            ann_dir = os.path.join(tmp, 'anno', 'joint_positions', f'v{i}')
            os.makedirs(ann_dir)
            sio.savemat(os.path.join(ann_dir, 'joint_positions.mat'), {'pos_img': gt + 1})
            infos.append(dict(frame_dir=frame_dir, total_frames=T))
            results.append(maps)
            out[f'pck/{i}/zero'] = np.asarray(zero, np.int64).reshape(-1, 2)
            out[f'pck/{i}/gt'] = gt
        jh.video_infos, jh.data_prefix, jh.anno_prefix = infos, os.path.join(tmp, 'data'), os.path.join(tmp, 'anno')
        with np.errstate(invalid='ignore', divide='ignore'):
            pck = jh.evaluate(results, metrics='pck')
            feat = jh.evaluate([[r, r] for r in results], metrics='pck')
    out['pck/keys'] = np.asarray(list(pck))
    out['pck/values'] = np.asarray([pck[k] for k in pck], np.float64)
    out['pck/feat_keys'] = np.asarray(list(feat))
    out['pck/feat_values'] = np.asarray([feat[k] for k in feat], np.float64)
    print('pck', pck)
    d = [np.asarray([0.05, 0.1, 0.30000000000000004, 0.7]), np.asarray([0.2]), np.asarray([0.5, 0.6])]
    out['pck/compute_in'] = np.concatenate(d)
    out['pck/compute_split'] = np.asarray([len(x) for x in d], np.int64)
    out['pck/compute_out'] = np.stack([JHMDBDataset.compute_pck(d, a) for a in (0.1, 0.2, 0.3, 0.4, 0.5)])

    # ---- mIoU
    out['label/cases'] = np.asarray(LABEL_CASES, np.int64)
    preds, gts = [], []
    for seed, T, H, W in LABEL_CASES:
        p, g = seeded_labels(seed, T, H, W)
        assert (p == 20).any() and (p == 23).any() and (g == 255).any() and not (p == 7).any() and not (g == 7).any()
        preds.append(p)
        gts.append(g)
    frames_p = [f for p in preds for f in p]
    frames_g = [f for g in gts for f in g]
    per_frame = np.stack([np.stack(iou.intersect_and_union(p, g, 20, 255)) for p, g in zip(frames_p, frames_g)])
    out['label/per_frame'] = per_frame.astype(np.int64)                     # [frames][4][20]: intersect, union, pred, label
    out['label/total'] = np.stack(iou.total_intersect_and_union(frames_p, frames_g, 20, 255))
    with np.errstate(invalid='ignore', divide='ignore'):
        all_acc, acc, miou = iou.mean_iou(frames_p, frames_g, 20, 255)
    out['label/all_acc'], out['label/acc'], out['label/iou'] = np.float64(all_acc), acc, miou
    tiny = np.full((2, 2), 20, np.uint8)      # np.histogram's closed last bin
    out['label/closed_bin'] = np.stack(iou.intersect_and_union(tiny, tiny.copy(), 20, 255)).astype(np.int64)
    # vip_evaluate on files: frames *.jpg (names only), annotations and predictions *.png
    with tempfile.TemporaryDirectory() as tmp:
        vip = object.__new__(VIPDataset)
        vip.data_prefix, vip.anno_prefix = os.path.join(tmp, 'Images'), os.path.join(tmp, 'Annotations')
        vip.video_infos = []
        for i, (p, g) in enumerate(zip(preds, gts)):
            fd, ad = os.path.join(vip.data_prefix, f'v{i}'), os.path.join(vip.anno_prefix, f'v{i}')
            os.makedirs(fd)
            os.makedirs(ad)
            for f in range(len(g)):
                open(os.path.join(fd, f'{f:012}.jpg'), 'wb').close()
                Image.fromarray(g[f]).save(os.path.join(ad, f'{f:012}.png'))
            vip.video_infos.append(dict(frame_dir=fd, total_frames=len(g)))
        with np.errstate(invalid='ignore', divide='ignore'):
            summary = vip.evaluate(preds, metrics='mIoU', output_dir=os.path.join(tmp, 'out'))
    out['label/summary_keys'] = np.asarray(list(summary))
    out['label/summary_values'] = np.asarray([summary[k] for k in summary], np.float64)
    print('vip', summary)

    path = os.path.join(HERE, 'prop_eval.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
