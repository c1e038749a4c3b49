"""JHMDB pose (PCK) and VIP human-part (mIoU) evaluation of label propagation on the GPU: counterparts of
JHMDBDataset.img2coord / .pck_evaluate / .evaluate (reference mmaction/datasets/jhmdb_dataset.py:107-242), of
VIPDataset.vip_evaluate / .evaluate (datasets/vip_dataset.py:71-184) over mean_iou (core/evaluation/iou.py) and of
the key-point heat maps RawFrameDecode draws for the tracker (datasets/pipelines/loading.py:1055-1101).

The passes over full-resolution maps run on the device (csrc/propeval.hip: vfs_heatmap_topk, vfs_label_counts,
vfs_pose_heatmaps); what is left - a handful of numbers per map or per class - is finished on the host with the
reference's own numpy expressions in float64.  Ground truth is handed over as arrays instead of dataset directories;
results may be numpy arrays, `.npy` paths (save_np) or torch tensors on either device.

Not pinned to the reference: its Resize step interpolates a float ref_seg_map with cv2 (augmentations.py:583-587) and no
JHMDB / VIP config ships with it, so `pose_heatmaps` draws at the size it is given, in the [1][K][H][W] layout
`forward_test` takes."""
import numpy as np
import torch

from ._lib import get_lib
from .davis_eval import save_palette_pngs

NUM_KEYPOINTS = 15                           # jhmdb_dataset.py:18
PCK_RANGES = (0.1, 0.2, 0.3, 0.4, 0.5)       # jhmdb_dataset.py:210
MAX_TOPK = 8
MAX_PATCH = 1024
TOPK_ALL_ZERO, TOPK_NAN, TOPK_NEG_INF = 1, 2, 4      # flags of vfs_heatmap_topk
# vip_dataset.py:26-31
VIP_CLASSES = ['background', 'hat', 'hair', 'sun-glasses', 'upper-clothes', 'dress', 'coat', 'socks', 'pants', 'gloves',
               'scarf', 'skirt', 'torso-skin', 'face', 'right-arm', 'left-arm', 'right-leg', 'left-leg', 'right-shoe',
               'left-shoe']


def _device(device, *tensors):
    if device is not None:
        return torch.device(device)
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device('cuda')


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream if device.type == 'cuda' else None


def _load(x):
    """a result as the tracker hands it over: array, tensor, or the path of a save_np file"""
    if isinstance(x, str):
        return np.load(x)
    return x


def _to(x, device, dtype):
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.ascontiguousarray(x))
    return x.to(device=device, dtype=dtype).contiguous()


# ---- key-point heat maps -----------------------------------------------------------------------------------------
def gaussian_patch(sigma):
    """float64 [P][P], P = 6 sigma + 1: exp(-d^2 / (2 sigma^2)) around the centre pixel, 1 at the centre (the values
    draw_label_map pastes, loading.py:1086-1091); [[1.]] for sigma <= 0"""
    if sigma <= 0:
        return np.ones((1, 1), dtype=np.float64)
    side = 6 * sigma + 1
    if not float(side).is_integer() or side > MAX_PATCH:
        raise ValueError(f'pose_heatmaps: 6 * sigma + 1 must be an integer <= {MAX_PATCH} (got sigma = {sigma})')
    side = int(side)
    d2 = (np.arange(side, dtype=np.float64) - side // 2) ** 2
    return np.exp(-(d2[None, :] + d2[:, None]) / (2 * sigma**2))


def keypoint_corners(pose_coord, sigma, H, W):
    """int32 [K][5] = ul_x, ul_y, br_x, br_y, inside.  Corners truncate towards zero as the reference's int() does
    (loading.py:1078-1079), `inside` is the outcome of its early-return test (:1080-1083); for sigma <= 0 the corner is
    the single pixel (int(x), int(y)) and `inside` its bounds test (:1065-1067)."""
    xy = np.asarray(pose_coord, dtype=np.float64).T                 # [K][2]
    if not np.isfinite(xy).all():
        raise ValueError('pose_heatmaps: key-point coordinates must be finite')
    if sigma > 0:
        lo, hi = np.trunc(xy - 3 * sigma), np.trunc(xy + 3 * sigma + 1)
        inside = (lo[:, 0] < W) & (lo[:, 1] < H) & (hi[:, 0] >= 0) & (hi[:, 1] >= 0)
    else:
        lo = np.trunc(xy)
        hi = lo + 1
        inside = (lo[:, 0] >= 0) & (lo[:, 0] < W) & (lo[:, 1] >= 0) & (lo[:, 1] < H)
    far = float(1 << 30)                                            # far outside either way
    kp = np.concatenate([np.clip(lo, -far, far), np.clip(hi, -far, far), inside[:, None].astype(np.float64)], axis=1)
    return np.ascontiguousarray(kp, dtype=np.int32)         # (the transposed input makes numpy choose column-major above)


def pose_heatmaps(pose_coord, sigma, H, W, device=None):
    """pose_coord [2][K] (x row, y row; 0-based) -> fp32 [1][K][H][W] on `device`: the reference's float64 pose_map
    rounded to fp32, in the layout forward_test takes as a 4-D ref_seg_map."""
    pose_coord = pose_coord.detach().cpu().numpy() if torch.is_tensor(pose_coord) else np.asarray(pose_coord)
    if pose_coord.ndim != 2 or pose_coord.shape[0] != 2:
        raise ValueError(f'pose_heatmaps: pose_coord must be [2][K] (got {pose_coord.shape})')
    K = pose_coord.shape[1]
    if K > 65535 or H < 1 or W < 1 or H * W > 1 << 30:
        raise NotImplementedError(f'pose_heatmaps: at most 65535 key points and 2^30 pixels per map (got {K}, {H} x {W})')
    device = _device(device)
    patch = torch.from_numpy(gaussian_patch(sigma).astype(np.float32)).to(device)
    kp = torch.from_numpy(keypoint_corners(pose_coord, sigma, H, W)).to(device)
    out = torch.empty(1, K, H, W, dtype=torch.float32, device=device)
    get_lib().pose_heatmaps(patch, kp, out, K, H, W, patch.shape[0], _stream(device))
    return out


# ---- heat maps -> coordinates ------------------------------------------------------------------------------------
def heatmap_topk(maps, topk=5, device=None):
    """maps [..., H, W] -> (values fp32 [..., topk], indices int64 [..., topk], minimum fp32 [...], flags int32 [...]) as
    numpy arrays, in the order of vfs_heatmap_topk (ascending; ties: the lower flat index ranks higher)."""
    if not 1 <= topk <= MAX_TOPK:
        raise NotImplementedError(f'heatmap_topk: topk 1..{MAX_TOPK} (got {topk})')
    device = _device(device, maps)
    maps = _to(_load(maps), device, torch.float32)
    lead, (H, W) = tuple(maps.shape[:-2]), maps.shape[-2:]
    if H * W < topk:
        raise ValueError(f'heatmap_topk: a {H} x {W} map has fewer than topk = {topk} elements')
    if H * W > 1 << 28:
        raise NotImplementedError(f'heatmap_topk: at most 2^28 pixels per map (got {H} x {W})')
    N = int(np.prod(lead, dtype=np.int64))
    vals = torch.empty(N, topk, dtype=torch.float32, device=device)
    idx = torch.empty(N, topk, dtype=torch.int32, device=device)
    minv = torch.empty(N, dtype=torch.float32, device=device)
    flags = torch.empty(N, dtype=torch.int32, device=device)
    get_lib().heatmap_topk(maps, vals, idx, minv, flags, N, H, W, topk, _stream(device))
    return (vals.cpu().numpy().reshape(lead + (topk,)), idx.cpu().numpy().astype(np.int64).reshape(lead + (topk,)),
            minv.cpu().numpy().reshape(lead), flags.cpu().numpy().reshape(lead))


def heatmap_coords(maps, topk=5, device=None):
    """JHMDBDataset.img2coord (jhmdb_dataset.py:118-136): maps [T][K][H][W] -> float64 [2][K][T] (x, y), -1 for an
    all-zero map.  The top-k selection runs on the device; the weighted mean is the reference's numpy arithmetic."""
    maps = _load(maps)
    if len(maps.shape) != 4:
        raise ValueError(f'heatmap_coords: maps must be [T][K][H][W] (got {tuple(maps.shape)})')
    width = maps.shape[3]
    vals, flat, minv, flags = heatmap_topk(maps, topk, device)
    if (flags & TOPK_NAN).any():
        raise ValueError('heatmap_coords: a map holds a NaN')
    if (flags & TOPK_NEG_INF).any():
        raise ValueError('heatmap_coords: a map holds a negative infinity (propagated heat maps are non-negative)')
    if (minv < 0).any():
        # the reference tests `sum == 0` for "all zero", which is that test only for non-negative maps
        raise ValueError('heatmap_coords: a map holds a negative value (propagated heat maps are non-negative)')
    # weights in fp32 (value / fp32 sum of the topk values), positions as integers, products and sums in float64 in
    # ascending rank order: the arithmetic img2coord is pinned to by tests/golden/prop_eval.npz
    with np.errstate(invalid='ignore', divide='ignore'):
        weight = vals / vals.sum(axis=-1, keepdims=True)
    row, col = np.divmod(flat, width)
    xy = np.stack([(col * weight).sum(axis=-1), (row * weight).sum(axis=-1)])      # [2][T][K]
    xy = np.ascontiguousarray(xy.transpose(0, 2, 1))
    xy[:, ((flags & TOPK_ALL_ZERO) != 0).T] = -1
    return xy


def normalised_distances(pred, gt):
    """pred, gt float64 [2][K][T] of one video -> per key point the distances of its visible predictions (x > 0) to the
    ground truth, in units of 0.6 x the diagonal of the box around the ground-truth points that are visible in that frame
    (jhmdb_dataset.py:182-207)"""
    if pred.shape != gt.shape:
        raise ValueError(f'pck: predictions {pred.shape} and ground truth {gt.shape} differ in shape')
    seen = pred[0] > 0                                                   # [K][T]
    upper = np.where(seen, gt, -1.0).max(axis=1)                         # [2][T]; the fill values are the reference's
    lower = np.where(seen, gt, 1e6).min(axis=1)
    unit = 0.6 * np.sqrt(((upper - lower) ** 2).sum(axis=0))             # [T]
    with np.errstate(invalid='ignore', divide='ignore'):
        d = np.sqrt(((pred - gt) ** 2).sum(axis=0)) / unit[None, :]      # [K][T]
    return [d[k, seen[k]] for k in range(pred.shape[1])]


def pck_from_poses(preds, gts, num_keypoints=NUM_KEYPOINTS):
    """mean over the key points of the share (in percent) of visible predictions within alpha box units, for every alpha
    of PCK_RANGES (compute_pck and the tail of pck_evaluate, jhmdb_dataset.py:107-116,210-218).  A key point without a
    single visible prediction in the whole dataset: ZeroDivisionError, as there."""
    per_video = [normalised_distances(p, g) for p, g in zip(preds, gts)]
    pooled = [np.concatenate([v[k] for v in per_video]) if per_video else np.zeros(0) for k in range(num_keypoints)]
    out = {}
    for alpha in PCK_RANGES:
        share = [100.0 * int((d <= alpha).sum()) / int(d.size) for d in pooled]
        out[f'PCK@{alpha}'] = np.mean(np.asarray(share))
    return out


class JHMDBEvaluator:
    """`evaluate(results, metrics='pck')` of the reference's JHMDBDataset, fed with the ground-truth key points instead
    of joint_positions.mat files: gt_poses = list of float [2][15][T_gt] (one per video, already 0-based: the
    reference subtracts 1 from pos_img), results = list of propagated heat maps [T][15][H][W]."""

    def __init__(self, gt_poses, names=None, device=None, topk=5):
        self.gt_poses = [np.asarray(g, dtype=np.float64) for g in gt_poses]
        for g in self.gt_poses:
            if g.ndim != 3 or g.shape[:2] != (2, NUM_KEYPOINTS):
                raise ValueError(f'JHMDBEvaluator: ground truth must be [2][{NUM_KEYPOINTS}][T] (got {g.shape})')
        self.names = list(names) if names is not None else [f'video{i:03d}' for i in range(len(self.gt_poses))]
        self.device = device
        self.topk = topk

    def __len__(self):
        return len(self.gt_poses)

    def pck_evaluate(self, results, output_dir=None, logger=None):
        assert len(results) == len(self)
        preds, gts = [], []
        for res, gt in zip(results, self.gt_poses):
            res = _load(res)
            clip_len = min(len(res), gt.shape[-1])          # the shorter of the two decides (jhmdb_dataset.py:157-160)
            res = res[:clip_len]
            if tuple(res.shape[:2]) != (clip_len, NUM_KEYPOINTS):
                raise ValueError(f'JHMDBEvaluator: a result must be [T][{NUM_KEYPOINTS}][H][W] (got {tuple(res.shape)})')
            preds.append(heatmap_coords(res, self.topk, self.device))
            gts.append(gt[..., :clip_len])
        self.pred_poses = preds
        out = pck_from_poses(preds, gts)
        if logger is not None:
            logger.info('PCK: ' + ', '.join(f'{k} {v:.2f}' for k, v in out.items()))
        return out

    def evaluate(self, results, metrics='pck', output_dir=None, logger=None):
        metrics = metrics if isinstance(metrics, (list, tuple)) else [metrics]
        for metric in metrics:
            if metric not in ('pck',):
                raise KeyError(f'metric {metric} is not supported')
        out = {}
        if len(results) and all(isinstance(r, list) for r in results):      # several feature levels (jhmdb_dataset.py:228-235)
            for fi in range(len(results[0])):
                part = self.pck_evaluate([r[fi] for r in results], output_dir, logger)
                out.update({f'feat_{fi}.{k}': v for k, v in part.items()})
        else:
            out.update(self.pck_evaluate(results, output_dir, logger))
        return out


# ---- label maps -> mIoU ------------------------------------------------------------------------------------------
def label_counts(pred, gt, num_classes, ignore_index=255, device=None, out=None):
    """pred, gt: label maps of one shape (any rank) -> int64 tensor [num_classes][3] on the device = intersect, prediction
    area, label area of intersect_and_union (iou.py:51-60), ADDED onto `out` when one is given."""
    if not 1 <= num_classes <= 256:
        raise NotImplementedError(f'label_counts: 1..256 classes (got {num_classes})')
    ignore = -1 if ignore_index is None else int(ignore_index)
    if not -1 <= ignore <= 255:
        raise ValueError(f'label_counts: ignore_index 0..255, or None / -1 for none (got {ignore_index})')
    device = _device(device, pred, gt) if out is None else out.device
    pred, gt = _load(pred), _load(gt)
    if not torch.is_tensor(pred):
        pred = np.asarray(pred).astype(np.uint8)            # vip_dataset.py:101
    pred, gt = _to(pred, device, torch.uint8), _to(gt, device, torch.uint8)
    if pred.shape != gt.shape:
        raise ValueError(f'label_counts: prediction {tuple(pred.shape)} and ground truth {tuple(gt.shape)} differ in shape')
    if out is None:
        out = torch.zeros(num_classes, 3, dtype=torch.int64, device=device)
    assert out.shape == (num_classes, 3) and out.dtype == torch.int64 and out.is_contiguous()
    get_lib().label_counts(pred, gt, out, pred.numel(), num_classes, ignore, _stream(device))
    return out


def metrics_from_counts(counts):
    """counts int [num_classes][3] -> (overall accuracy, accuracy [num_classes], IoU [num_classes]) in float64: hits over
    label pixels, per class and in total, and hits over the union (eval_metrics, iou.py:213-224); NaN for an absent class"""
    hit, predicted, labelled = (np.asarray(counts)[:, c].astype(np.float64) for c in range(3))
    with np.errstate(invalid='ignore', divide='ignore'):
        return hit.sum() / labelled.sum(), hit / labelled, hit / (predicted + labelled - hit)


def summary_from_metrics(metrics):
    """(overall accuracy, accuracy, IoU) -> ({'mIoU', 'mAcc', 'aAcc'}, {'IoU': [..], 'Acc': [..]} in percent) with the
    rounding of vip_evaluate (vip_dataset.py:119-147): percent rounded to two decimals, class means skip NaN, summary / 100"""
    def percent(v):
        return np.round(v * 100, 2)
    with np.errstate(invalid='ignore'):
        a_acc, m_acc, m_iou = (percent(np.nanmean(m)) for m in metrics)
    return {'mIoU': m_iou / 100.0, 'mAcc': m_acc / 100.0, 'aAcc': a_acc / 100.0}, {'IoU': percent(metrics[2]), 'Acc': percent(metrics[1])}


class VIPEvaluator:
    """`evaluate(results, metrics='mIoU')` of the reference's VIPDataset, fed with ground-truth part maps instead of
    annotation directories: gts = list of uint8 [T][H][W] (one per video; videos may differ in size).  The counts of the
    whole dataset are summed on the device (one vfs_label_counts call per video) and read back once."""

    def __init__(self, gts, num_classes=20, ignore_index=255, names=None, device=None, class_names=None):
        if not 1 <= num_classes <= 256:
            raise NotImplementedError(f'VIPEvaluator: 1..256 classes (got {num_classes})')
        self.gts = list(gts)
        self.num_classes, self.ignore_index = num_classes, ignore_index
        self.names = list(names) if names is not None else [f'video{i:03d}' for i in range(len(self.gts))]
        self.class_names = list(class_names) if class_names is not None else (
            VIP_CLASSES if num_classes == len(VIP_CLASSES) else [str(i) for i in range(num_classes)])
        self.device = device

    def __len__(self):
        return len(self.gts)

    def vip_evaluate(self, results, output_dir=None, logger=None):
        assert len(results) == len(self)
        results = [_load(r) for r in results]
        for name, res, gt in zip(self.names, results, self.gts):
            assert len(res) == len(gt), (name, len(res), len(gt))
        if output_dir is not None:
            save_palette_pngs(results, output_dir, self.names)
        device = _device(self.device, *results, *self.gts)
        counts = torch.zeros(self.num_classes, 3, dtype=torch.int64, device=device)
        for res, gt in zip(results, self.gts):
            label_counts(res, gt, self.num_classes, self.ignore_index, out=counts)
        self.counts = counts.cpu().numpy()
        summary, self.per_class = summary_from_metrics(metrics_from_counts(self.counts))
        if logger is not None:
            logger.info('Summary: ' + ', '.join(f'{k} {v * 100:.2f}' for k, v in summary.items()))
        return summary

    def evaluate(self, results, metrics='mIoU', output_dir=None, logger=None):
        metrics = metrics if isinstance(metrics, (list, tuple)) else [metrics]
        for metric in metrics:
            if metric not in ('mIoU',):
                raise KeyError(f'metric {metric} is not supported')
        out = {}
        first = results[0]
        if isinstance(first, list) or getattr(first, 'ndim', 0) == 4:      # several feature levels (array or tensor)
            for fi in range(len(first)):
                part = self.vip_evaluate([r[fi] for r in results], output_dir, logger)
                out.update({f'feat_{fi}.{k}': v for k, v in part.items()})
        else:
            out.update(self.vip_evaluate(results, output_dir, logger))
        return out
