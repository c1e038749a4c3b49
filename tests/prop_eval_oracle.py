"""numpy restatement of the JHMDB / VIP evaluation path (vfs_amd/prop_eval.py over csrc/propeval.hip): the contracts of the
three kernels as include/vfs_hip.h states them, and the two evaluators with the reference's arithmetic
(mmaction/datasets/jhmdb_dataset.py:107-218, datasets/vip_dataset.py:114-147, core/evaluation/iou.py:5-63,183-233,
datasets/pipelines/loading.py:1055-1101).  Nothing here touches the library; tests/golden/prop_eval.npz pins it to the
reference's own functions (tests/golden/gen_prop_eval_golden.py)."""
import numpy as np

NUM_KEYPOINTS = 15
PCK_RANGES = (0.1, 0.2, 0.3, 0.4, 0.5)
TOPK_ALL_ZERO, TOPK_NAN, TOPK_NEG_INF = 1, 2, 4


# ---- seeded inputs shared by the golden generator and the tests (RandomState streams are frozen by numpy) ----------------
def seeded_maps(seed, T, K, H, W, zero=(), sparse=()):
    """non-negative fp32 maps [T][K][H][W] with continuous values; `zero`: (t, k) maps set to 0; `sparse`: (t, k) maps that
    keep only 9 non-zero pixels (what a propagated key point looks like)"""
    rng = np.random.RandomState(seed)
    maps = rng.rand(T, K, H, W).astype(np.float32)
    for t, k in zero:
        maps[t, k] = 0
    for t, k in sparse:
        keep = rng.choice(H * W, 9, replace=False)
        m = np.zeros(H * W, np.float32)
        m[keep] = maps[t, k].reshape(-1)[keep]
        maps[t, k] = m.reshape(H, W)
    return maps


def seeded_labels(seed, T, H, W, num_classes=20, ignore_index=255, absent=(7,), ignore_frac=0.05, noise=0.2):
    """(pred, gt) uint8 [T][H][W]: blocky ground truth, a prediction that disagrees on `noise` of the pixels and also holds the
    values num_classes (np.histogram's closed last bin) and num_classes + 3 (dropped); `absent` classes occur in neither"""
    rng = np.random.RandomState(seed)
    classes = np.array([c for c in range(num_classes) if c not in absent], np.uint8)
    coarse = classes[rng.randint(0, len(classes), (T, (H + 5) // 6, (W + 7) // 8))]
    gt = np.repeat(np.repeat(coarse, 6, axis=1), 8, axis=2)[:, :H, :W].copy()
    pred = gt.copy()
    flip = rng.rand(T, H, W) < noise
    pred[flip] = classes[rng.randint(0, len(classes), int(flip.sum()))]
    special = rng.rand(T, H, W)
    pred[special < 0.02] = num_classes
    pred[(special >= 0.02) & (special < 0.03)] = min(num_classes + 3, 254)
    if ignore_index is not None:
        gt[rng.rand(T, H, W) < ignore_frac] = ignore_index
    return pred, gt


# ---- vfs_pose_heatmaps --------------------------------------------------------------------------------------------------
def gaussian_patch(sigma):
    if sigma <= 0:
        return np.ones((1, 1))
    size = 6 * sigma + 1
    x = np.arange(0, size, 1, float)
    y = x[:, np.newaxis]
    x0 = y0 = size // 2
    return np.exp(-((x - x0)**2 + (y - y0)**2) / (2 * sigma**2))


def keypoint_corners(pose_coord, sigma, H, W):
    rows = []
    for j in range(pose_coord.shape[1]):
        x, y = pose_coord[0, j], pose_coord[1, j]
        if sigma > 0:
            ul = [int(x - 3 * sigma), int(y - 3 * sigma)]
            br = [int(x + 3 * sigma + 1), int(y + 3 * sigma + 1)]
            inside = not (ul[0] >= W or ul[1] >= H or br[0] < 0 or br[1] < 0)
        else:
            ul = [int(x), int(y)]
            br = [ul[0] + 1, ul[1] + 1]
            inside = 0 <= ul[0] < W and 0 <= ul[1] < H
        rows.append(ul + br + [int(inside)])
    return np.asarray(rows, np.int64).reshape(-1, 5)


def paste_patch(patch, kp, H, W):
    """the kernel's contract: out[k][y][x] = patch[y - ul_y][x - ul_x] for max(0, ul) <= (x, y) < min(br, (W, H)) when inside"""
    out = np.zeros((len(kp), H, W), np.float32)
    P = patch.shape[0]
    for k, (ulx, uly, brx, bry, inside) in enumerate(kp):
        if not inside:
            continue
        for y in range(max(0, uly), min(bry, H)):
            for x in range(max(0, ulx), min(brx, W)):
                if y - uly < P and x - ulx < P:
                    out[k, y, x] = patch[y - uly, x - ulx]
    return out


def pose_heatmaps(pose_coord, sigma, H, W):
    """fp32 [K][H][W]"""
    pose_coord = np.asarray(pose_coord, np.float64)
    return paste_patch(gaussian_patch(sigma).astype(np.float32), keypoint_corners(pose_coord, sigma, H, W), H, W)


# ---- vfs_heatmap_topk ---------------------------------------------------------------------------------------------------
def heatmap_topk(maps, topk):
    """maps fp32 [N][HW] -> vals fp32 [N][topk], idx int64 [N][topk] (ascending rank: larger value ranks higher, among equal
    values the lower index ranks higher), minv fp32 [N], flags int32 [N].  A map with a NaN or a -inf: only its flags are defined."""
    maps = np.asarray(maps, np.float32)
    N, HW = maps.shape
    assert HW >= topk
    vals = np.zeros((N, topk), np.float32)
    idx = np.zeros((N, topk), np.int64)
    minv = np.zeros(N, np.float32)
    flags = np.zeros(N, np.int32)
    ar = np.arange(HW)
    for n in range(N):
        m = maps[n]
        bad = (TOPK_NAN if np.isnan(m).any() else 0) | (TOPK_NEG_INF if np.isneginf(m).any() else 0)
        if bad:
            flags[n] = bad
            continue
        order = np.lexsort((ar, -m.astype(np.float64)))[:topk][::-1]      # primary key: value descending, then index ascending
        idx[n], vals[n], minv[n] = order, m[order], m.min()
        flags[n] = 0 if (m != 0).any() else TOPK_ALL_ZERO
    return vals, idx, minv, flags


def heatmap_coords(maps, topk=5):
    """img2coord (jhmdb_dataset.py:118-136) with the defined tie order: maps [T][K][H][W] -> float64 [2][K][T]"""
    maps = np.asarray(maps, np.float32)
    T, K, H, W = maps.shape
    vals, idx, minv, flags = heatmap_topk(maps.reshape(T * K, H * W), topk)
    if (flags & (TOPK_NAN | TOPK_NEG_INF)).any() or (minv < 0).any():
        raise ValueError('NaN or negative value in a map')
    vals, idx, flags = vals.reshape(T, K, topk), idx.reshape(T, K, topk), flags.reshape(T, K)
    coords = np.zeros((2, K, T), dtype=float)
    with np.errstate(invalid='ignore', divide='ignore'):
        w = vals / np.sum(vals, keepdims=True, axis=-1)
    coords[0] = np.sum((idx % W) * w, axis=-1).T
    coords[1] = np.sum((idx // W) * w, axis=-1).T
    coords[:, (flags == TOPK_ALL_ZERO).T] = -1
    return coords


# ---- vfs_label_counts ---------------------------------------------------------------------------------------------------
def label_counts(pred, gt, num_classes, ignore_index=255):
    """int64 [num_classes][3] = intersect, prediction area, label area of intersect_and_union (iou.py:51-60)"""
    pred, gt = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(gt).reshape(-1).astype(np.int64)
    if ignore_index is not None and ignore_index >= 0:
        keep = gt != ignore_index
        pred, gt = pred[keep], gt[keep]

    def hist(v):      # np.histogram(v, bins=np.arange(num_classes + 1)): the last bin is closed
        v = v[v <= num_classes]
        return np.bincount(np.minimum(v, num_classes - 1), minlength=num_classes)

    return np.stack([hist(pred[pred == gt]), hist(pred), hist(gt)], axis=1).astype(np.int64)


def metrics_from_counts(counts):
    counts = np.asarray(counts)
    i, p, l = (counts[:, c].astype(float) for c in range(3))
    u = p + l - i
    with np.errstate(invalid='ignore', divide='ignore'):
        return i.sum() / l.sum(), i / l, i / u


def vip_summary(ret_metrics):
    """vip_dataset.py:119-147"""
    rounded = [np.round(m * 100, 2) for m in ret_metrics]
    with np.errstate(invalid='ignore'):
        mean = [np.round(np.nanmean(m) * 100, 2) for m in ret_metrics]
    return {'mIoU': mean[2] / 100.0, 'mAcc': mean[1] / 100.0, 'aAcc': mean[0] / 100.0}, {'IoU': rounded[2], 'Acc': rounded[1]}


def vip_evaluate(results, gts, num_classes=20, ignore_index=255):
    counts = np.zeros((num_classes, 3), np.int64)
    for res, gt in zip(results, gts):
        counts += label_counts(np.asarray(res).astype(np.uint8), gt, num_classes, ignore_index)
    summary, per_class = vip_summary(metrics_from_counts(counts))
    return summary, per_class, counts


# ---- PCK ----------------------------------------------------------------------------------------------------------------
def compute_pck(dist_all, thresh):
    out = np.zeros((len(dist_all), ))
    for p in range(len(dist_all)):
        out[p] = 100.0 * len(np.argwhere(dist_all[p] <= thresh)) / len(dist_all[p])
    return out


def pck_from_poses(preds, gts):
    dist_all = [np.zeros((0, 0)) for _ in range(NUM_KEYPOINTS)]
    for pred, gt in zip(preds, gts):
        vis = pred[0] > 0
        hi, lo = gt.copy(), gt.copy()
        hi[:, ~vis] = -1
        lo[:, ~vis] = 1e6
        boxes = np.stack((hi[0].max(axis=0) - lo[0].min(axis=0), hi[1].max(axis=0) - lo[1].min(axis=0)), axis=0)
        boxes = 0.6 * np.linalg.norm(boxes, axis=0)
        for f in range(pred.shape[-1]):
            for t in range(NUM_KEYPOINTS):
                if vis[t, f]:
                    dist = np.linalg.norm(np.subtract([pred[0, t, f], pred[1, t, f]], [gt[0, t, f], gt[1, t, f]])) / boxes[f]
                    dist_all[t] = np.append(dist_all[t], [[dist]])
    return {f'PCK@{a}': np.mean(compute_pck(dist_all, a)) for a in PCK_RANGES}


def pck_evaluate(results, gt_poses, topk=5):
    preds, gts = [], []
    for res, gt in zip(results, gt_poses):
        gt = np.asarray(gt, np.float64)
        n = min(len(res), gt.shape[-1])
        preds.append(heatmap_coords(np.asarray(res)[:n], topk))
        gts.append(gt[..., :n])
    return pck_from_poses(preds, gts)
