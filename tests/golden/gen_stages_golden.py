#!/usr/bin/env python3
"""Label maps of the REAL reference's `VanillaTracker.forward_test` over SEVERAL backbone stages in one run.

Runs only in the build container (imports the reference through the mmcv stand-in of gen_golden.py).  tools/test.py:130-131 sets the
backbone's out_indices / strides from the test-time config; with more than one entry `ResNet.forward` returns a tuple and
`VanillaTracker.forward_test` (trackers/vanilla_tracker.py:86-93, 199-205) propagates once per stage and stacks the label maps
[num_feats, T, H, W].  Every label map stored below is the output of the reference's own code on torch-CPU fp32:

  forward_test_r18_stages.npz   ResNet-18, filler weights (seed 5), the clip and first-frame map of forward_test_r18_all_blocks.npz
                                (6 frames of 96 x 128), out_indices (0, 1, 2), strides (1, 2, 1, 1): stage 0 at stride 4 with 64
                                channels (24 x 32), stages 1 and 2 at stride 8 with 128 / 256 channels (12 x 16); neighbor_range 8,
                                precede_frames 3.  original_shape (90, 120) differs from the map's 96 x 128: stages 1 and 2 resize the
                                first-frame map from the map already resized to 90 x 120 (vanilla_tracker.py:101-104 overwrites
                                ref_seg_map inside the level loop).

The clip is a closed-form fill (oracle/vfs_oracle.py fill_tensor): the fixture stores its shape, seed and scale and a strided
sample of it instead of its 884 KB, next to the first-frame map, the config and the label maps.

Usage:  python tests/golden/gen_stages_golden.py
"""
import os
import runpy
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402
from oracle.vfs_oracle import fill_state_dict_, fill_tensor  # noqa: E402

IMGS = dict(shape=[1, 1, 3, 6, 96, 128], seed=41, scale=2.0)
ORIGINAL_SHAPE = (90, 120, 3)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    builder, trackers, common = GG.import_reference_hot_path()
    cfg = runpy.run_path(os.path.join(GG.REF, 'configs', 'r18_nc_sgd_cos_100e_r2_1xNx8_k400.py'))
    tc = GG.AttrDict(cfg['test_cfg'])
    tc.update(neighbor_range=8, precede_frames=3, out_indices=(0, 1, 2), strides=(1, 2, 1, 1))
    bb = dict(cfg['model']['backbone'])
    bb['out_indices'], bb['strides'] = tc['out_indices'], tc['strides']       # tools/test.py:129-133
    model = builder.build_model(dict(type='VanillaTracker', backbone=bb), train_cfg=None, test_cfg=tc)
    fill_state_dict_(model, seed=5)
    model.eval()
    imgs = fill_tensor(IMGS['shape'], IMGS['seed'], scale=IMGS['scale'])
    seg = np.load(os.path.join(HERE, 'forward_test_r18_all_blocks.npz'))['ref_seg']
    with torch.no_grad():
        res = model(imgs, return_loss=False, ref_seg_map=torch.from_numpy(seg)[None], img_meta=[dict(original_shape=ORIGINAL_SHAPE)])
    maps = res[0].astype(np.uint8)
    assert maps.shape == (3, IMGS['shape'][3]) + ORIGINAL_SHAPE[:2], maps.shape
    out = os.path.join(os.environ.get('VFS_GOLDEN_OUT', HERE), 'forward_test_r18_stages.npz')
    np.savez_compressed(out, seg_preds=maps, ref_seg=seg, original_shape=np.array(ORIGINAL_SHAPE),
                        imgs_shape=np.array(IMGS['shape']), imgs_seed=np.array(IMGS['seed']), imgs_scale=np.array(IMGS['scale']),
                        imgs_sample=imgs.flatten()[::997].numpy().copy(),
                        test_cfg=np.array(repr({k: tc[k] for k in sorted(tc) if k != 'output_dir'})))
    print('wrote', out, maps.shape, [np.bincount(m[-1].ravel(), minlength=3).tolist() for m in maps])


if __name__ == '__main__':
    main()
