"""Shared model builder of tests/test_grad_clip.py, and - run as a script - one data-parallel rank on the CPU (gloo) that takes
clipped steps of the fused train step through the fiber emulator.  Usage: grad_clip_worker.py OUT.npz (env RANK/WORLD_SIZE/...)"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHALLOW_MINE = dict(num_stages=2, strides=(1, 2), out_indices=(1,), dilations=(1, 1))
SHALLOW_HEAD = dict(in_channels=128, projection_mid_channels=128, projection_out_channels=128,
                    predictor_mid_channels=64, predictor_out_channels=128)


def shallow_r18(dev, optimizer_config=None, **backbone):
    """the one-block-per-stage ResNet-18 tracker with seeded weights, and its optimizer -> (model, optimizer, cfg)"""
    import vfs_amd
    cfg = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', 'vfs_r18.py'))
    mcfg = dict(cfg.model)
    mcfg['backbone'] = dict(mcfg['backbone'], **SHALLOW_MINE, **backbone)
    mcfg['img_head'] = dict(mcfg['img_head'], **SHALLOW_HEAD)
    torch.manual_seed(0)
    model = vfs_amd.build_model(mcfg, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(dev).train()
    if optimizer_config is None:
        return model, vfs_amd.build_optimizer(model, cfg.optimizer), cfg
    return model, vfs_amd.build_optimizer(model, cfg.optimizer, optimizer_config=optimizer_config), cfg


def run(rank, world, out_path):
    from oracle import vfs_oracle as O
    from tests.emu_util import emu_lib
    from vfs_amd import engine
    torch.set_num_threads(2)
    eng = engine.Engine(lib=emu_lib())
    engine.set_shared_engine(eng)
    model, opt, _ = shallow_r18(torch.device('cpu'), dict(grad_clip=dict(max_norm=float(os.environ['VFS_TEST_MAX_NORM']))))
    imgs = O.fill_tensor([4 * world, 2, 3, 1, 32, 32], seed=11, scale=2.0)
    local = imgs[rank * 4:(rank + 1) * 4]
    norms = []
    for step in range(2):
        batch = (local * (1.0 + 0.25 * step)).contiguous()
        out = model.train_step(dict(imgs=batch, label=torch.zeros(4, 1)), None)
        opt.zero_grad()
        out['loss'].backward()
        opt.step()
        norms.append(opt.last_grad_norm())
    res = {'norms': np.array(norms, np.float32)}
    for n, p in model.named_parameters():
        res['param/' + n] = p.detach().numpy().copy()
    np.savez(out_path, **res)


if __name__ == '__main__':
    import torch.distributed as dist
    rank, world = int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        dist.init_process_group('gloo', rank=rank, world_size=world)
    run(rank, world, sys.argv[1])
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
