"""Golden vectors of DenseSimSiamHead, captured from the REAL reference class (mmaction/models/heads/sim_siam_head.py:177-284)
in the build container.

    python tests/golden/gen_dense_head_golden.py        -> tests/golden/dense_head.npz

Two heads, train mode, weights from fill_state_dict_(seed 21), inputs two fill_tensor(shape, 31 / 32, scale 1.5):
  (no prefix) in_channels 40, projection 48 / 72, predictor 24 / 72, inputs [4,40,3,5]: odd channel counts, for the state_dict
              contract and the CPU helper;
  k64/        in_channels 64, projection 64 / 128, predictor 64 / 128, inputs [4,64,3,5]: channel counts the 1x1 convolution
              kernels take, for the HIP head.
Stored per head: the state_dict keys, z and p of both inputs, head.loss(p1, z1, p2, z2)['loss_feat'], the gradients of its mean wrt
every parameter and both inputs, and (captured first, from the filled running statistics) z and p of input 1 in eval mode."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G      # noqa: E402
from gen_golden import fill_state_dict_, fill_tensor      # noqa: E402

HEAD = dict(in_channels=40, projection_mid_channels=48, projection_out_channels=72, predictor_mid_channels=24,
            predictor_out_channels=72)
SHAPE = [4, 40, 3, 5]
HEAD64 = dict(in_channels=64, projection_mid_channels=64, projection_out_channels=128, predictor_mid_channels=64,
              predictor_out_channels=128)
SHAPE64 = [4, 64, 3, 5]


def capture(cls, kw, shape, prefix, res):
    import torch
    head = cls(**kw)
    fill_state_dict_(head, seed=21)
    x1 = fill_tensor(shape, 31, scale=1.5).requires_grad_(True)
    x2 = fill_tensor(shape, 32, scale=1.5).requires_grad_(True)
    head.eval()
    with torch.no_grad():
        ze, pe = head(x1)
    head.train()
    z1, p1 = head(x1)
    z2, p2 = head(x2)
    loss = head.loss(p1, z1, p2, z2)['loss_feat']
    loss.mean().backward()
    out = dict(keys=np.array(list(head.state_dict().keys())), z1=z1.detach().numpy(), p1=p1.detach().numpy(), z2=z2.detach().numpy(),
               p2=p2.detach().numpy(), loss=loss.detach().numpy(), dx1=x1.grad.numpy(), dx2=x2.grad.numpy(), z1_eval=ze.numpy(),
               p1_eval=pe.numpy())
    for n, p in head.named_parameters():
        out['grad/' + n] = p.grad.numpy()
    print(prefix or '-', loss.detach().numpy())
    res.update({prefix + k: v for k, v in out.items()})


def main():
    G.import_reference_hot_path()
    from mmaction.models.heads.sim_siam_head import DenseSimSiamHead
    res = {}
    capture(DenseSimSiamHead, HEAD, SHAPE, '', res)
    capture(DenseSimSiamHead, HEAD64, SHAPE64, 'k64/', res)
    np.savez_compressed(os.path.join(os.environ.get('VFS_GOLDEN_OUT', HERE), 'dense_head.npz'), **res)


if __name__ == '__main__':
    main()
