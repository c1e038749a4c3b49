"""Golden vectors for the differentiable masked_attention (vfs_amd/attention.py, csrc/attn_train.hip), captured from the REAL
reference function (mmaction/models/common/local_attention.py:161-234) with mask = spatial_neighbor(..., mode='circle')
(affinity_utils.py:144-156) in the build container.

    python tests/golden/gen_masked_attention_grad_golden.py
        -> tests/golden/masked_attention_grad.npz        inputs, the reference's fp32 output and gradients, the selected keys,
                                                         the reference's own fp32-against-fp64 error per tensor
        -> tests/golden/masked_attention_grad_f64.npz    the fp64 evaluation, as the fp32 array `fp32 result - fp64 result`

Per case: query / key / value / dout, out and the gradients of <out, dout> wrt query / key / value by torch autograd on the CPU,
in fp32 and in fp64, and err/<tensor> = ||fp32 - fp64||_2 / ||fp64||_2.

Storage (a committed file stays below 1 MiB; case 4 alone is 105k input elements): the inputs are standard-normal draws
ROUNDED TO bf16-REPRESENTABLE fp32 values and stored as their upper 16 bits (`<name>_bf16bits`, expanded exactly by
`load_case`); the fp64 results are stored as diff = float32(fp32 result - fp64 result), so that fp64 = fp32 - diff to about
1e-14 relative (the difference is ~1e-7 of the value and keeps 24 bits of its own).

Two properties of the reference function that the generator works around:
  * it runs for N = 1 only: the mask is expanded to [T * HW, HW] and `reshape_as(affinity)` ([N, T * HW, HW], :202-204) raises
    for N > 1 (and the value gather of :218-220 indexes the flattened batch with per-sample key indices).  Attention is per
    sample by the function's own contract (:171-174), so the reference is evaluated ONE SAMPLE AT A TIME and the results are
    stacked: cases 1 and 4 check the batch stride of the kernels against two independent reference runs.
  * it has no `mask=None`: neighbor_range=None is evaluated with an all-true mask.

The gap condition: a seed is refused (the next one is tried) unless for EVERY query the fp64 gap between the k-th and the
(k+1)-th in-window score, before the division by the temperature, is at least 16 * C * 2^-24 * max||q|| * max||k|| (row norms
of the operands of the dot product: 1 after normalisation) - an fp32 dot product is within C * 2^-24 * ||q|| * ||k|| of the
exact one, so membership of the top-k cannot depend on the order of summation.  A query with at most k in-window keys selects
all of them: there is no (k+1)-th score and nothing to decide."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

CASES = [   # name, N, C, T (0: 4-D key / value), H, W, CO, neighbor_range, topk, temperature, normalize
    ('borders_two_frames', 2, 64, 2, 6, 7, 3, 5, 3, 0.07, True),
    ('unmasked_raw', 1, 128, 0, 9, 5, 5, None, 10, 1.0, False),
    ('fewer_than_topk', 1, 64, 2, 5, 5, 2, 2, 3, 1.0, True),
    ('odd_channels', 2, 192, 3, 8, 8, 17, 7, 10, 1.0, True),
]
TENSORS = ('out', 'dq', 'dk', 'dv')
MAIN, F64 = 'masked_attention_grad.npz', 'masked_attention_grad_f64.npz'


def bf16_bits(x):
    """fp32 tensor of bf16-representable values -> uint16 array of its upper halves"""
    u = x.contiguous().view(torch.int32).numpy().astype(np.uint32)
    assert not (u & 0xFFFF).any()
    return (u >> 16).astype(np.uint16)


def from_bf16_bits(a):
    return torch.from_numpy((a.astype(np.uint32) << 16).view(np.float32).copy())


def load_case(name, golden_dir=HERE):
    """-> dict: inputs (fp32 tensors), the reference's fp32 results, `<tensor>64` fp64 results, err/<tensor>, idx"""
    g, g64 = np.load(os.path.join(golden_dir, MAIN)), np.load(os.path.join(golden_dir, F64))
    d = {k: from_bf16_bits(g[f'{name}/{k}_bf16bits']) for k in ('query', 'key', 'value', 'dout')}
    for t in TENSORS:
        d[t] = torch.from_numpy(g[f'{name}/{t}'])
        d[t + '64'] = d[t].double() - torch.from_numpy(g64[f'{name}/{t}_diff']).double()
        d['err/' + t] = float(g[f'{name}/err/{t}'])
    d['idx'] = torch.from_numpy(g[f'{name}/idx'])
    return d


def _inputs(case, seed):
    _, N, C, T, H, W, CO, _, _, _, _ = case
    gen = torch.Generator().manual_seed(seed)
    tt = (T,) if T else ()
    shapes = dict(query=(N, C, H, W), key=(N, C) + tt + (H, W), value=(N, CO) + tt + (H, W), dout=(N, CO, H, W))
    return {k: torch.randn(s, generator=gen).to(torch.bfloat16).float() for k, s in shapes.items()}


def _mask(spatial_neighbor, H, W, nr, dtype):
    if nr is None:
        return torch.ones(H * W, H * W, dtype=torch.bool)
    return spatial_neighbor(1, H, W, nr, torch.device('cpu'), dtype, mode='circle')


def _selected(case, x):
    """the keys the reference selects, from the fp64 scores: int32 [N, HW, topk] ascending per query, -1 = the fill of a
    query with fewer than topk in-window keys; and whether the gap condition holds"""
    _, N, C, T, H, W, CO, nr, topk, temp, normalize = case
    q, k = x['query'].double(), x['key'].double()
    if normalize:
        q, k = torch.nn.functional.normalize(q, dim=1), torch.nn.functional.normalize(k, dim=1)
    q, k = q.reshape(N, C, H * W), k.reshape(N, C, -1)
    aff = torch.einsum('bci,bcj->bij', k, q)      # [N, THW, HW], before the temperature
    y, xx = torch.arange(H * W) // W, torch.arange(H * W) % W
    if nr is not None:
        inwin = ((y[:, None] - y[None]) ** 2 + (xx[:, None] - xx[None]) ** 2) < (nr // 2) ** 2
    else:
        inwin = torch.ones(H * W, H * W, dtype=torch.bool)
    inwin = inwin.repeat(max(T, 1), 1)[None].expand_as(aff)
    aff = aff.masked_fill(~inwin, float('-inf'))
    srt, order = aff.sort(dim=1, descending=True)
    need = 16 * C * 2.0 ** -24 * float(q.norm(dim=1).max()) * float(k.norm(dim=1).max())
    ok = True
    if srt.shape[1] > topk:
        kth, nxt = srt[:, topk - 1], srt[:, topk]
        decided = torch.isinf(nxt)      # at most topk in-window keys: all of them are selected
        ok = bool((decided | (kth - nxt >= need)).all())
    sel = order[:, :topk].clone()
    sel[torch.isinf(srt[:, :topk])] = -1
    sel = sel.permute(0, 2, 1).sort(dim=2).values      # [N, HW, topk]
    return sel.to(torch.int32), ok


def _reference(fn, mask, case, x, dtype):
    """out and the three gradients of <out, dout>, the reference evaluated one sample at a time"""
    _, N, _, _, _, _, _, _, topk, temp, normalize = case
    res = {t: [] for t in TENSORS}
    for n in range(N):
        q, k, v = (x[a][n:n + 1].to(dtype).clone().requires_grad_() for a in ('query', 'key', 'value'))
        out = fn(q, k, v, mask, temperature=temp, topk=topk, normalize=normalize)
        (out * x['dout'][n:n + 1].to(dtype)).sum().backward()
        for t, a in zip(TENSORS, (out.detach(), q.grad, k.grad, v.grad)):
            res[t].append(a)
    return {t: torch.cat(a) for t, a in res.items()}


def main():
    import gen_golden as G
    G.import_reference_hot_path()
    from mmaction.models.common.affinity_utils import spatial_neighbor
    from mmaction.models.common.local_attention import masked_attention
    main_npz, f64_npz = {}, {}
    for ci, case in enumerate(CASES):
        name, N, C, T, H, W, CO, nr, topk, temp, normalize = case
        for seed in range(1000 * (ci + 1), 1000 * (ci + 1) + 200):
            x = _inputs(case, seed)
            sel, ok = _selected(case, x)
            if ok:
                break
            print(f'{name}: seed {seed} refused (gap condition)')
        else:
            raise SystemExit(f'{name}: no seed meets the gap condition')
        mask = _mask(spatial_neighbor, H, W, nr, torch.float32)
        r32 = _reference(masked_attention, mask, case, x, torch.float32)
        r64 = _reference(masked_attention, mask, case, x, torch.float64)
        main_npz[f'{name}/seed'] = np.array(seed)
        main_npz[f'{name}/idx'] = sel.numpy()
        for a in ('query', 'key', 'value', 'dout'):
            main_npz[f'{name}/{a}_bf16bits'] = bf16_bits(x[a])
        line = []
        for t in TENSORS:
            main_npz[f'{name}/{t}'] = r32[t].numpy()
            f64_npz[f'{name}/{t}_diff'] = (r32[t].double() - r64[t]).float().numpy()
            err = float((r32[t].double() - r64[t]).norm() / r64[t].norm())
            main_npz[f'{name}/err/{t}'] = np.array(err)
            line.append(f'{t} {err:.3e}')
        print(f'{name}: seed {seed}, fp32 against fp64: ' + ', '.join(line))
    out_dir = os.environ.get('VFS_GOLDEN_OUT', HERE)
    np.savez_compressed(os.path.join(out_dir, MAIN), **main_npz)
    np.savez_compressed(os.path.join(out_dir, F64), **f64_npz)
    for f in (MAIN, F64):
        print(f, os.path.getsize(os.path.join(out_dir, f)), 'bytes')


if __name__ == '__main__':
    main()
