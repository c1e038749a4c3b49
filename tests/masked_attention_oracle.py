"""A torch restatement of vfs_amd.masked_attention, written from the operator's formula (tests only; differentiable by torch
autograd, any dtype, any device).  It builds what the kernels never build - the [N, T*HW, HW] scores and the window mask - which
is fine at test sizes.

    score(i, j) = <k^_i, q^_j> / temperature      k^, q^: rows divided by max(||row||_2, 1e-12) when normalize
    window:       key (t, y', x') belongs to query (y, x) iff (y - y')^2 + (x - x')^2 < (neighbor_range // 2)^2
    per query:    the topk largest in-window scores, softmax over them, out_j = sum_a w_a value[:, i_a]
    fewer than topk in-window keys: the rest of the list has weight 0"""
import torch


def window(H, W, neighbor_range, device):
    """bool [HW keys, HW queries]"""
    pos = torch.arange(H * W, device=device)
    y, x = pos // W, pos % W
    if neighbor_range is None:
        return torch.ones(H * W, H * W, dtype=torch.bool, device=device)
    return ((y[:, None] - y[None]) ** 2 + (x[:, None] - x[None]) ** 2) < (neighbor_range // 2) ** 2


def masked_attention(query, key, value, neighbor_range=None, temperature=1.0, topk=10, normalize=True, return_selection=False):
    N, C, H, W = query.shape
    if key.dim() == 4:
        key, value = key[:, :, None], value[:, :, None]
    T, CO = key.shape[2], value.shape[1]
    q, k, v = query.reshape(N, C, H * W), key.reshape(N, C, T * H * W), value.reshape(N, CO, T * H * W)
    if normalize:
        q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
        k = k / k.norm(dim=1, keepdim=True).clamp_min(1e-12)
    s = torch.einsum('nci,ncj->nij', k, q) / temperature
    s = s.masked_fill(~window(H, W, neighbor_range, query.device).repeat(T, 1)[None], float('-inf'))
    kk = min(topk, T * H * W)
    top, idx = s.topk(kk, dim=1)      # [N, kk, HW]
    w = top.softmax(dim=1)            # exp(-inf) = 0: the fill
    picked = torch.gather(v[:, :, :, None].expand(N, CO, T * H * W, H * W), 2, idx[:, None].expand(N, CO, kk, H * W))
    out = (picked * w[:, None]).sum(dim=2).reshape(N, CO, H, W)
    if return_selection:
        return out, torch.where(torch.isinf(top), torch.full_like(idx, -1), idx), w
    return out
