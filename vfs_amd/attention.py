"""masked_attention (mmaction/models/common/local_attention.py:161-234) as a differentiable operator on the HIP kernels of
csrc/attn_train.hip: the local top-k attention of the reconstruction / propagation losses of correspondence learning, for a
loss written on top of the module-level autograd path (autograd.py):

    x_q, x_k = backbone(frame_q), backbone(frame_k)                         # fp32 [N, C, h, w], train mode
    rec = vfs_amd.masked_attention(x_q, x_k, value, neighbor_range=12, temperature=0.07, topk=10)
    F.mse_loss(rec, target).backward()

The reference takes a mask tensor; here the mask is `spatial_neighbor(..., neighbor_range, mode='circle')`
(affinity_utils.py:144-156) and is never built: key (y', x') is in the window of query (y, x) iff
(y - y')^2 + (x - x')^2 < (neighbor_range // 2)^2, in every key frame; neighbor_range=None is no window.  The forward keeps, per
query, the topk selected key indices and their softmax weights; the backward wrt query, key and value runs from those
(include/vfs_hip.h, vfs_masked_attention_*).  No [T*HW, HW] affinity exists at any point, and the backward has no atomics: it is
bit-identical from run to run.

Limits of the kernels (refused by name, before any launch): 1 <= topk <= 10 (topk=None is not served), neighbor_range >= 2 or
None, C % 64 == 0 and C <= 2048, 1 <= T <= 64, 1 <= CO <= 256, T*H*W < 2^31, fp32 tensors on the GPU."""
import os

import torch

from . import build
from .engine import shared_engine

MAX_TOPK, MAX_C, MAX_T, MAX_CO = 10, 2048, 64, 256


def _check(query, key, value, neighbor_range, temperature, topk):
    who = 'masked_attention'
    if topk is None:
        raise NotImplementedError(f'{who}: topk=None (softmax over every in-window key) is not served by the kernels; 1 <= topk <= {MAX_TOPK}')
    if int(topk) != topk or not 1 <= topk <= MAX_TOPK:
        raise NotImplementedError(f'{who}: 1 <= topk <= {MAX_TOPK} (got {topk})')
    if neighbor_range is not None and (int(neighbor_range) != neighbor_range or neighbor_range < 2):
        raise ValueError(f'{who}: neighbor_range >= 2 or None (got {neighbor_range}): a radius of neighbor_range // 2 = 0 leaves no key in the window')
    if not temperature > 0 or temperature == float('inf'):
        raise ValueError(f'{who}: temperature must be positive and finite (got {temperature})')
    if query.dim() != 4 or key.dim() not in (4, 5) or value.dim() != key.dim():
        raise ValueError(f'{who}: query [N, C, H, W], key [N, C, T, H, W] or [N, C, H, W], value like key with CO channels; got '
                         f'{tuple(query.shape)}, {tuple(key.shape)}, {tuple(value.shape)}')
    N, C, H, W = query.shape
    T = key.shape[2] if key.dim() == 5 else 1
    CO = value.shape[1]
    if key.shape[0] != N or value.shape[0] != N or key.shape[1] != C or tuple(key.shape[-2:]) != (H, W) or tuple(value.shape[2:]) != tuple(key.shape[2:]):
        raise ValueError(f'{who}: shapes do not agree: query {tuple(query.shape)}, key {tuple(key.shape)}, value {tuple(value.shape)}')
    if C % 64 or C > MAX_C:
        raise NotImplementedError(f'{who}: C % 64 == 0 and C <= {MAX_C} (got C = {C})')
    if not 1 <= T <= MAX_T:
        raise NotImplementedError(f'{who}: 1 <= T <= {MAX_T} key frames (got T = {T})')
    if not 1 <= CO <= MAX_CO:
        raise NotImplementedError(f'{who}: 1 <= CO <= {MAX_CO} value channels (got CO = {CO})')
    if N < 1 or H < 1 or W < 1 or N > 65535:
        raise ValueError(f'{who}: empty operand or N > 65535: query {tuple(query.shape)}')
    if T * H * W >= 2 ** 31:
        raise NotImplementedError(f'{who}: T*H*W < 2^31 (got {T * H * W})')
    for name, t in (('query', query), ('key', key), ('value', value)):
        if t.dtype != torch.float32:
            raise TypeError(f'{who}: {name} is {t.dtype}; the kernels take fp32 (what the grad-mode ResNet.forward returns)')
    if not (query.device == key.device == value.device):
        raise ValueError(f'{who}: operands on different devices')
    return N, C, T, H, W, CO


def _check_device(query, lib):
    """the product library launches on the GPU; only the host build of the same sources (the tests' emulator) takes host memory"""
    if query.device.type != 'cuda' and os.path.basename(getattr(lib, 'path', '')) != os.path.basename(build.EMU_LIB):
        raise RuntimeError(f'masked_attention: {query.device.type} tensors; the operator runs on the HIP kernels only (there is no CPU path): '
                           'move query, key and value to the GPU')


def attention_forward(lib, stream, query, key, value, shape, neighbor_range, temperature, topk, normalize):
    """the forward launch on contiguous fp32 operands -> out [N, CO, H, W], idx int32 [N, topk, H*W] (-1: weight-0 fill),
    weights [N, topk, H*W], invq [N, H*W], invk [N, T*H*W] (None without normalize)"""
    N, C, T, H, W, CO = shape
    dev = query.device
    out = torch.empty(N, CO, H, W, dtype=torch.float32, device=dev)
    idx = torch.empty(N, topk, H * W, dtype=torch.int32, device=dev)
    w = torch.empty(N, topk, H * W, dtype=torch.float32, device=dev)
    invq = torch.empty(N, H * W, dtype=torch.float32, device=dev) if normalize else None
    invk = torch.empty(N, T * H * W, dtype=torch.float32, device=dev) if normalize else None
    lib.masked_attention_fwd(query, key, value, out, idx, w, invq, invk, N, C, T, H, W, CO, int(neighbor_range or 0), int(topk),
                             float(temperature), int(bool(normalize)), stream)
    return out, idx, w, invq, invk


class _MaskedAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, query, key, value, neighbor_range, temperature, topk, normalize):
        shape = _check(query, key, value, neighbor_range, temperature, topk)
        eng = shared_engine(query.device)
        _check_device(query, eng.lib)
        q, k, v = query.detach().contiguous(), key.detach().contiguous(), value.detach().contiguous()
        out, idx, w, invq, invk = attention_forward(eng.lib, eng.stream(q.device), q, k, v, shape, neighbor_range, temperature, topk, normalize)
        ctx.save_for_backward(q, k, v, idx, w, invq, invk)
        ctx.cfg = (shape, int(neighbor_range or 0), float(temperature), int(topk), bool(normalize), key.shape, value.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, idx, w, invq, invk = ctx.saved_tensors
        (N, C, T, H, W, CO), nr, temperature, topk, normalize, kshape, vshape = ctx.cfg
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        eng = shared_engine(q.device)
        lib, dev = eng.lib, q.device
        dq = torch.empty_like(q) if need_q else None
        dk = torch.empty(kshape, dtype=torch.float32, device=dev) if need_k else None
        dv = torch.empty(vshape, dtype=torch.float32, device=dev) if need_v else None
        if need_q or need_k or need_v:
            nbytes = torch.zeros(1, dtype=torch.int64)
            eng.host_lib.masked_attention_workspace_bytes(N, C, T, H, W, CO, topk, int(normalize), nbytes)
            ws = eng.ws('ws.masked_attention', (int(nbytes) + 3) // 4, torch.float32, dev)
            lib.masked_attention_bwd(q, k, v, dout.detach().float().contiguous(), idx, w, invq, invk, dq, dk, dv, ws, ws.numel() * 4,
                                     N, C, T, H, W, CO, nr, topk, temperature, int(normalize), eng.stream(dev))
        return dq, dk, dv, None, None, None, None


def masked_attention(query, key, value, neighbor_range=None, temperature=1.0, topk=10, normalize=True):
    """local_attention.py:161-234 with mask = spatial_neighbor(neighbor_range, mode='circle').

    query [N, C, H, W]; key [N, C, T, H, W] or [N, C, H, W] (T = 1); value [N, CO, T, H, W] or [N, CO, H, W]; fp32, on the GPU
    -> [N, CO, H, W] fp32; gradients flow to whichever of query / key / value requires them (HIP backward, no atomics)."""
    return _MaskedAttentionFn.apply(query, key, value, neighbor_range, temperature, topk, normalize)
