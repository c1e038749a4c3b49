"""The per-position cosine loss of DenseSimSiamHead (csrc/simloss_dense.hip) through the C ABI, against torch fp32 on the same
bf16-rounded operands: oracle.vfs_oracle.cosine_sim_loss_general on [N,C,S] views inside the roll loop of the tracker.
backend=emu: fiber emulator on the CPU; backend=gpu: libvfs_hip.so on the MI355X."""
import pytest
import torch

from oracle import vfs_oracle as O
from tests.emu_util import rb, relerr

BF16 = torch.bfloat16

# N, S, C, T, K: S odd and smaller than the 4 * (64 / 16) positions a workgroup holds, C no multiple of 64 (9 chunks on 16 lanes);
# the same without rolls (K = 1 of T = 3) and without videos; the channel limit (4 chunks per lane); one position
SHAPES = [(6, 15, 72, 3, 3), (6, 15, 72, 3, 1), (6, 15, 72, 1, 1), (2, 2, 2048, 1, 1), (4, 1, 64, 2, 2)]


def _operands(N, S, C, seed):
    g = torch.Generator().manual_seed(seed)
    p1, z1, p2, z2 = (rb(torch.randn(N, S, C, generator=g)) for _ in range(4))
    z2[N - 1, S - 1] = 0      # a zero z position on either side: the eps clamp of the normalisation
    z1[0, 0] = 0
    gl = torch.randn(8, N, generator=g)
    return p1, z1, p2, z2, gl


def _reference(p1, z1, p2, z2, T, K, negative, w):
    """loss rows [K][N] of the reference composition; operands [N,S,C] fp32, p1 / p2 may require grad"""
    def ncs(t):
        return t.permute(0, 2, 1)

    def half(p, z):
        return O.cosine_sim_loss_general(ncs(p), ncs(z).detach(), negative=negative)

    def head_loss(pa, za, pb, zb):
        return (half(pa, zb) * 0.5 + half(pb, za) * 0.5) * w
    rows = [head_loss(p1, z1, p2, z2)]
    if K > 1:
        z2v, p2v = O.images2video(ncs(z2), T), O.images2video(ncs(p2), T)
        for i in range(1, T):
            p2r, z2r = O.video2images(p2v.roll(i, dims=2)), O.video2images(z2v.roll(i, dims=2))
            rows.append(head_loss(p1, z1, p2r.permute(0, 2, 1), z2r.permute(0, 2, 1)))
    return torch.stack(rows)


def _workspace(lib, N, S, C, K):
    n = torch.zeros(1, dtype=torch.int64)
    lib.dense_cosine_loss_workspace_bytes(N, S, C, K, n)
    assert n.item() >= K * N * 2 * 4 and n.item() % 8 == 0
    return torch.zeros(n.item() // 4), n.item()


def _run(backend, ops, N, S, C, T, K, negative, w):
    lib = backend.hostlib
    p1, z1, p2, z2, gl = ops
    args = [t.to(BF16) for t in (p1, z1, p2, z2)]
    ws, nbytes = _workspace(backend.lib, N, S, C, K)
    loss = torch.empty(K, N)
    lib.dense_cosine_loss_fwd(*args, loss, ws, nbytes, N, S, C, T, K, int(negative), w, None)
    dp1, dp2 = torch.empty(N, S, C, dtype=BF16), torch.empty(N, S, C, dtype=BF16)
    lib.dense_cosine_loss_bwd(*args, gl[:K].contiguous(), dp1, dp2, N, S, C, T, K, int(negative), w, None)
    return loss, dp1, dp2


@pytest.mark.parametrize('negative', [False, True])
@pytest.mark.parametrize('N,S,C,T,K', SHAPES)
def test_dense_cosine_loss_matches_torch(backend, N, S, C, T, K, negative):
    ops = _operands(N, S, C, seed=7)
    p1, z1, p2, z2, gl = ops
    w = 1.0 / T if K > 1 else 1.0
    loss, dp1, dp2 = _run(backend, ops, N, S, C, T, K, negative, w)
    p1r, p2r = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    ref = _reference(p1r, z1, p2r, z2, T, K, negative, w)
    e_loss = relerr(loss, ref.detach())
    (ref * gl[:K]).sum().backward()
    e1, e2 = relerr(dp1.float(), p1r.grad), relerr(dp2.float(), p2r.grad)
    print(f'loss {e_loss:.3g} dp1 {e1:.3g} dp2 {e2:.3g}')
    assert e_loss < 1e-5
    assert e1 < 6e-3 and e2 < 6e-3      # bf16 storage of the result
    if S == 1:      # one position: the frame-level loss on the same rows
        flat = [t.to(BF16).reshape(N, C) for t in (p1, z1, p2, z2)]
        frame = torch.empty(K, N)
        backend.hostlib.cosine_loss_fwd(*flat, frame, N, C, T, K, int(negative), w, None)
        assert relerr(loss, frame) < 1e-6
    # no atomics, fixed summation order: the same bits again
    loss2, dp1b, dp2b = _run(backend, ops, N, S, C, T, K, negative, w)
    assert torch.equal(loss, loss2) and torch.equal(dp1, dp1b) and torch.equal(dp2, dp2b)


SHAPE, ARG = -1, -3


def _argument_error_cases():
    P = torch.zeros(16384)
    cases = []
    for who in ('dense_cosine_loss_fwd', 'dense_cosine_loss_bwd'):
        def args(N=6, S=15, C=72, T=3, K=3, p1=P, ws=P, nbytes=1 << 16, who=who):
            head = (p1, P, P, P, P, ws, nbytes) if who.endswith('fwd') else (p1, P, P, P, P, P, P)
            return head + (N, S, C, T, K, 0, 1.0, None)
        for cid, kw, code, msg in (('N%T', dict(N=7), SHAPE, 'N % T'), ('T0', dict(T=0), SHAPE, 'N % T'),
                                   ('K0', dict(K=0), SHAPE, '1 <= K <= T'), ('K>T', dict(K=4), SHAPE, '1 <= K <= T'),
                                   ('S0', dict(S=0), SHAPE, 'S >= 1'), ('C%8', dict(C=76), SHAPE, 'C % 8'),
                                   ('C0', dict(C=0), SHAPE, 'C % 8'), ('C2056', dict(C=2056), SHAPE, 'C > 2048'),
                                   ('null', dict(p1=None), ARG, 'null or unaligned operand (16 bytes)')):
            cases.append(pytest.param(who, args(**kw), code, f'{who}: {msg}', id=f'{who}-{cid}'))
    short = 'dense_cosine_loss_fwd: workspace smaller than vfs_dense_cosine_loss_workspace_bytes(N, S, C, K)'
    need = 3 * 6 * 1 * 2 * 4      # K * N * Z * 2 floats: 15 positions of 72 channels are one unit of 16
    cases.append(pytest.param('dense_cosine_loss_fwd', (P, P, P, P, P, P, need - 1, 6, 15, 72, 3, 3, 0, 1.0, None), ARG, short, id='fwd-short-workspace'))
    cases.append(pytest.param('dense_cosine_loss_fwd', (P, P, P, P, P, None, need, 6, 15, 72, 3, 3, 0, 1.0, None), ARG, short, id='fwd-null-workspace'))
    cases.append(pytest.param('dense_cosine_loss_bwd', (P, P, P, P, P, None, P, 6, 15, 72, 3, 3, 0, 1.0, None), ARG,
                              'dense_cosine_loss_bwd: null or unaligned gradient buffer', id='bwd-null-gradient'))
    return cases


@pytest.mark.parametrize('name,args,code,message', _argument_error_cases())
def test_dense_cosine_loss_argument_errors(name, args, code, message):
    """return code and vfs_last_error() text of every argument check; each returns before anything is launched (P is a host buffer)"""
    from tests.emu_util import emu_lib
    lib = emu_lib()
    fn = lib.cfunc(name)
    assert len(args) == len(lib.protos['vfs_' + name][1]), 'the case does not match the prototype'
    rc = fn(*[a.data_ptr() if hasattr(a, 'data_ptr') else a for a in args])
    assert (rc, lib.last_error()) == (code, message)


def test_dense_cosine_loss_workspace_query_is_host_only():
    from tests.emu_util import emu_lib
    from vfs_amd import _lib
    lib = emu_lib()
    n = torch.zeros(1, dtype=torch.int64)
    lib.dense_cosine_loss_workspace_bytes(6, 15, 72, 3, n)
    assert n.item() == 3 * 6 * 1 * 2 * 4
    lib.dense_cosine_loss_workspace_bytes(4, 49, 512, 2, n)      # 64 lanes per position: 13 units of 4 positions
    assert n.item() == 2 * 4 * 13 * 2 * 4
    lib.dense_cosine_loss_workspace_bytes(4, 4096, 512, 2, n)     # capped at 32 workgroups per (image, roll)
    assert n.item() == 2 * 4 * 32 * 2 * 4
    with pytest.raises(_lib.VfsError, match='dense_cosine_loss_workspace_bytes'):
        lib.dense_cosine_loss_workspace_bytes(4, 49, 513, 2, n)
    with pytest.raises(_lib.VfsError):
        lib.dense_cosine_loss_workspace_bytes(4, 49, 512, 2, None)
