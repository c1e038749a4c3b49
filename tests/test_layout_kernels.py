"""The layout kernels of the module-level autograd boundary (csrc/layout.hip), bit for bit against the torch passes they replace:
vfs_nhwc_bf16_to_nchw_f32 == x.float().permute(0, 3, 1, 2).contiguous(), vfs_nchw_f32_to_nhwc_bf16 ==
g.permute(0, 2, 3, 1).contiguous().to(bf16), vfs_nchw_f32_add_nhwc_bf16 == (acc.float() + g.permute(0, 2, 3, 1)).to(bf16) (one
rounding), vfs_bf16_add == (a.float() + b.float()).to(bf16).  Emulator and GPU run the same bodies."""
import pytest
import torch

BF16 = torch.bfloat16
TILE = 64      # pixels of a workgroup's tile (csrc/layout_host.h VFS_LAYOUT_TILE)
SHAPES = [(1, 1, 64), (3, 35, 64), (2, 7 * 9, 192), (2, 16 * 16, 512), (1, 33, 2048),
          (2, TILE + 1, 64), (1, 2 * TILE + 1, 128),      # HW one more than a multiple of the tile
          (5, 1, 192), (3, 1, 2048)]      # HW == 1 (the heads' [N, C] tensors): the plain-cast path, more than one workgroup
SHAPE_ERR = -1


def _f32(bits):
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)


def _special_f32():
    """fp32 values around the bf16 rounding: exactly halfway between neighbouring bf16 values (lower neighbour even and odd), one
    fp32 step either side of halfway, +-0, the largest finite bf16, the halfway point above it (rounds to Inf), +-Inf, NaN"""
    bits = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0x4048, 0x0001, 0x0080, 0x7F7E):
        for lo in (0x8000, 0x7FFF, 0x8001, 0x0001, 0xFFFF):
            bits += [(hi << 16) | lo, 0x80000000 | (hi << 16) | lo]
    bits += [0x00000000, 0x80000000, 0x7F7F0000, 0xFF7F0000, 0x7F7F8000, 0x7F7F7FFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001]
    return _f32(bits)


def _scatter(t, vals, seed):
    """vals at distinct random positions of t (every tile gets some when t is small; all of them always land)"""
    flat = t.view(-1)
    n = min(vals.numel(), flat.numel())
    idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(seed))[:n]
    flat[idx] = vals[:n]
    return t


def _same_bits(got, want, what):
    """torch.equal on the bits; NaNs compared as NaNs (their payload is the converter's business)"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f'{what}: NaN positions differ'
    view = torch.int16 if got.dtype == BF16 else torch.int32
    assert torch.equal(torch.where(gn, torch.zeros_like(got), got).view(view), torch.where(wn, torch.zeros_like(want), want).view(view)), what


def _src_f32(N, HW, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, HW, generator=g) * torch.tensor(2.0).pow(torch.randint(-12, 12, (N, C, 1), generator=g).float())
    return _scatter(x, _special_f32(), seed + 1)


@pytest.mark.parametrize('N,HW,C', SHAPES)
def test_nhwc_bf16_to_nchw_f32(backend, N, HW, C):
    g = torch.Generator().manual_seed(HW + C)
    bits = torch.randint(-32768, 32768, (N, HW, C), generator=g).to(torch.int16)      # every bf16 pattern class: NaN, Inf, subnormals, -0
    special = torch.tensor([0x7F80, 0xFF80, 0x7FC0, 0xFF81, 0x0000, 0x8000, 0x7F7F, 0x0001], dtype=torch.int32).to(torch.int16)
    src = _scatter(bits, special, HW).view(BF16)
    dst = torch.full((N, C, HW), float('nan'))
    backend.hostlib.nhwc_bf16_to_nchw_f32(src, dst, N, HW, C, None)
    _same_bits(dst, src.float().permute(0, 2, 1).contiguous(), 'nhwc_bf16_to_nchw_f32')
    assert torch.isnan(dst).any() and torch.isinf(dst).any()


@pytest.mark.parametrize('N,HW,C', SHAPES)
def test_nchw_f32_to_nhwc_bf16(backend, N, HW, C):
    src = _src_f32(N, HW, C, 7 * HW + C)
    dst = torch.full((N, HW, C), float('nan'), dtype=BF16)
    backend.hostlib.nchw_f32_to_nhwc_bf16(src, dst, N, HW, C, None)
    want = src.permute(0, 2, 1).contiguous().to(BF16)
    _same_bits(dst, want, 'nchw_f32_to_nhwc_bf16')
    if src.numel() >= 128:
        assert torch.isnan(want).any() and torch.isinf(want).any() and (want.float() != src.permute(0, 2, 1)).any()


def _join_operands(N, HW, C, seed):
    """acc (bf16 NHWC) and src (fp32 NCHW) whose fp32 sums sit on and around the rounding boundaries: sums exactly halfway (even
    and odd lower neighbour), cases where rounding src first and the sum second gives another result than one rounding, +-0 sums,
    overflow to Inf, Inf - Inf = NaN, NaN operands - scattered over random operands"""
    g = torch.Generator().manual_seed(seed)
    acc = (torch.randn(N, HW, C, generator=g) * 4).to(BF16)
    src = torch.randn(N, C, HW, generator=g) * 4
    e = 2.0 ** -8      # half a bf16 step at 1.0
    pairs = [(1.0, e), (1.0 + 2 * e, e), (1.0, e + 2.0 ** -17), (1.0 + 2 * e, e - 2.0 ** -17), (1.0, e - 2.0 ** -17), (-1.0, -e), (-1.0 - 2 * e, -e),
             (2.0, -2 * e), (0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (1.0, -1.0), (-0.0, 0.0), (3.3895313892515355e+38, 3.3895313892515355e+38),
             (float('inf'), 1.0), (float('inf'), float('-inf')), (float('nan'), 1.0), (1.0, float('nan')), (1.0, float('inf')),
             (3.3895313892515355e+38, 2.0 ** 119), (3.3895313892515355e+38, 2.0 ** 119 - 2.0 ** 96)]
    n = min(len(pairs), N * HW * C)
    idx = torch.randperm(N * HW * C, generator=g)[:n]
    for (a, s), i in zip(pairs, idx.tolist()):
        nn_, rest = divmod(i, HW * C)
        hw, c = divmod(rest, C)
        acc[nn_, hw, c] = a
        src[nn_, c, hw] = s
    return acc, src


@pytest.mark.parametrize('inplace', [False, True])
@pytest.mark.parametrize('N,HW,C', SHAPES)
def test_nchw_f32_add_nhwc_bf16(backend, N, HW, C, inplace):
    acc, src = _join_operands(N, HW, C, 3 * HW + C)
    want = (acc.float() + src.permute(0, 2, 1)).to(BF16)
    if N * HW * C >= 1024:      # the operands tell one rounding from two
        assert not torch.equal(torch.nan_to_num(want.float()), torch.nan_to_num((acc + src.permute(0, 2, 1).to(BF16)).float()))
    if inplace:
        dev_acc = backend.d(acc.clone())
        backend.lib.nchw_f32_add_nhwc_bf16(backend.d(src), dev_acc, dev_acc, N, HW, C, None)
        got = dev_acc.cpu()
    else:
        got = torch.full((N, HW, C), float('nan'), dtype=BF16)
        backend.hostlib.nchw_f32_add_nhwc_bf16(src, acc.clone(), got, N, HW, C, None)
    _same_bits(got, want, 'nchw_f32_add_nhwc_bf16')


@pytest.mark.parametrize('n', [8, 64 * 35, 8 * 256 + 8, 2 * 16 * 16 * 512])
def test_bf16_add(backend, n):
    acc, src = _join_operands(1, n // 8, 8, n)
    a, b = acc.reshape(-1), src.permute(0, 2, 1).reshape(-1).to(BF16)
    want = (a.float() + b.float()).to(BF16)
    got = torch.full((n,), float('nan'), dtype=BF16)
    backend.hostlib.bf16_add(a, b, got, n, None)
    _same_bits(got, want, 'bf16_add')
    dev_a = backend.d(a.clone())
    backend.lib.bf16_add(dev_a, backend.d(b), dev_a, n, None)      # in place
    _same_bits(dev_a.cpu(), want, 'bf16_add in place')


def _refusal_cases():
    ok = dict(N=2, HW=5, C=64)
    bad = [('C=96', dict(ok, C=96), None, 'C must be a multiple of 64'), ('N=0', dict(ok, N=0), None, 'N, HW and C must be positive'),
           ('HW=-1', dict(ok, HW=-1), None, 'N, HW and C must be positive'), ('tiles', dict(N=1 << 30, HW=1 << 30, C=1 << 30), None, '2^31 tiles or more')]
    cases = []
    for name, nargs in (('nhwc_bf16_to_nchw_f32', 2), ('nchw_f32_to_nhwc_bf16', 2), ('nchw_f32_add_nhwc_bf16', 3)):
        for tag, dims, _, msg in bad:
            cases.append(pytest.param(name, nargs, dims, None, msg, id=f'{name}-{tag}'))
        for null in range(nargs):
            cases.append(pytest.param(name, nargs, ok, null, 'null buffer', id=f'{name}-null{null}'))
    return cases


@pytest.mark.parametrize('name,nargs,dims,null,msg', _refusal_cases())
def test_layout_argument_refusals(backend, name, nargs, dims, null, msg):
    """VFS_ERR_SHAPE and the text of vfs_last_error(), before anything is launched (the buffers are far too small for the sizes)"""
    bufs = [backend.d(torch.zeros(2 * 5 * 64)) for _ in range(nargs)]
    ptrs = [None if i == null else b.data_ptr() for i, b in enumerate(bufs)]
    rc = backend.lib.cfunc(name)(*ptrs, dims['N'], dims['HW'], dims['C'], None)
    assert (rc, backend.lib.last_error()) == (SHAPE_ERR, f'{name}: {msg}')


def test_bf16_add_argument_refusals(backend):
    buf = backend.d(torch.zeros(64, dtype=BF16))
    p = buf.data_ptr()
    fn = backend.lib.cfunc('bf16_add')
    for args, msg in (((p, p, p, 0), 'n must be positive'), ((p, p, p, 12), 'n must be a multiple of 8'), ((None, p, p, 8), 'null buffer'),
                      ((p, None, p, 8), 'null buffer'), ((p, p, None, 8), 'null buffer'), ((p, p, p, (1 << 40) + 8), 'more than 2^40 elements')):
        assert (fn(*args, None), backend.lib.last_error()) == (SHAPE_ERR, f'bf16_add: {msg}')


def test_host_statement_of_the_maps(tmp_path):
    """tools/layout_check.cpp: the element-wise maps, the rounding and the argument checks of csrc/layout_host.h (the text the
    launchers' checks compile), as a stand-alone host program"""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')      # the emulator build's compiler (vfs_amd/build.py)
    exe = str(tmp_path / 'layout_check')
    subprocess.run([cxx, '-std=c++17', '-O1', os.path.join(repo, 'tools', 'layout_check.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert (run.returncode, run.stdout.strip()) == (0, 'layout_check: ok'), run.stdout + run.stderr
