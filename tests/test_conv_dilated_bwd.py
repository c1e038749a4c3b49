"""Backward of the dilated convolutions (vfs_conv_dgrad_dilated / vfs_conv_wgrad_dilated, csrc/conv_dilated.hip) against torch
autograd of F.conv2d(x, w, None, stride, dil, dil) on the same bf16-rounded operands, exact-operand parity against float64
(regimes A and B of tests/test_conv_exact.py), and the argument checks of the two entry points.
backend=emu: host build through the fiber emulator; backend=gpu: libvfs_hip.so on the MI355X."""
import pytest
import torch
import torch.nn.functional as F

from tests.emu_util import nchw, nhwc, pack_relu_mask, rb, relerr
from tests.test_conv_exact import assert_bits, exact_ok, expect_bf16, ints, nan_like, nhwc64, oihw, signs, small_ok
from tests.test_emu_conv import pack
from vfs_amd.packing import build_reduce_table

BF16 = torch.bfloat16
CASES = [  # N, H, W, Cin, Cout, stride, dil   (3x3, padding = dilation)
    (2, 12, 16, 64, 128, 1, 2),      # the dilation-2 layer shape in small
    (1, 16, 16, 128, 64, 1, 4),      # two K-chunks per tap
    (2, 13, 13, 64, 64, 2, 2),       # stride 2 with dilation on an odd map
    (1, 5, 7, 64, 64, 1, 4),         # map smaller than the 9-pixel tap span: most taps are padding
    (3, 9, 11, 64, 64, 1, 2),        # ragged M = 297, odd batch
]
# the weight-gradient split plan of each case: (nsplit, pix_per_split); the last case runs its last split past M
PLANS = {CASES[0]: (2, 192), CASES[1]: (2, 128), CASES[2]: (2, 64), CASES[3]: (1, 64), CASES[4]: (3, 128)}


def out_hw(H, W, stride, dil):
    return (H + 2 * dil - 2 * dil - 1) // stride + 1, (W + 2 * dil - 2 * dil - 1) // stride + 1


def wgrad(lib, dy, x, partial, grad, N, H, W, Cin, Ho, Wo, Cout, stride, dil, nsplit, pps):
    lib.conv_wgrad_dilated(dy, x, partial, grad, N, H, W, Cin, Ho, Wo, Cout, 3, 3, stride, dil, dil, nsplit, pps, None)


@pytest.mark.parametrize('case', CASES)
def test_dilated_dgrad_wgrad_match_autograd(backend, case):
    N, H, W, Cin, Cout, stride, dil = case
    lib, d, dev = backend.lib, backend.d, backend.dev
    g = torch.Generator().manual_seed(N * 100 + H + dil)
    x = rb(torch.randn(N, Cin, H, W, generator=g))
    w = rb(torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (Cin * 9)) ** 0.5)
    _, wd = pack(backend, w)
    Ho, Wo = out_hw(H, W, stride, dil)
    M = N * Ho * Wo
    dy = rb(torch.randn(N, Cout, Ho, Wo, generator=g))
    add = rb(torch.randn(N, Cin, H, W, generator=g))
    y_blk = rb(torch.relu(torch.randn(N, H, W, Cin, generator=g)))      # the block output whose ReLU mask gates `add`
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    F.conv2d(xr, wr, None, stride, dil, dil).backward(dy)
    dyh, xh = d(nhwc(dy)), d(nhwc(x))

    def dgrad(add_t, mask_t):
        dx = nan_like((N, H, W, Cin), dev)
        lib.conv_dgrad_dilated(dyh, wd, dx, add_t, mask_t, N, H, W, Cin, Ho, Wo, Cout, 3, 3, stride, dil, dil, None)
        return nchw(dx.cpu())
    assert relerr(dgrad(None, None), xr.grad) < 6e-3
    assert relerr(dgrad(d(nhwc(add)), None), xr.grad + add) < 6e-3
    gated = add * (y_blk > 0).permute(0, 3, 1, 2)
    assert relerr(dgrad(d(nhwc(add)), d(pack_relu_mask(y_blk))), xr.grad + gated) < 6e-3

    nsplit, pps = PLANS[case]
    assert nsplit * pps >= M and (nsplit - 1) * pps < M
    if case == CASES[4]:
        assert nsplit >= 2 and nsplit * pps > M      # the last split runs past M = 297
    grads, parts = [], []
    for _ in range(2):
        partial = torch.full((nsplit, Cout, 9 * Cin), float('nan'), device=dev)
        grad = torch.ones(Cout, Cin, 3, 3, device=dev)
        wgrad(lib, dyh, xh, partial, grad, N, H, W, Cin, Ho, Wo, Cout, stride, dil, nsplit, pps)
        grads.append(grad.cpu())
        parts.append(partial.cpu())
    print(f'dilated wgrad relerr {relerr(grads[0] - 1.0, wr.grad):.3e}')
    assert relerr(grads[0] - 1.0, wr.grad) < 3e-4
    assert torch.equal(grads[0], grads[1]) and torch.equal(parts[0], parts[1])      # bit-identical from run to run
    # grad == NULL: partials only, reduced by the table-driven launch; equal to the direct form
    partial = torch.full((nsplit, Cout, 9 * Cin), float('nan'), device=dev)
    grad = torch.ones(Cout, Cin, 3, 3, device=dev)
    wgrad(lib, dyh, xh, partial, None, N, H, W, Cin, Ho, Wo, Cout, stride, dil, nsplit, pps)
    assert torch.equal(partial.cpu(), parts[0])
    assert torch.equal(grad.cpu(), torch.ones(Cout, Cin, 3, 3))
    tab, n, total = build_reduce_table([(partial, grad, nsplit, Cout, 9 * Cin, Cin, 3, 3, 0)], dev)
    lib.wgrad_reduce_table(tab, n, total, None)
    assert relerr(grad.cpu() - 1.0, wr.grad) < 3e-4
    assert relerr(grad.cpu(), grads[0]) < 2e-6      # (another fp32 order of the same split sums)


def im2col64_dil(x, stride, dil):
    """[M][(r, s, c)] float64: the rows the weight gradient reduces over, in its K order"""
    N, Cin = x.shape[:2]
    cols = F.unfold(x.double(), 3, dilation=dil, padding=dil, stride=stride)            # [N][(c, r, s)][L]
    return cols.reshape(N, Cin, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * Cin)


def run_dilated_backward_exact_operands(backend, case, regime):
    N, H, W, Cin, Cout, stride, dil = case
    lib, d, dev = backend.lib, backend.d, backend.dev
    g = torch.Generator().manual_seed(N * 100 + H + Cout + dil)
    r, dens = (2, 0.25) if regime == 'A' else (16, 0.75)
    Ho, Wo = out_hw(H, W, stride, dil)
    M = N * Ho * Wo
    x = ints(g, (N, Cin, H, W), -r, r)
    w = signs(g, (Cout, Cin, 3, 3), dens)
    dy = ints(g, (N, Cout, Ho, Wo), -r, r)
    add = ints(g, (N, Cin, H, W), -2 * r, 2 * r)
    y_blk = ints(g, (N, H, W, Cin), -1, 1)
    _, wd = pack(backend, w)
    dyh, xh = d(nhwc(dy)), d(nhwc(x))
    # ---- dgrad
    exact_ok(9 * Cout, dy, w)
    ref = nhwc64(F.conv_transpose2d(dy.double(), w.double(), None, stride, dil, (H - 1 + 2 * dil - 2 * dil) - (Ho - 1) * stride, 1, dil))
    assert ref.shape == (N, H, W, Cin)
    gated = nhwc64(add.double()) * (y_blk > 0)
    for add_t, mask_t, want, what in ((None, None, ref, 'dgrad'), (d(nhwc(add)), None, ref + nhwc64(add.double()), 'dgrad + add'),
                                      (d(nhwc(add)), d(pack_relu_mask(y_blk)), ref + gated, 'dgrad + add * mask')):
        small_ok(regime, want)
        dx = nan_like((N, H, W, Cin), dev)
        lib.conv_dgrad_dilated(dyh, wd, dx, add_t, mask_t, N, H, W, Cin, Ho, Wo, Cout, 3, 3, stride, dil, dil, None)
        assert_bits(dx, expect_bf16(want), f'{what} {case} regime {regime}')
    # ---- wgrad: one more split than M needs, so the last slice lies wholly past M
    exact_ok(M, dy, x)
    pps = 64 if M <= 128 else 128
    nsplit = (M + pps - 1) // pps + 1
    cols = im2col64_dil(x, stride, dil)                                   # [M][K]
    dyq = nhwc64(dy.double()).reshape(M, Cout)
    partial = torch.full((nsplit, Cout, 9 * Cin), float('nan'), device=dev)
    grad0 = ints(g, (Cout, Cin, 3, 3), -3, 3)
    grad = d(grad0.clone())
    wgrad(lib, dyh, xh, partial, grad, N, H, W, Cin, Ho, Wo, Cout, stride, dil, nsplit, pps)
    part = partial.cpu()
    for s in range(nsplit):
        sl = slice(s * pps, min(M, (s + 1) * pps))
        want = (dyq[sl].t() @ cols[sl]).float() if s * pps < M else torch.zeros(Cout, 9 * Cin)
        assert_bits(part[s], want, f'wgrad partial slice {s} of {nsplit} {case} regime {regime}', pixels=False)
    assert_bits(grad, (grad0.double() + oihw(dyq.t() @ cols, Cout, Cin, 3)).float(), f'wgrad {case} regime {regime}', pixels=False)


@pytest.mark.parametrize('regime', ['A', 'B'])
@pytest.mark.parametrize('case', [CASES[0], CASES[2], CASES[3]])
def test_dilated_backward_exact_operands(backend, case, regime):
    """every dgrad output is the RNE of the float64 sum (the residual added before the rounding, gated by the mask); every
    wgrad partial slice is the float64 sum over its pixel range, slices past M all zero; the reduced gradient is exact"""
    run_dilated_backward_exact_operands(backend, case, regime)


GOOD = dict(N=1, H=8, W=8, Cin=64, Ho=8, Wo=8, Cout=64, KH=3, KW=3, stride=1, pad=2, dilation=2)


@pytest.mark.parametrize('which', ['dgrad', 'wgrad'])
@pytest.mark.parametrize('change,code,word', [
    (dict(dilation=0), -3, 'dilation >= 1'),
    (dict(Ho=9), -1, 'output size does not match'),
    (dict(Wo=6), -1, 'output size does not match'),
    (dict(stride=2), -1, 'output size does not match'),        # stride 2 gives 4 x 4, not 8 x 8
    (dict(Cin=96), -1, 'Cin % 64 == 0'),
    (dict(Cout=72), -1, 'Cout % 64 == 0'),
    (dict(N=1 << 19, Cin=128), -1, '4 GiB'),                     # 2^19 * 64 * 128 * 2 bytes = 8 GiB of x
    (dict(null=0), -3, 'null'),
    (dict(null=1), -3, 'null'),
    (dict(null=2), -3, 'null'),
])
def test_dilated_backward_argument_errors(backend, which, change, code, word):
    """the checks run before any launch: the code and the message come back through vfs_last_error()"""
    lib, dev = backend.lib, backend.dev
    a = dict(GOOD, **{k: v for k, v in change.items() if k != 'null'})
    t = torch.zeros(64 * 64 * 9, dtype=BF16, device=dev)          # never touched: every call here fails its checks
    f = torch.zeros(64, device=dev)
    ptrs = [t, t, f if which == 'wgrad' else t]
    if 'null' in change:
        ptrs[change['null']] = None
    geom = (a['N'], a['H'], a['W'], a['Cin'], a['Ho'], a['Wo'], a['Cout'], a['KH'], a['KW'], a['stride'], a['pad'], a['dilation'])
    if which == 'dgrad':
        rc = lib.cfunc('conv_dgrad_dilated')(*[p.data_ptr() if p is not None else None for p in ptrs], None, None, *geom, None)
    else:
        rc = lib.cfunc('conv_wgrad_dilated')(*[p.data_ptr() if p is not None else None for p in ptrs], None, *geom, 1, 64, None)
    assert rc == code, (rc, lib.last_error())
    msg = lib.last_error()
    assert msg.startswith(f'conv_{which}_dilated: ') and word in msg, msg


def test_dilated_backward_other_argument_errors(backend):
    lib, dev = backend.lib, backend.dev
    t = torch.zeros(64 * 64 * 9, dtype=BF16, device=dev)
    f = torch.zeros(64, device=dev)
    geom = tuple(GOOD.values())
    m = torch.zeros(64, dtype=torch.uint8, device=dev)
    assert lib.cfunc('conv_dgrad_dilated')(t.data_ptr(), t.data_ptr(), t.data_ptr(), None, m.data_ptr(), *geom, None) == -3
    assert 'add_mask needs an add operand' in lib.last_error()
    assert lib.cfunc('conv_wgrad_dilated')(t.data_ptr(), t.data_ptr(), f.data_ptr(), None, *geom, 1, 32, None) == -1
    assert 'multiple of 64' in lib.last_error()
    assert lib.cfunc('conv_wgrad_dilated')(t.data_ptr(), t.data_ptr(), f.data_ptr(), None, *geom, 0, 64, None) == -1
    assert lib.cfunc('conv_wgrad_dilated')(t.data_ptr(), t.data_ptr(), f.data_ptr(), None, *geom, 1, 0, None) == -1
    assert lib.cfunc('conv_wgrad_dilated')(t.data_ptr(), t.data_ptr(), f.data_ptr(), None, *dict(GOOD, N=2).values(), 1, 64, None) == -1
    assert 'do not cover' in lib.last_error()
