"""Exact-operand parity of the bf16 convolution kernels against a float64 reference: every stored value is compared for
equality, no tolerance anywhere.

The kernels take bf16 operands, form exact products and accumulate in fp32.  With small-integer (or dyadic) operands every
product and every partial sum is representable, whatever the K order, split-K order, MFMA shape or tile walk, so the only
correct bf16 output is round-to-nearest-even of the exact sum, and the only correct fp32 output is the exact sum itself.

Two operand regimes:
  A (exact)    x, dy in [-2, 2], w in {-1, 0, 1} with a quarter of the entries non-zero, bias in [-3, 3], add in [-4, 4]: every
               output is an integer of magnitude <= 256, which bf16 stores unchanged - any wrong index, guard, tap, channel or
               split moves at least one output by >= 1.
  B (rounding) x, dy in [-16, 16], three quarters of the weights non-zero, bias in quarters: the exact sums reach the thousands
               and the stored value must be their RNE rounding.  A constructed 1x1 block in which EVERY output is an exact tie
               (odd integers 257 .. 511 and their negatives, bf16 spacing 2) separates RNE from truncation, round-half-away and
               round-half-up; the same block with a bias (forward) / residual (dgrad) of +-0.5 checks that the fp32 add
               happens before the rounding.
Each case asserts its own preconditions (K max|a| max|b| < 2^24 for every accumulation; max|reference| <= 256 in regime A)
before it calls a kernel.  Values are compared as numbers: NaN never matches, the sign of a zero is not looked at.

The fused BatchNorm epilogues are included because they are exact for dyadic parameters: vfs_conv_dgrad_bn sums g * mask and
g * mask * ((x - mean) * invstd) in fp32 (vfs_conv.h bnfuse_accum; integer g, x, dyadic mean, invstd = 1: every term and every
128-pixel sum is representable), vfs_conv_fwd_bnin / vfs_conv_wgrad_bnin stage relu(x * scale + shift) rounded to bf16
(bn_relu_vec; even-integer x, power-of-two scale, integer shift: a small integer).  Only the scale and shift rows take part in
the folded input BatchNorm; the mean / invstd rows are not combined with them.

Weight-gradient partials: the generic kernels split over linear pixel ranges, so slice s must equal the float64 sum over
pixels [s pps, (s + 1) pps) - splits and steps past M contribute exactly zero.  The 3x3 halo kernel splits over spatial tiles
with a split count of its own choosing that the C API does not report: there the written slices must add up to the gradient.
vfs_stem_wgrad and the 1x1 vfs_conv_wgrad_bnin run the generic kernel, which takes every split plan as offered: their slices
are compared one by one as well (the stem at its k = (r 8 + s + 1) 4 + c columns, c < 3; the padding columns, which hold the
fourth channel and are dropped by the reduction, are not looked at), the stem also on a plan whose second split runs past M.
The 3x3 vfs_conv_wgrad_bnin is the halo kernel again: its `partial` is zero-filled and not inspected, the reduced gradient it
adds into a non-zero integer `grad` is compared - with exact operands a wrong or doubled contribution moves it by at least 1.

backend=emu: host build through the fiber emulator; backend=gpu: libvfs_hip.so on the MI355X."""
import pytest
import torch
import torch.nn.functional as F

from tests.emu_util import nhwc, pack_relu_mask, rb, relerr
from tests.test_emu_conv import CASES, pack
from tests.test_pw import SHAPES as PW_SHAPES
from vfs_amd.packing import conv_halo_eligible, conv_stats_rows, igemm_ksplit, wgrad_halo_eligible, wgrad_inl_floats, wgrad_splits

BF16 = torch.bfloat16
REGIMES = ['A', 'B']


# ---------------------------------------------------------------------------------------------- helpers
def ints(g, shape, lo, hi, density=1.0):
    """integer-valued fp32 tensor, uniform in [lo, hi]; density < 1: that fraction of the entries kept, the rest zero"""
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g).float()
    if density < 1.0:
        t = t * (torch.rand(tuple(shape), generator=g) < density)
    return t


def signs(g, shape, density):
    """weights in {-1, 0, 1}: `density` of the entries non-zero"""
    return (ints(g, shape, 0, 1) * 2 - 1) * (torch.rand(tuple(shape), generator=g) < density)


def expect_bf16(t64):
    """RNE of the exact result (float64 -> fp32 is exact under the 2^24 precondition)"""
    return t64.float().to(BF16)


def exact_ok(K, *ops):
    """precondition of every accumulation: all partial sums are fp32-representable"""
    bound = float(K)
    for o in ops:
        bound *= float(o.abs().max())
    assert bound < 2 ** 24, f'test bug: K max|a| max|b| = {bound} is not below 2^24'


def small_ok(regime, ref):
    if regime == 'A':
        assert float(ref.abs().max()) <= 256, f'test bug: regime A reference reaches {float(ref.abs().max())} > 256'


def assert_bits(got, want, what, tile=128, pixels=True):
    """got == want element for element.  On a mismatch the message holds the count, the first wrong index - (n, h, w, c) for
    an NHWC tensor (pixels=False: any other 4-d tensor) -, both values, and where ALL the mismatches lie: image border, last
    pixel tile (the last `tile` rows of the [M][C] output matrix), last 8 / 32 / 64 channels"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, f'{what}: shape {tuple(got.shape)} != {tuple(want.shape)}'
    assert got.dtype == want.dtype, f'{what}: dtype {got.dtype} != {want.dtype}'
    bad = ~(got.double() == want.double())
    nbad = int(bad.sum())
    if nbad == 0:
        return
    idx = bad.nonzero()
    first = tuple(int(i) for i in idx[0])
    msg = f'{what}: {nbad} of {bad.numel()} elements differ; first at {first}: got {float(got[first])!r}, expected {float(want[first])!r}'
    if got.dim() == 4 and pixels:
        N, H, W, C = got.shape
        n, h, w, c = idx.unbind(1)
        M = N * H * W
        where = []
        if bool(((h == 0) | (h == H - 1) | (w == 0) | (w == W - 1)).all()):
            where.append('on an image border')
        if bool((((n * H + h) * W + w) >= (M - 1) // tile * tile).all()):
            where.append('in the last pixel tile')
        for last in (8, 32, 64):
            if C > last and bool((c >= C - last).all()):
                where.append(f'in the last {last} channels')
                break
        msg += '; (n, h, w, c) index; every mismatch lies ' + (', '.join(where) if where else 'nowhere in particular (spread)')
    raise AssertionError(msg)


def nhwc64(t):
    """NCHW float64 -> NHWC float64"""
    return t.permute(0, 2, 3, 1).contiguous()


def operands(regime, g, N, H, W, Cin, Cout, k, Ho, Wo):
    r, dens = (2, 0.25) if regime == 'A' else (16, 0.75)
    x = ints(g, (N, Cin, H, W), -r, r)
    w = signs(g, (Cout, Cin, k, k), dens)
    bias = ints(g, (Cout,), -3, 3) if regime == 'A' else ints(g, (Cout,), -12, 12) / 4
    dy = ints(g, (N, Cout, Ho, Wo), -r, r)
    add = ints(g, (N, Cin, H, W), -2 * r, 2 * r)
    return x, w, bias, dy, add


def out_size(H, W, k, stride, pad, dil=1):
    return (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1


def nan_like(shape, dev, dtype=BF16):
    return torch.full(tuple(shape), float('nan'), dtype=dtype, device=dev)


def check_stats_rows(regime, st, yq, linear, halves, what):
    """statistics rows [rows][2][C] against the stored values yq [M][C] (bf16 values as float64): every row where the rows are
    linear 128-pixel blocks, each half of the batch and the total otherwise.  The sums are exact (fp32 rows, values that are
    multiples of 1/4 below 2^13, 128 per row); the sums of squares are exact in regime A (128 * 256^2 < 2^24).  Regime B
    checks column 0 only: there 128 y^2 can exceed 2^24, so the fp32 sum of squares depends on the summation order and has
    no single correct value to compare with."""
    st = st.cpu().double()
    M, C = yq.shape
    nrow = st.shape[0]
    cols = (0, 1) if regime == 'A' else (0,)
    if regime == 'A':
        assert 128 * float(yq.abs().max()) ** 2 < 2 ** 24
    val = (yq, yq * yq)
    for col in cols:
        if linear:
            assert nrow == (M + 127) // 128
            want = torch.stack([val[col][r * 128:(r + 1) * 128].sum(0) for r in range(nrow)])
            assert_bits(st[:, col], want, f'{what}: statistics column {col}, one row per 128 pixels')
        else:
            for h in range(halves):
                rows = slice(h * nrow // halves, (h + 1) * nrow // halves)
                assert_bits(st[rows, col].sum(0), val[col][h * M // halves:(h + 1) * M // halves].sum(0),
                            f'{what}: statistics column {col}, part {h} of {halves} of the batch')
            assert_bits(st[:, col].sum(0), val[col].sum(0), f'{what}: statistics column {col}, total')


def im2col64(x, k, stride, pad):
    """[M][(r, s, c)] float64: the rows the weight-gradient kernels reduce over, in their K order"""
    N, Cin = x.shape[:2]
    cols = F.unfold(x.double(), k, padding=pad, stride=stride)            # [N][(c, r, s)][L]
    return cols.reshape(N, Cin, k * k, -1).permute(0, 3, 2, 1).reshape(-1, k * k * Cin)


def oihw(dwk, Cout, Cin, k):
    """[Cout][(r, s, c)] -> [Cout][Cin][k][k]"""
    return dwk.reshape(Cout, k, k, Cin).permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------- forward
FWD_CASES = CASES + [(3, 7, 7, 128, 72, 1, 1, 0),       # ragged channel tile (72 = 64 + 8)
                     (2, 2, 2, 1024, 256, 1, 1, 0)]     # DMA ring, 8 rows only
# dgrad / wgrad: the same, without the Cout = 72 shape (72 is no legal K of the dgrad, no legal tile height of the wgrad);
# (2, 2, 2, 1024, 256) is the 8-row DMA-ring dgrad and the ring weight gradient with M = 8
BWD_CASES = CASES + [(2, 2, 2, 1024, 256, 1, 1, 0)]


def run_fwd(be, regime, N, H, W, Cin, Cout, k, stride, pad):
    lib, d, dev = be.lib, be.d, be.dev
    g = torch.Generator().manual_seed(N * 100 + H + Cout)
    Ho, Wo = out_size(H, W, k, stride, pad)
    x, w, bias, _, _ = operands(regime, g, N, H, W, Cin, Cout, k, Ho, Wo)
    exact_ok(k * k * Cin, x, w)
    wf, _ = pack(be, w)
    xh = d(nhwc(x))
    nblk = conv_stats_rows(N, 1, H, W, Cin, Cout, k, stride, pad, Ho, Wo, lib=lib)
    linear = not conv_halo_eligible(N, H, W, Cin, Cout, k, stride, pad, lib=lib)
    halves = 2 if (N % 2 == 0 and conv_stats_rows(N, 2, H, W, Cin, Cout, k, stride, pad, Ho, Wo, lib=lib) is not None) else 1
    ref0 = nhwc64(F.conv2d(x.double(), w.double(), None, stride, pad))
    for b, flags in ((bias, (1,)), (None, (1, 0))):       # bias-free: statistics rows on the matrix cores (1) / per element (0)
        ref = ref0 + b.double() if b is not None else ref0
        small_ok(regime, ref)
        want = expect_bf16(ref)
        for flag in flags:
            lib.set_option(b'igemm_mfma_stats', flag)
            try:
                y = nan_like((N, Ho, Wo, Cout), dev)
                stats = nan_like((nblk, 2, Cout), dev, torch.float32)
                lib.conv_fwd(xh, wf, y, d(b) if b is not None else None, stats, N, H, W, Cin, Ho, Wo, Cout, k, k, stride, pad, None)
            finally:
                lib.set_option(b'igemm_mfma_stats', 1)
            what = f'conv_fwd {"with" if b is not None else "without"} bias, igemm_mfma_stats={flag}'
            assert_bits(y, want, what)
            check_stats_rows(regime, stats, want.double().reshape(-1, Cout), linear, halves, what)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout,k,stride,pad', FWD_CASES)
def test_forward(backend, regime, N, H, W, Cin, Cout, k, stride, pad):
    run_fwd(backend, regime, N, H, W, Cin, Cout, k, stride, pad)


# ---------------------------------------------------------------------------------------------- dgrad
def run_dgrad(be, regime, N, H, W, Cin, Cout, k, stride, pad):
    lib, d, dev = be.lib, be.d, be.dev
    g = torch.Generator().manual_seed(N * 100 + H + Cout + 1)
    Ho, Wo = out_size(H, W, k, stride, pad)
    _, w, _, dy, add = operands(regime, g, N, H, W, Cin, Cout, k, Ho, Wo)
    exact_ok(k * k * Cout, dy, w)
    _, wd = pack(be, w)
    ref = nhwc64(torch.nn.grad.conv2d_input((N, Cin, H, W), w.double(), dy.double(), stride, pad) + add.double())
    small_ok(regime, ref)
    dx = nan_like((N, H, W, Cin), dev)
    lib.conv_dgrad(d(nhwc(dy)), wd, dx, d(nhwc(add)), N, H, W, Cin, Ho, Wo, Cout, k, k, stride, pad, None)
    assert_bits(dx, expect_bf16(ref), 'conv_dgrad with the residual add')


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout,k,stride,pad', BWD_CASES)
def test_dgrad(backend, regime, N, H, W, Cin, Cout, k, stride, pad):
    run_dgrad(backend, regime, N, H, W, Cin, Cout, k, stride, pad)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout,k,stride,pad', [(3, 7, 7, 128, 64, 1, 1, 0), (2, 9, 11, 64, 64, 3, 2, 1), (1, 12, 12, 256, 128, 1, 1, 0)])
@pytest.mark.parametrize('onek', [3, 0])
def test_single_and_double_buffer_pipeline(backend, regime, N, H, W, Cin, Cout, k, stride, pad, onek):
    """igemm_onek = 3 (single buffer) / 0 (double buffer) without the DMA ring taking the 1x1 cases"""
    backend.lib.set_option(b'igemm_onek', onek)
    backend.lib.set_option(b'igemm_ring_tiles', 0)
    try:
        run_fwd(backend, regime, N, H, W, Cin, Cout, k, stride, pad)
        run_dgrad(backend, regime, N, H, W, Cin, Cout, k, stride, pad)
    finally:
        backend.lib.set_option(b'igemm_onek', 3)
        backend.lib.set_option(b'igemm_ring_tiles', 512)


def bn_rows_check(regime, part, gq, xq, mean, mask, linear, what):
    """fused BatchNorm-backward rows {sum g mask, sum g mask (x - mean)} (invstd = 1) of the stored gradient gq [M][C]"""
    t1 = gq * mask
    t2 = t1 * (xq - mean)
    exact_ok(128, t2)
    part = part.cpu().double()
    for col, val in ((0, t1), (1, t2)):
        if linear:
            want = torch.stack([val[r * 128:(r + 1) * 128].sum(0) for r in range(part.shape[0])])
            assert_bits(part[:, col], want, f'{what}: BatchNorm-backward column {col}, one row per 128 pixels')
        else:
            assert_bits(part[:, col].sum(0), val.sum(0), f'{what}: BatchNorm-backward column {col}, total')


def run_dgrad_masked_add_and_fused_bn_rows(backend, regime, N, H, W, Cin, Cout, k):
    lib, d, dev = backend.lib, backend.d, backend.dev
    g = torch.Generator().manual_seed(N * 13 + Cin + k)
    pad = k // 2
    _, w, _, dy, add = operands(regime, g, N, H, W, Cin, Cout, k, H, W)
    exact_ok(k * k * Cout, dy, w)
    _, wd = pack(backend, w)
    y = ints(g, (N, H, W, Cin), -3, 3)                      # block output whose ReLU mask gates the identity gradient
    gate = (y > 0).double()
    bits = d(pack_relu_mask(y))
    conv = nhwc64(torch.nn.grad.conv2d_input((N, Cin, H, W), w.double(), dy.double(), 1, pad))
    addh = nhwc64(add.double())
    ref = conv + addh * gate
    small_ok(regime, ref)
    want = expect_bf16(ref)
    dyd, addd = d(nhwc(dy)), d(nhwc(add))
    dx = nan_like((N, H, W, Cin), dev)
    lib.conv_dgrad_maskadd(dyd, wd, dx, addd, bits, N, H, W, Cin, H, W, Cout, k, k, 1, pad, None)
    assert_bits(dx, want, 'conv_dgrad_maskadd')
    # fused BatchNorm-backward rows
    M = N * H * W
    x = ints(g, (N, H, W, Cin), -3, 3)
    scale = 2.0 ** ints(g, (Cin,), -1, 1)
    shift, mean = ints(g, (Cin,), -4, 4) / 2, ints(g, (Cin,), -4, 4) / 2
    bnp = torch.stack([scale, shift, mean, torch.ones(Cin)], 0).reshape(1, 4, Cin).contiguous()
    nblk = conv_stats_rows(N, 1, H, W, Cout, Cin, k, 1, pad, H, W, lib=lib)       # the dgrad as a conv producing [N,H,W,Cin]
    linear = not conv_halo_eligible(N, H, W, Cout, Cin, k, 1, pad, lib=lib)
    xq, gq = x.double().reshape(M, Cin), want.double().reshape(M, Cin)
    ym = ints(g, (N, H, W, Cin), -2, 2)                     # activation of the unit the gradient belongs to (mask operand)
    pa, pb = nan_like((nblk, 2, Cin), dev, torch.float32), nan_like((nblk, 2, Cin), dev, torch.float32)
    dx2, dx3 = nan_like((N, H, W, Cin), dev), nan_like((N, H, W, Cin), dev)
    lib.conv_dgrad_bn(dyd, wd, dx2, d((addh * gate).to(BF16)), d(x.to(BF16)), d(pack_relu_mask(ym)), d(bnp), pa, M, 2,
                      N, H, W, Cin, H, W, Cout, k, k, 1, pad, None)
    assert_bits(dx2, want, 'conv_dgrad_bn')
    bn_rows_check(regime, pa, gq, xq, mean.double(), (ym > 0).double().reshape(M, Cin), linear, 'conv_dgrad_bn, bit-packed mask')
    lib.conv_dgrad_bn_maskadd(dyd, wd, dx3, addd, bits, d(x.to(BF16)), None, d(bnp), pb, M, 1, N, H, W, Cin, H, W, Cout, k, k, 1, pad, None)
    assert_bits(dx3, want, 'conv_dgrad_bn_maskadd')
    relu = ((xq * scale.double() + shift.double()) > 0).double()
    bn_rows_check(regime, pb, gq, xq, mean.double(), relu, linear, 'conv_dgrad_bn_maskadd, mask from x scale + shift')


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout,k', [
    (2, 8, 16, 128, 64, 1),      # implicit-GEMM dgrad, 128 produced channels: two 64-channel tiles by default (4 < igemm_narrow_below tiles)
    (3, 7, 7, 64, 256, 1),       # implicit-GEMM dgrad, 64-channel tile (32-channel waves), DMA ring, ragged M
    (2, 16, 32, 128, 64, 3),     # halo dgrad, 128 output channels
    (2, 32, 32, 64, 64, 3),      # halo dgrad, 64 output channels (16x16 tiles)
    (4, 7, 7, 128, 128, 3),      # halo dgrad on whole 7x7 images
])
def test_dgrad_masked_add_and_fused_bn_rows(backend, regime, N, H, W, Cin, Cout, k):
    """vfs_conv_dgrad_maskadd, vfs_conv_dgrad_bn (bit-packed mask operand) and vfs_conv_dgrad_bn_maskadd (mask recomputed from
    x scale + shift) against float64; dyadic BatchNorm parameters, invstd = 1"""
    run_dgrad_masked_add_and_fused_bn_rows(backend, regime, N, H, W, Cin, Cout, k)


# ---------------------------------------------------------------------------------------------- wgrad
def ring_settings(Cin, Cout, k, stride, pad):
    """`wgrad_ring` = 0 launches another kernel only where the LDS-DMA ring is dispatched: 1x1 / stride 1 / no padding with
    K = Cin and Cout both multiples of 128; elsewhere both settings are the same register-staged kernel"""
    return (1, 0) if (k == 1 and stride == 1 and pad == 0 and Cin % 128 == 0 and Cout % 128 == 0) else (1,)


def run_wgrad(be, regime, x, dy, k, stride, pad, nsplit, pps, halo):
    """conv_wgrad accumulating into a non-zero integer gradient (`wgrad_ring` = 1 and, where the ring is reached, 0) and
    conv_wgrad_inl"""
    lib, d, dev = be.lib, be.d, be.dev
    N, Cin, H, W = x.shape
    Cout, Ho, Wo = dy.shape[1], dy.shape[2], dy.shape[3]
    M, Ktot = N * Ho * Wo, k * k * Cin
    rings = ring_settings(Cin, Cout, k, stride, pad)
    exact_ok(M, x, dy)
    cols, dym = im2col64(x, k, stride, pad), nhwc64(dy.double()).reshape(M, Cout)
    slices = torch.stack([dym[s * pps:(s + 1) * pps].t() @ cols[s * pps:(s + 1) * pps] for s in range(nsplit)])
    dw = oihw(slices.sum(0), Cout, Cin, k)
    assert torch.equal(dw, torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, k, k), dy.double(), stride, pad))
    grad0 = ints(torch.Generator().manual_seed(M), (Cout, Cin, k, k), -5, 5)
    want = (grad0.double() + dw).float()
    xh, dyh = d(nhwc(x)), d(nhwc(dy))
    try:
        for ring in rings:
            lib.set_option(b'wgrad_ring', ring)
            partial = nan_like((nsplit, Cout, Ktot), dev, torch.float32)
            grad = d(grad0.clone())
            lib.conv_wgrad(dyh, xh, partial, grad, N, H, W, Cin, Ho, Wo, Cout, k, k, stride, pad, nsplit, pps, None)
            assert_bits(grad, want, f'conv_wgrad (wgrad_ring={ring}): gradient', pixels=False)
            p = partial.cpu()
            if not halo:
                assert_bits(p, slices.float(), f'conv_wgrad (wgrad_ring={ring}): partial slices [split][cout][(r, s, c)]')
            else:
                written = torch.isfinite(p).reshape(nsplit, -1)
                assert bool((written.all(1) | ~written.any(1)).all()) and bool(written[0].all())
                assert_bits(p[written.all(1)].double().sum(0), slices.sum(0), 'conv_wgrad (halo tiles): sum of the written slices')
    finally:
        lib.set_option(b'wgrad_ring', 1)
    tickets = torch.zeros(lib.cfunc('wgrad_tickets')(), dtype=torch.int32, device=dev)
    for rep in range(2):      # the second launch finds the tickets at zero
        gq = d(grad0.clone())
        wsi = nan_like((wgrad_inl_floats(nsplit, Cout, Ktot),), dev, torch.float32)
        lib.conv_wgrad_inl(dyh, xh, None, 0, wsi, gq, tickets, N, H, W, Cin, Ho, Wo, Cout, k, k, stride, pad, nsplit, pps, None)
        assert_bits(gq, want, f'conv_wgrad_inl, launch {rep}: gradient', pixels=False)
        assert int(tickets.cpu().abs().sum()) == 0


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout,k,stride,pad', BWD_CASES)
def test_wgrad(backend, regime, N, H, W, Cin, Cout, k, stride, pad):
    g = torch.Generator().manual_seed(N * 100 + H + Cout + 2)
    Ho, Wo = out_size(H, W, k, stride, pad)
    x, _, _, dy, _ = operands(regime, g, N, H, W, Cin, Cout, k, Ho, Wo)
    is_halo = wgrad_halo_eligible(N, H, W, Cin, Cout, k, stride, pad, lib=backend.lib)
    nsplit, pps = wgrad_splits(N * Ho * Wo, Cout, k * k * Cin, target_blocks=12, halo_geom=(N, H, W, Cin) if is_halo else None, lib=backend.lib)
    run_wgrad(backend, regime, x, dy, k, stride, pad, nsplit, pps, is_halo)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('M_img,Cin,Cout,nsplit,pps', [
    (8, 128, 64, 1, 64), (16, 128, 64, 1, 128), (24, 128, 64, 1, 192), (40, 128, 64, 1, 320), (40, 128, 64, 2, 192), (72, 128, 64, 3, 192),
    (33, 128, 64, 1, 320),                                  # pixel steps in pairs: 1, 2, 3, 5 per split, last steps past M
    (50, 256, 128, 4, 128), (64, 128, 128, 1, 512)])        # the LDS-DMA ring: M = 400, the last split half past M; 8 steps
def test_wgrad_pixel_steps_and_splits_past_m(backend, regime, M_img, Cin, Cout, nsplit, pps):
    """the seven Cout = 64 shapes run the register-staged kernel (one `wgrad_ring` setting: the ring needs Cout % 128 == 0),
    the last two the ring and, with `wgrad_ring` = 0, the register-staged kernel on the same splits"""
    g = torch.Generator().manual_seed(M_img + nsplit + Cin)
    assert nsplit * pps >= M_img * 8
    x, _, _, dy, _ = operands(regime, g, 1, M_img, 8, Cin, Cout, 1, M_img, 8)
    run_wgrad(backend, regime, x, dy, 1, 1, 0, nsplit, pps, False)


# ---------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize('regime', REGIMES)
def test_stem(backend, regime):
    """stem_fwd on every stem_blocks / stem_direct setting and stem_wgrad; a non-zero fourth input channel (padding: its
    weights are zero, its gradient columns are dropped) must change nothing"""
    lib, d, dev = backend.lib, backend.d, backend.dev
    g = torch.Generator().manual_seed(5)
    N, H, W = 2, 20, 18
    r = 2 if regime == 'A' else 16
    x = ints(g, (N, 3, H, W), -r, r)
    w = signs(g, (64, 3, 7, 7), 0.25 if regime == 'A' else 0.75)
    exact_ok(147, x, w)
    wf, _ = pack(backend, w, stem=True)
    Ho, Wo = out_size(H, W, 7, 2, 3)
    M = N * Ho * Wo
    x4 = nan_like((N, H, W, 4), dev)
    lib.imgs_to_nhwc4(d(x.reshape(N, 1, 3, 1, H, W).contiguous()), x4, N, 1, 1, H, W, W, None)
    x4n = x4.clone()
    x4n[..., 3] = 3.0
    ref = nhwc64(F.conv2d(x.double(), w.double(), None, 2, 3))
    small_ok(regime, ref)
    want = expect_bf16(ref)
    ntile = N * ((Ho + 7) // 8) * ((Wo + 15) // 16)
    for src, blocks in ((x4, 0), (x4, 1), (x4, 3), (x4n, 0)):
        y, stats = nan_like((N, Ho, Wo, 64), dev), nan_like((ntile, 2, 64), dev, torch.float32)
        lib.set_option(b'stem_blocks', blocks)
        try:
            lib.stem_fwd(src, wf, y, stats, N, H, W, Ho, Wo, None)
        finally:
            lib.set_option(b'stem_blocks', 0)
        what = f'stem_fwd, stem_blocks={blocks}' + (', fourth channel non-zero' if src is x4n else '')
        assert_bits(y, want, what)
        check_stats_rows(regime, stats, want.double().reshape(M, 64), False, 2, what)
    lib.set_option(b'stem_direct', 0)
    try:
        y2 = nan_like((N, Ho, Wo, 64), dev)
        lib.stem_fwd(x4, wf, y2, None, N, H, W, Ho, Wo, None)
    finally:
        lib.set_option(b'stem_direct', 1)
    assert_bits(y2, want, 'stem_fwd, stem_direct=0')
    dy = ints(g, (N, 64, Ho, Wo), -r, r)
    exact_ok(M, x, dy)
    grad0 = ints(g, (64, 3, 7, 7), -5, 5)
    wantg = (grad0.double() + torch.nn.grad.conv2d_weight(x.double(), (64, 3, 7, 7), dy.double(), 2, 3)).float()
    cols, dym = im2col64(x, 7, 2, 3), nhwc64(dy.double()).reshape(M, 64)                  # [M][(r, s, c)], c < 3
    kcol = torch.tensor([(r * 8 + s + 1) * 4 + c for r in range(7) for s in range(7) for c in range(3)])
    assert M % 128 != 0 and 2 * 128 >= M
    for src, (nsplit, pps) in ((x4, wgrad_splits(M, 64, 256, target_blocks=6)), (x4n, wgrad_splits(M, 64, 256, target_blocks=6)),
                               (x4n, (2, 128))):      # the second split of the last plan runs past M
        partial = nan_like((nsplit, 64, 256), dev, torch.float32)
        grad = d(grad0.clone())
        lib.stem_wgrad(d(nhwc(dy)), src, partial, grad, N, H, W, Ho, Wo, nsplit, pps, None)
        what = f'stem_wgrad, {nsplit} x {pps} pixels' + (', fourth channel non-zero' if src is x4n else '')
        assert_bits(grad, wantg, what, pixels=False)
        slices = torch.stack([dym[i * pps:(i + 1) * pps].t() @ cols[i * pps:(i + 1) * pps] for i in range(nsplit)])
        assert_bits(partial.cpu()[:, :, kcol], slices.float(), what + ': partial slices [split][cout][(r, s, c)]')


# ---------------------------------------------------------------------------------------------- dilated, split-K
def run_dilated_forward(backend, regime, N, H, W, Cin, Cout, stride, dil):
    lib, d = backend.lib, backend.d
    g = torch.Generator().manual_seed(N + H + dil)
    Ho, Wo = out_size(H, W, 3, stride, dil, dil)
    x, w, _, _, _ = operands(regime, g, N, H, W, Cin, Cout, 3, Ho, Wo)
    exact_ok(9 * Cin, x, w)
    wf, _ = pack(backend, w)
    ref = nhwc64(F.conv2d(x.double(), w.double(), None, stride, dil, dil))
    small_ok(regime, ref)
    y = nan_like((N, Ho, Wo, Cout), backend.dev)
    lib.conv_fwd_dilated(d(nhwc(x)), wf, y, None, None, N, H, W, Cin, Ho, Wo, Cout, 3, 3, stride, dil, dil, None)
    assert_bits(y, expect_bf16(ref), 'conv_fwd_dilated')


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout,stride,dil', [(2, 12, 16, 64, 128, 1, 2), (1, 16, 16, 128, 64, 1, 4), (2, 13, 13, 64, 64, 2, 2)])
def test_dilated_forward(backend, regime, N, H, W, Cin, Cout, stride, dil):
    run_dilated_forward(backend, regime, N, H, W, Cin, Cout, stride, dil)


def run_splitk(backend, regime, M, Cin, Cout):
    lib, d, dev = backend.lib, backend.d, backend.dev
    g = torch.Generator().manual_seed(M + Cin)
    x, w, bias, dy, add = operands(regime, g, M, 1, 1, Cin, Cout, 1, 1, 1)
    exact_ok(Cin, x, w)
    exact_ok(Cout, dy, w)
    wf, wd = pack(backend, w)
    xh = d(nhwc(x))
    ks, need = igemm_ksplit(M, Cout, Cin)
    assert ks > 1 and need > 1024
    ws = torch.zeros(need, device=dev)
    nblk = (M + 127) // 128
    ref = nhwc64(F.conv2d(x.double(), w.double(), bias.double()))
    small_ok(regime, ref)
    want = expect_bf16(ref)
    outs = []
    for which in ('plain', 'split', 'split'):
        y, st = nan_like((M, 1, 1, Cout), dev), nan_like((nblk, 2, Cout), dev, torch.float32)
        if which == 'plain':
            lib.conv_fwd(xh, wf, y, d(bias), st, M, 1, 1, Cin, 1, 1, Cout, 1, 1, 1, 0, None)
        else:
            lib.conv_fwd_splitk(xh, wf, y, d(bias), st, ws, ks, M, 1, 1, Cin, 1, 1, Cout, 1, 1, 1, 0, None)
        assert_bits(y, want, f'forward, {which} kernel')
        check_stats_rows(regime, st, want.double().reshape(M, Cout), True, 1, f'forward, {which} kernel')
        outs.append(st.cpu())
    assert_bits(outs[1], outs[0], 'statistics rows, split-K against the plain kernel')
    assert_bits(outs[2], outs[0], 'statistics rows, second split-K launch against the plain kernel')
    assert torch.equal(ws[:1024].cpu(), torch.zeros(1024))
    refd = nhwc64(torch.nn.grad.conv2d_input((M, Cin, 1, 1), w.double(), dy.double()) + add.double())
    small_ok(regime, refd)
    wantd = expect_bf16(refd)
    ks2, need2 = igemm_ksplit(M, Cin, Cout)
    assert (ks2 > 1) == (Cout >= 256), 'test bug: the split dgrad is expected on exactly the shapes with Cout >= 256'
    dx = nan_like((M, 1, 1, Cin), dev)
    lib.conv_dgrad(d(nhwc(dy)), wd, dx, d(nhwc(add)), M, 1, 1, Cin, 1, 1, Cout, 1, 1, 1, 0, None)
    assert_bits(dx, wantd, 'dgrad, plain kernel')
    if ks2 > 1:
        ws2 = torch.zeros(need2, device=dev)
        for rep in range(2):
            dx = nan_like((M, 1, 1, Cin), dev)
            lib.conv_dgrad_splitk(d(nhwc(dy)), wd, dx, d(nhwc(add)), ws2, ks2, M, 1, 1, Cin, 1, 1, Cout, 1, 1, 1, 0, None)
            assert_bits(dx, wantd, f'dgrad, split-K kernel, launch {rep}')
        assert torch.equal(ws2[:1024].cpu(), torch.zeros(1024))


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('M,Cin,Cout', [(64, 512, 256), (200, 256, 192), (8, 1024, 128),
                                        (40, 512, 512)])      # ragged M, eight K-steps in both directions
def test_splitk_equals_plain_kernel_and_float64(backend, regime, M, Cin, Cout):
    """exact partial tiles: the split-K forward / dgrad must equal the plain kernel element for element, statistics rows
    included, and both the float64 result; the tickets come back to zero (second launch).  The forward splits on every
    shape.  The dgrad's K is Cout: the planner splits only from four 64-channel K-steps on, so conv_dgrad_splitk runs on
    (64, 512, 256) and (40, 512, 512); with Cout = 192 and 128 the plan is one slice and the plain dgrad is all there is."""
    run_splitk(backend, regime, M, Cin, Cout)


# ---------------------------------------------------------------------------------------------- folded input BatchNorm
def run_folded_input_batchnorm(backend, regime, N, H, W, Cin, Cout, G, k):
    lib, d, dev = backend.lib, backend.d, backend.dev
    g = torch.Generator().manual_seed(N + H + Cin + k)
    pad = k // 2
    rr = 2 if regime == 'A' else 8
    raw = ints(g, (N, H, W, Cin), -rr, rr) * 2
    scale, shift = 2.0 ** ints(g, (G, Cin), -1, 0), ints(g, (G, Cin), -1, 1)
    bnp = torch.stack([scale, shift, ints(g, (G, Cin), -4, 4) / 2, torch.ones(G, Cin)], 1).contiguous()
    npg = N // G
    per_img = lambda p: p.repeat_interleave(npg, 0).reshape(N, 1, 1, Cin).double()
    act = torch.relu(raw.double() * per_img(scale) + per_img(shift))         # integers: exact in bf16
    assert torch.equal(act, act.round()) and float(act.max()) <= 256
    act_nchw = act.permute(0, 3, 1, 2).contiguous()
    w = signs(g, (Cout, Cin, k, k), 0.25 if regime == 'A' else 0.75)
    exact_ok(k * k * Cin, act, w)
    wf, _ = pack(backend, w)
    M = N * H * W
    ref = nhwc64(F.conv2d(act_nchw, w.double(), None, 1, pad))
    small_ok(regime, ref)
    want = expect_bf16(ref)
    rawd, bnpd = d(raw.to(BF16)), d(bnp)
    nblk = conv_stats_rows(N, 1, H, W, Cin, Cout, k, 1, pad, H, W, lib=lib)
    y, st = nan_like((N, H, W, Cout), dev), nan_like((nblk, 2, Cout), dev, torch.float32)
    lib.conv_fwd_bnin(rawd, bnpd, npg, wf, y, None, st, N, H, W, Cin, H, W, Cout, k, k, 1, pad, None)
    assert_bits(y, want, 'conv_fwd_bnin')
    check_stats_rows(regime, st, want.double().reshape(M, Cout), k == 1, 2 if G == 2 else 1, 'conv_fwd_bnin')
    dy = ints(g, (N, Cout, H, W), -rr, rr)
    exact_ok(M, act, dy)
    grad0 = ints(g, (Cout, Cin, k, k), -5, 5)
    wantg = (grad0.double() + torch.nn.grad.conv2d_weight(act_nchw, (Cout, Cin, k, k), dy.double(), 1, pad)).float()
    nsplit, pps = wgrad_splits(M, Cout, k * k * Cin, target_blocks=12, halo_geom=(N, H, W, Cin) if k == 3 else None, lib=lib)
    # 1x1: the generic kernel, linear pixel ranges - every slice is compared; 3x3: the halo kernel's own split count
    partial = nan_like((nsplit, Cout, Cin), dev, torch.float32) if k == 1 else torch.zeros(nsplit, Cout, 9 * Cin, device=dev)
    grad = d(grad0.clone())
    lib.conv_wgrad_bnin(d(nhwc(dy)), rawd, bnpd, npg, partial, grad, N, H, W, Cin, H, W, Cout, k, k, 1, pad, nsplit, pps, None)
    assert_bits(grad, wantg, 'conv_wgrad_bnin', pixels=False)
    if k == 1:
        am, dym = act.reshape(M, Cin), nhwc64(dy.double()).reshape(M, Cout)
        slices = torch.stack([dym[i * pps:(i + 1) * pps].t() @ am[i * pps:(i + 1) * pps] for i in range(nsplit)])
        assert_bits(partial.cpu(), slices.float(), 'conv_wgrad_bnin: partial slices [split][cout][cin]')
    if k == 3:
        tickets = torch.zeros(lib.cfunc('wgrad_tickets')(), dtype=torch.int32, device=dev)
        grad = d(grad0.clone())
        wsi = nan_like((wgrad_inl_floats(nsplit, Cout, 9 * Cin),), dev, torch.float32)
        lib.conv_wgrad_inl(d(nhwc(dy)), rawd, bnpd, npg, wsi, grad, tickets, N, H, W, Cin, H, W, Cout, 3, 3, 1, 1, nsplit, pps, None)
        assert_bits(grad, wantg, 'conv_wgrad_inl with the folded input BatchNorm', pixels=False)
        assert int(tickets.cpu().abs().sum()) == 0


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout,G,k', [
    (2, 16, 32, 128, 128, 2, 3),     # 8x16 tiles, two channel chunks, two groups
    (2, 32, 32, 64, 64, 2, 3),       # 16x16 tiles (64 output channels)
    (4, 8, 8, 64, 128, 2, 3),        # whole 8x8 images, two per tile
    (2, 14, 14, 64, 128, 2, 3),      # ragged 8x16 tiles
    (4, 7, 7, 64, 128, 2, 3),        # whole 7x7 images, two per tile
    (2, 28, 28, 64, 64, 1, 3),       # ragged 16x16 tiles (forward) / 8x16 tiles (weight gradient)
    (2, 8, 16, 64, 256, 2, 1),       # 1x1: one K-step (the single-buffer pipeline), four 64-channel tiles by default, two groups
    (4, 8, 8, 128, 512, 2, 1),       # 1x1: two K-steps, two groups of 128 pixels
    (2, 16, 16, 256, 128, 1, 1),     # 1x1: four K-steps
    (2, 8, 8, 64, 64, 1, 1),         # 1x1: 64-channel tile
])
def test_folded_input_batchnorm(backend, regime, N, H, W, Cin, Cout, G, k):
    """vfs_conv_fwd_bnin / vfs_conv_wgrad_bnin (/ vfs_conv_wgrad_inl with the fold, 3x3) against float64 on
    relu(raw scale + shift): even-integer raw values, scale in {1/2, 1}, integer shift, per group"""
    run_folded_input_batchnorm(backend, regime, N, H, W, Cin, Cout, G, k)


# ---------------------------------------------------------------------------------------------- opt-in pointwise kernels
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout', PW_SHAPES)
def test_persistent_pointwise_kernel(backend, regime, N, H, W, Cin, Cout):
    """the persistent producer / consumer 1x1 kernel (igemm_pw = 2): forward with and without bias (+ statistics rows),
    dgrad with the residual add"""
    lib, d, dev = backend.lib, backend.d, backend.dev
    g = torch.Generator().manual_seed(N * 17 + Cin + Cout)
    x, w, bias, dy, add = operands(regime, g, N, H, W, Cin, Cout, 1, H, W)
    exact_ok(Cin, x, w)
    exact_ok(Cout, dy, w)
    wf, wd = pack(backend, w)
    M, nblk = N * H * W, (N * H * W + 127) // 128
    ref0 = nhwc64(F.conv2d(x.double(), w.double()))
    refd = nhwc64(torch.nn.grad.conv2d_input((N, Cin, H, W), w.double(), dy.double()) + add.double())
    lib.set_option(b'igemm_pw', 2)
    try:
        for b in (None, bias):
            ref = ref0 + b.double() if b is not None else ref0
            small_ok(regime, ref)
            want = expect_bf16(ref)
            y, st = nan_like((N, H, W, Cout), dev), nan_like((nblk, 2, Cout), dev, torch.float32)
            lib.conv_fwd(d(nhwc(x)), wf, y, d(b) if b is not None else None, st, N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, None)
            what = f'persistent 1x1 forward {"with" if b is not None else "without"} bias'
            assert_bits(y, want, what)
            check_stats_rows(regime, st, want.double().reshape(M, Cout), True, 1, what)
        if Cout % 64 == 0:      # the dgrad's K is Cout
            small_ok(regime, refd)
            dx = nan_like((N, H, W, Cin), dev)
            lib.conv_dgrad(d(nhwc(dy)), wd, dx, d(nhwc(add)), N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, None)
            assert_bits(dx, expect_bf16(refd), 'persistent 1x1 dgrad with the residual add')
    finally:
        lib.set_option(b'igemm_pw', 0)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('M,Cin,Cout', [(64, 2048, 512), (40, 256, 64), (128, 512, 2048), (8, 128, 16), (97, 384, 48)])
def test_skinny_linear_layers(backend, regime, M, Cin, Cout):
    """the skinny GEMM (igemm_skinny = 1) and the implicit-GEMM kernel (0) on the head's Linear shapes: forward with bias,
    dgrad with the residual operand"""
    lib, d, dev = backend.lib, backend.d, backend.dev
    g = torch.Generator().manual_seed(M + Cin + Cout)
    x, w, bias, dy, add = operands(regime, g, M, 1, 1, Cin, Cout, 1, 1, 1)
    exact_ok(Cin, x, w)
    exact_ok(Cout, dy, w)
    wf, wd = pack(backend, w)
    ref = nhwc64(F.conv2d(x.double(), w.double(), bias.double()))
    refd = nhwc64(torch.nn.grad.conv2d_input((M, Cin, 1, 1), w.double(), dy.double()) + add.double())
    small_ok(regime, ref)
    for flag in (1, 0):
        lib.set_option(b'igemm_skinny', flag)
        try:
            y = nan_like((M, 1, 1, Cout), dev)
            lib.conv_fwd(d(nhwc(x)), wf, y, d(bias), None, M, 1, 1, Cin, 1, 1, Cout, 1, 1, 1, 0, None)
            assert_bits(y, expect_bf16(ref), f'linear forward, igemm_skinny={flag}')
            if Cout % 128 == 0 and Cin % 16 == 0:     # the dgrad's K is Cout
                small_ok(regime, refd)
                dx = nan_like((M, 1, 1, Cin), dev)
                lib.conv_dgrad(d(nhwc(dy)), wd, dx, d(nhwc(add)), M, 1, 1, Cin, 1, 1, Cout, 1, 1, 1, 0, None)
                assert_bits(dx, expect_bf16(refd), f'linear dgrad, igemm_skinny={flag}')
        finally:
            lib.set_option(b'igemm_skinny', 1)


# ---------------------------------------------------------------------------------------------- the tie block
def is_tie(t64):
    """exactly half way between two neighbouring bf16 values"""
    return (t64.float().contiguous().view(torch.int32) & 0xFFFF) == 0x8000


def tie_block(K, N=3, H=7, W=7, C=256):
    """1x1 problem whose every output is an exact bf16 tie: pixel p is sigma_p on channels (a_p, a_p + 1), a_p even, zero
    elsewhere; weight row c holds s_c 256 on the even channels and s_c (2 j_c + 1) on the odd ones, j_c = c mod 128: output
    (p, c) = sigma_p s_c (257 + 2 j_c), the odd integers 257 .. 511 and their negatives (bf16 spacing there: 2).
    Returns x [N][K][H][W], w [C][K][1][1] and the float64 NHWC result [N][H][W][C]."""
    M = N * H * W
    p = torch.arange(M)
    sigma = 1.0 - 2.0 * ((p // 3) % 2)
    xm = torch.zeros(M, K)
    a = 2 * (p % (K // 2))
    xm[p, a], xm[p, a + 1] = sigma, sigma
    c = torch.arange(C)
    s = 1.0 - 2.0 * ((c // 5) % 2)
    w = torch.zeros(C, K)
    w[:, 0::2] = (s * 256)[:, None]
    w[:, 1::2] = (s * (2 * (c % 128) + 1))[:, None]
    assert torch.equal(rb(w), w)
    ref = (xm.double() @ w.double().t()).reshape(N, H, W, C)
    ties = is_tie(ref)
    assert int(ties.sum()) == ref.numel(), 'test bug: the block holds outputs that are no ties'
    up = expect_bf16(ref).double().abs() > ref.abs()
    assert int(up.sum()) * 2 == ref.numel(), 'test bug: RNE must round half of the ties up and half down'
    return xm.reshape(N, H, W, K).permute(0, 3, 1, 2).contiguous(), w.reshape(C, K, 1, 1), ref


def run_tie_block(backend, K, half):
    lib, d, dev = backend.lib, backend.d, backend.dev
    N, H, W, C = 3, 7, 7, 256
    x, w, ref = tie_block(K)
    want = expect_bf16(ref + half)
    if half:
        assert not bool(is_tie(ref + half).any()) and not torch.equal(want, expect_bf16(expect_bf16(ref).double() + half))
    wf, _ = pack(backend, w)
    y = nan_like((N, H, W, C), dev)
    lib.conv_fwd(d(nhwc(x)), wf, y, d(torch.full((C,), half)) if half else None, None, N, H, W, K, H, W, C, 1, 1, 1, 0, None)
    assert_bits(y, want, f'tie block forward, bias {half}')
    # dgrad: the same matrix as the transposed weight (K = Cout of the dgrad, outputs = its Cin)
    _, wd = pack(backend, w.reshape(C, K).t().reshape(K, C, 1, 1).contiguous())
    dx = nan_like((N, H, W, C), dev)
    add = d(torch.full((N, H, W, C), half, dtype=BF16)) if half else None
    lib.conv_dgrad(d(nhwc(x)), wd, dx, add, N, H, W, C, H, W, K, 1, 1, 1, 0, None)
    assert_bits(dx, want, f'tie block dgrad, residual {half}')


@pytest.mark.parametrize('K', [64, 256])        # one K-step; four K-steps (the DMA-ring variant)
@pytest.mark.parametrize('half', [0.0, 0.5, -0.5])
def test_tie_block(backend, K, half):
    """every output an exact tie (half = 0): RNE alone passes.  half = +-0.5 as bias (forward) / residual (dgrad): no ties
    any more - the fp32 add must happen before the rounding (257 + 0.5 -> 258, rne(257) + 0.5 -> 256)"""
    run_tie_block(backend, K, half)


# ---------------------------------------------------------------------------------------------- self-check of the comparison
def _fails(got, want, match=None):
    with pytest.raises(AssertionError, match=match) as e:
        assert_bits(got, want, 'self-check')
    return str(e.value)


def _truncate(t64):
    f = t64.float().contiguous()
    return (f.view(torch.int32) & -65536).view(torch.float32).to(BF16)


def test_comparison_catches_what_the_max_norm_bar_accepts():
    """CPU only, no kernel: four perturbations of a float64 reference standing in for a broken kernel.  On the Gaussian
    operands of CASES[0] the existing bar (relerr < 6e-3) accepts them; on exact operands assert_bits rejects them.
    Perturbations are picked deterministically: at one fixed pixel, the first (output channel, input channel) in index
    order that changes the Gaussian reference and that the old bar accepts; the test fails if there is none.  The regime-A
    data get an index of their own, the first at which the same perturbation changes that reference: the sparse regime-A
    weights are zero at most positions, and removing or swapping a zero product would change nothing there."""
    N, H, W, Cin, Cout, k, stride, pad = CASES[0]
    g = torch.Generator().manual_seed(N * 100 + H)
    xg = rb(torch.randn(N, Cin, H, W, generator=g))
    wg = rb(torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5)
    ga = torch.Generator().manual_seed(1)
    xa, wa, _, _, _ = operands('A', ga, N, H, W, Cin, Cout, k, H, W)
    refg = nhwc64(F.conv2d(xg.double(), wg.double(), None, stride, pad))
    refa = nhwc64(F.conv2d(xa.double(), wa.double(), None, stride, pad))
    bar = lambda got64: relerr(expect_bf16(got64).float(), refg)
    assert bar(refg) < 6e-3
    n, ho, wo, r, s = 1, 0, 4, 1, 1                      # a pixel of the top border; its centre tap reads x[n, :, ho, wo]

    # 1. one product x w missing at that pixel
    def drop(ref, x, w, co, ci):
        out = ref.clone()
        out[n, ho, wo, co] -= x[n, ci, ho, wo].double() * w[co, ci, r, s].double()
        return out
    pairs = [(co, ci) for co in range(Cout) for ci in range(Cin)]
    under_bar = next((p for p in pairs if xg[n, p[1], ho, wo] * wg[p][r, s] != 0 and bar(drop(refg, xg, wg, *p)) < 6e-3), None)
    assert under_bar is not None, 'no missing product at that pixel stays under the old bar'
    co, ci = next((p for p in pairs if xa[n, p[1], ho, wo] * wa[p][r, s] != 0), (None, None))
    assert co is not None, 'test bug: no non-zero product at that pixel in the regime-A data'
    msg = _fails(expect_bf16(drop(refa, xa, wa, co, ci)), expect_bf16(refa), match='on an image border')
    assert f'first at ({n}, {ho}, {wo}, {co})' in msg and '1 of' in msg

    # 2. the last two input channels (inside the last 8-channel chunk) swapped for that tap
    def swap(ref, x, w, co):
        c1, c2 = Cin - 2, Cin - 1
        x1, x2, w1, w2 = (t.double() for t in (x[n, c1, ho, wo], x[n, c2, ho, wo], w[co, c1, r, s], w[co, c2, r, s]))
        out = ref.clone()
        out[n, ho, wo, co] += (x2 - x1) * (w1 - w2)
        return out
    under_bar = next((co for co in range(Cout) if not torch.equal(swap(refg, xg, wg, co), refg) and bar(swap(refg, xg, wg, co)) < 6e-3), None)
    assert under_bar is not None, 'no channel swap at that pixel stays under the old bar'
    co = next((co for co in range(Cout) if not torch.equal(swap(refa, xa, wa, co), refa)), None)
    assert co is not None, 'test bug: the swap changes no output of the regime-A data'
    _fails(expect_bf16(swap(refa, xa, wa, co)), expect_bf16(refa), match='on an image border')

    # 3. truncation instead of RNE: under the bar on Gaussian data, caught by the tie block (as are round-half-away and
    #    round-half-up, which move the other half of the ties)
    assert relerr(_truncate(refg).float(), refg) < 6e-3
    _, _, tie = tie_block(64)
    want = expect_bf16(tie)
    lo, hi = _truncate(tie).double(), _truncate(tie).double() + 2 * torch.sign(tie)
    assert torch.equal(torch.minimum(lo.abs(), hi.abs()), lo.abs()) and torch.equal((lo + hi) / 2, tie)
    for name, got in (('truncation', lo), ('round half away from zero', hi), ('round half up', torch.maximum(lo, hi))):
        msg = _fails(got.to(BF16), want)
        if name != 'round half up':      # (that one moves the ties RNE rounds down where positive, up where negative)
            assert f'{tie.numel() // 2} of {tie.numel()}' in msg, (name, msg)

    # 4. the last (ragged) row of the output matrix written one slot early
    want = expect_bf16(refa)
    M = N * H * W
    got = want.clone().reshape(M, Cout)
    got[M - 2] = want.reshape(M, Cout)[M - 1]
    got[M - 1] = float('nan')                            # (output buffers are pre-filled with NaN)
    assert M % 128 != 0
    msg = _fails(got.reshape(N, H, W, Cout), want, match='in the last pixel tile')
    assert f'first at ({N - 1}, {H - 1}, {W - 2}, ' in msg
