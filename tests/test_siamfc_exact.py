"""Exact-operand parity of the SiamFC head kernels (vfs_amd/csrc/xcorr.hip: xcorr_fwd_kernel, xcorr_bwd_z_kernel,
xcorr_bwd_x_kernel, siamfc_loss_kernel, adam_kernel) at the C ABI against float64 references.  The cross-correlation, forward
and backward, and the first Adam step are compared for equality on every element; the probe losses and the later Adam steps
to the bounds derived below.

Operand recipe, cross-correlation.  z and x hold integers (bf16 holds every integer up to 256), drawn per exemplar and per
search image, so that no two exemplars and no two search images are alike and a wrong (m, m % nz) pairing gives another map.
`scale` is a power of two.  The upstream gradient g of the backward holds odd numerators over 4 or 16: non-zero dyadic values
whose products with the integers need more than 8 bits.  Every product is then a multiple of a quantum q (1 forward, 1/4 or
1/16 backward) and every partial sum, in any order and under any contraction, is a multiple of q no larger than the sum of the
absolute products S: with S / q < 2^24 all of them are fp32 values.  Each case asserts that on its own reference (`sums_exact`
on the same correlation / autograd of the absolute operands, `fp32_exact` on the result), so the only correct fp32 response is
the float64 one and the only correct bf16 gradient its round-to-nearest-even (`expect_bf16`).  The reference is
oracle.siamfc_oracle.fast_xcorr in float64 times `scale`, autograd against g for the gradients.  Outputs are pre-filled with
NaN: a vector that is never stored shows.  Where a case is there for the rounding of the bf16 store it asserts, on the
reference alone, that more than 10 % of the exact results are not bf16 values (`rounded_share`), and one case that exact bf16
ties occur in dz and in dx (a truncating or round-half-up store then cannot pass).

Adam, step 1.  b1 = 1/2, b2 = 3/4, lr = 2^-3, eps = 2^k, g + wd p = +-3 2^k, p a multiple of 1/8 that depends on the index:
m = +-3 2^(k-1), v = 9 4^(k-1), sqrt(v) = 3 2^(k-1), bc1 = 1/2, sqrt(1 - b2) = 1/2, the denominator 4 2^k, the quotient
+-3/8, the update +-3/32 - every operation is exact in fp32 (asserted with `fp32_exact` on each intermediate), so p, m and v
are compared for equality.  This needs powf(b, 1.0f) == b in the launcher.  256 NaN-filled guard elements follow the n live
ones in p, m and v and must stay NaN.

Bounded quantities (everything else is equality).  u = 2^-24, the fp32 unit roundoff.

  Probe losses (siamfc_loss_kernel calls expf, log1pf, powf: no single correct fp32 value).  Reference: balanced_loss /
        focal_loss of oracle/siamfc_oracle.py in float64, autograd for the gradient.  The tolerance is a multiple of a
        reference-only measurement: e_l = |loss32 - loss64| and e_g = max |grad32 - grad64| / max |grad64|, where loss32 /
        grad32 are the SAME oracle functions in fp32 on the CPU.  The kernel is allowed |loss - loss64| <= 4 e_l + ulp32(loss64)
        and max |grad - scale grad64| / max |scale grad64| <= 4 e_g + 2^-23 (the same floor in the gradient's own unit: one
        fp32 ulp of its largest element).  The factor covers the device's expf / log1pf / powf (not correctly rounded), the
        block reduction's order, and the kernel's fp32 steps that are not the oracle's (BCE-with-logits in the stable form,
        1 / (1 + exp(-x)) for the sigmoid).  The loss with and without `grad` must agree bit for bit (the order of the
        reduction is fixed), and a power-of-two `scale` must scale the gradient exactly and leave the loss alone.
        (focal, gamma = 2, n = 257, three label values) is the regression case of the kernel's fp32 reductions: with the two
        focal sums in fp32 the loss was 1.84 ulp off where this bound allows 1.64; they are kept in double since.

  Adam, steps 2 to 4 with the default hyper-parameters (b1 = 0.9, b2 = 0.999, lr = 1e-3, eps = 1e-8 as the fp32 values the C
        ABI takes, wd = 0).  Reference: the documented formula in float64, per step from the state the kernel stored before it
        (p0, m0, v0 as doubles) - each stored quantity is held to its own bound, so no error carries from step to step:
          m = fl(fl(b1 m0) + fl((1 - b1) g))                 1 - b is exact for b in [1/2, 1] (Sterbenz), three roundings:
              |m - m64| <= u (|b1 m0| + |(1 - b1) g| + |m64|)
          v = fl(fl(b2 v0) + fl(fl((1 - b2) g) g))           four roundings: |v - v64| <= u (|b2 v0| + 2 (1 - b2) g^2 + |v64|)
          update U = fl(lr / bc1) fl(m / fl(fl(sqrt(v) / bc2s) + eps)) with the STORED m and v (they were just compared):
              bc1 = fl(1 - powf(b1, t)): powf within one ulp (2 u relative) of b1^t, amplified by the subtraction to
                    2 u c1, c1 = b1^t / (1 - b1^t), plus u for the subtraction;
              bc2s = sqrtf(fl(1 - powf(b2, t))): (2 u c2 + u) / 2 through the root, c2 = b2^t / (1 - b2^t), plus one ulp
                    (2 u) for the launcher's sqrtf;
              lr / bc1, sqrt(v) (correctly rounded in the kernel), / bc2s, + eps, m / (.), the product: u each, the terms of the
                    denominator are positive, so their relative errors do not grow.
              |U - U64| <= u (2 c1 + c2 + 9.5) |U64|, and the stored p = fl(p0 - U) adds half an ulp of itself:
              |(p - p0) - (-U64)| <= 1.001 (u (2 c1 + c2 + 9.5) |U64| + u |p0 - U64|)       (1.001: second-order terms)
        c2 is 499 at t = 2: the cancellation in 1 - b2^t is the launcher's and dominates the bound (about 3e-5 of U); the half
        ulp of a correctly rounded powf alone uses up to half of it.  m and v get the factor 1.001 as well.  The worst
        observed fractions are in MEASUREMENTS.md.

The head on the engine's unit path (section 6).  vfs_amd.SiamConvFC holds one engine.ConvUnit per 1x1 conv, and
head_loss_backward_nhwc runs their backward through Engine.conv_bwd.  The test restates the head's forward and backward as
plain library calls in the documented order (conv_fwd per conv; xcorr_fwd, siamfc_loss, xcorr_bwd; per conv conv_wgrad with
packing.wgrad_splits(M, cout, cin), bias_grad, conv_dgrad) on weights it packs itself.  The same kernels on the same operands
with the same split plan give the same bits, so everything is compared with torch.equal: loss, responses, dz, dx, both weight
and both bias gradients, from a non-zero starting .grad.  Shapes: z [2,3,3,C], x [4,5,7,C] - nx = 2 nz, 18 and 140 pixels
against the 128-pixel tile (ragged, one and two blocks); C = 64 -> 64 and 128 -> 64 (cin != cout in the dgrad packing).

Every case takes well under a second on the emulator, so none is marked `gpu` only.
backend=emu: host build through the fiber emulator; backend=gpu: libvfs_hip.so on the MI355X."""
import numpy as np
import pytest
import torch

from oracle import siamfc_oracle as SO
from tests.test_bn_exact import fp32_exact, one_ulp, pm, rounded_share, seed
from tests.test_conv_exact import assert_bits, expect_bf16, ints, is_tie, nan_like
from tests.test_loss_exact import assert_exact

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
CPU = torch.device('cpu')
SHAPE_ERR, ARG_ERR = -1, -3
U = 2.0 ** -24
NHWC = ('image', 'row', 'column', 'channel')
RESP = ('image', 'map', 'row', 'column')


# ---------------------------------------------------------------------------------------------- helpers
def nhwc16(t):
    """NCHW fp32 integers -> NHWC bf16, checked to lose nothing"""
    b = t.permute(0, 2, 3, 1).contiguous().to(BF16)
    assert torch.equal(b.float(), t.permute(0, 2, 3, 1)), 'test bug: an operand is not a bf16 value'
    return b


def sums_exact(quantum, **abs_sums):
    """precondition of an accumulation in any order: the terms are multiples of `quantum` and the sum of their absolute values
    stays below 2^24 quanta, so every partial sum is an fp32 value"""
    for name, s in abs_sums.items():
        worst = float(torch.as_tensor(s).abs().max())
        assert worst / quantum < 2 ** 24, f'test bug: {name}: the absolute terms sum to {worst}, {worst / quantum} quanta - not below 2^24'


def all_distinct(t):
    return all(not torch.equal(t[i], t[j]) for i in range(t.shape[0]) for j in range(i))


def xcorr_operands(g, nz, nx, C, Hz, Wz, H, W, zmax, xmax):
    """NCHW fp32 integers in [-zmax, zmax] / [-xmax, xmax]; every exemplar and every search image its own draw"""
    z, x = ints(g, (nz, C, Hz, Wz), -zmax, zmax), ints(g, (nx, C, H, W), -xmax, xmax)
    assert all_distinct(z) and all_distinct(x), 'test bug: two exemplars or two search images are alike'
    return z, x


def odd_over(g, shape, nmax, den):
    """non-zero dyadic values: odd numerators up to nmax (odd) over den, either sign"""
    return (pm(g, shape) * (2 * ints(g, shape, 0, (nmax - 1) // 2) + 1) / den).contiguous()


def call_raw(be, name, args):
    """the entry point without the checking wrapper -> (return code, error text); tensors of `args` live on the backend's device"""
    lib = be.lib
    assert len(args) == len(lib.protos['vfs_' + name][1])
    rc = lib.cfunc(name)(*[a.data_ptr() if hasattr(a, 'data_ptr') else a for a in args])
    if be.dev.type == 'cuda':
        torch.cuda.synchronize()
    return rc, lib.last_error()


def all_nan(*ts):
    return all(bool(torch.isnan(t.float()).all()) for t in ts)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------- 1. cross-correlation forward
def fwd_reference(z, x, scale):
    ref = SO.fast_xcorr(z.double(), x.double()) * scale
    sums_exact(1.0, products=SO.fast_xcorr(z.double().abs(), x.double().abs()))
    fp32_exact(response=ref)
    return ref


#            tag: nz, nx, C, Hz, Wz, H, W, |z| <=, |x| <=, scale
FWD_CASES = {'rowv3_idle_lanes': (1, 1, 8, 3, 3, 5, 6, 255, 255, 0.5),
             'rowv1_single_lane': (1, 2, 8, 2, 1, 4, 3, 255, 255, 1.0),
             'rowv18_c72': (1, 1, 72, 2, 2, 4, 5, 127, 127, 0.25),
             'rowv195_c520': (1, 1, 520, 2, 3, 3, 5, 63, 63, 2.0 ** -4),
             'rowv128_two_full_trips': (1, 1, 256, 2, 4, 3, 6, 63, 63, 0.5),
             'nx_3nz': (2, 6, 16, 2, 3, 7, 9, 255, 255, 2.0 ** -3),
             'nz3_nx3': (3, 3, 16, 2, 2, 4, 4, 255, 255, 1.0),
             'non_square': (1, 2, 16, 2, 3, 5, 7, 255, 255, 2.0 ** -3),
             'response_1x1': (2, 2, 16, 3, 4, 3, 4, 255, 255, 0.5),
             'outputs_9_ragged_workgroup': (1, 1, 8, 2, 2, 4, 4, 255, 255, 2.0),
             'c2056': (2, 2, 2056, 1, 2, 2, 3, 63, 63, 2.0 ** -5)}


def fwd_edge(tag, nz, nx, C, Hz, Wz, H, W):
    """the property of the shape that the case is there for"""
    rowv, total = Wz * C // 8, nx * (H - Hz + 1) * (W - Wz + 1)
    return {'rowv3_idle_lanes': 1 < rowv < 64, 'rowv1_single_lane': rowv == 1, 'rowv18_c72': rowv == 18 and C % 64 != 0,
            'rowv195_c520': rowv == 195 and rowv // 64 == 3 and rowv % 64 != 0, 'rowv128_two_full_trips': rowv == 128,
            'nx_3nz': nz == 2 and nx == 3 * nz, 'nz3_nx3': nz == nx == 3, 'non_square': Hz != Wz and H != W,
            'response_1x1': Hz == H and Wz == W, 'outputs_9_ragged_workgroup': total % 4 != 0, 'c2056': C // 8 > 256}[tag]


@pytest.mark.parametrize('tag', list(FWD_CASES))
def test_xcorr_fwd(backend, tag):
    nz, nx, C, Hz, Wz, H, W, zmax, xmax, scale = FWD_CASES[tag]
    assert fwd_edge(tag, nz, nx, C, Hz, Wz, H, W), 'test bug: the case no longer reaches the edge it is there for'
    z, x = xcorr_operands(seed(31, list(FWD_CASES).index(tag)), nz, nx, C, Hz, Wz, H, W, zmax, xmax)
    ref = fwd_reference(z, x, scale)
    out = nan_like(ref.shape, CPU, F32)
    backend.hostlib.xcorr_fwd(nhwc16(z), nhwc16(x), out, nz, nx, Hz, Wz, H, W, C, scale, None)
    assert_exact(out, ref.float(), f'xcorr_fwd {tag}', RESP)


@pytest.mark.parametrize('why,nz,nx,C,Hz,Wz,H,W,text', [
    ('C % 8 != 0', 1, 1, 12, 2, 2, 4, 4, 'xcorr: C % 8, filter <= search size'),
    ('nx % nz != 0', 2, 3, 8, 2, 2, 4, 4, 'xcorr: nx must be a multiple of nz'),
    ('filter taller than the search image', 1, 1, 8, 4, 2, 3, 4, 'xcorr: C % 8, filter <= search size'),
    ('filter wider than the search image', 1, 1, 8, 2, 5, 3, 4, 'xcorr: C % 8, filter <= search size')])
def test_xcorr_fwd_refuses(backend, why, nz, nx, C, Hz, Wz, H, W, text):
    """the shape error, and the NaN pre-fill untouched; the output is sized for the largest map any reading of the shape gives"""
    dev = backend.dev
    z, x = torch.ones(nz, Hz, Wz, C, dtype=BF16, device=dev), torch.ones(nx, H, W, C, dtype=BF16, device=dev)
    out = nan_like((nx, 1, H, W), dev, F32)
    assert call_raw(backend, 'xcorr_fwd', (z, x, out, nz, nx, Hz, Wz, H, W, C, 1.0, None)) == (SHAPE_ERR, text), why
    assert all_nan(out)


@pytest.mark.parametrize('tag', ['non_square', 'nx_3nz'])
def test_xcorr_fwd_through_module(backend, tag):
    """vfs_amd.SiamFC on the same integers as NCHW fp32: _nhwc_bf16 and _xcorr"""
    import vfs_amd
    nz, nx, C, Hz, Wz, H, W, zmax, xmax, scale = FWD_CASES[tag]
    z, x = xcorr_operands(seed(32, list(FWD_CASES).index(tag)), nz, nx, C, Hz, Wz, H, W, zmax, xmax)
    ref = fwd_reference(z, x, scale)
    with torch.no_grad():
        got = vfs_amd.SiamFC(out_scale=scale)(z.to(backend.dev), x.to(backend.dev)).cpu()
    assert_exact(got, ref.float(), f'SiamFC {tag}', RESP)


# ---------------------------------------------------------------------------------------------- 2. cross-correlation backward
def bwd_reference(z, x, g, scale, quantum):
    """float64 autograd of fast_xcorr(z, x) * scale against g -> (dz, dx) as NHWC; the same on the absolute operands bounds every
    partial sum"""
    def grads(z, x, g):
        z, x = z.double().requires_grad_(True), x.double().requires_grad_(True)
        (SO.fast_xcorr(z, x) * scale).backward(g.double())
        return z.grad.permute(0, 2, 3, 1).contiguous(), x.grad.permute(0, 2, 3, 1).contiguous()
    az, ax = grads(z.abs(), x.abs(), g.abs())
    sums_exact(quantum * scale, dz=az, dx=ax)
    num = g.double() / quantum
    assert bool((num == num.round()).all()) and bool((num.abs() % 2 == 1).all()), 'test bug: g is not odd numerators over 1 / quantum'
    dz, dx = grads(z, x, g)
    fp32_exact(dz=dz, dx=dx)
    return dz, dx


#            tag: nz, nx, C, Hz, Wz, H, W, |z| <=, |x| <=, numerators of g <=, over, scale, asserted: rounded share of dz, of dx, ties
BWD_CASES = {'nx_3nz_dz_sums_three': (2, 6, 16, 2, 3, 7, 9, 31, 31, 7, 4, 0.5, True, False, False),
             'non_square': (1, 2, 16, 2, 3, 5, 7, 255, 31, 255, 16, 0.25, False, True, True),
             'borders_small_c': (1, 1, 8, 3, 3, 6, 6, 255, 31, 255, 16, 0.5, False, True, False),
             'resp_17x17_two_staging_passes': (1, 1, 8, 2, 2, 18, 18, 31, 31, 7, 4, 1.0, False, False, False),
             'resp_4096_the_limit': (1, 1, 8, 1, 1, 64, 64, 15, 15, 7, 4, 0.5, False, False, False),
             'c2056_second_c8_trip': (2, 2, 2056, 1, 2, 2, 3, 255, 255, 15, 4, 0.25, False, False, False),
             'c72': (1, 3, 72, 3, 2, 5, 4, 15, 15, 7, 4, 0.5, True, False, False)}


def bwd_edge(tag, nz, nx, C, Hz, Wz, H, W):
    n = (H - Hz + 1) * (W - Wz + 1)
    return {'nx_3nz_dz_sums_three': nz == 2 and nx == 6, 'non_square': Hz != Wz and H != W, 'borders_small_c': Hz > 1 and Wz > 1,
            'resp_17x17_two_staging_passes': 256 < n <= 512, 'resp_4096_the_limit': n == 4096, 'c2056_second_c8_trip': C // 8 > 256,
            'c72': C % 64 != 0}[tag]


def bwd_case(tag, salt=0):
    nz, nx, C, Hz, Wz, H, W, zmax, xmax, gmax, den, scale = BWD_CASES[tag][:12]
    assert bwd_edge(tag, nz, nx, C, Hz, Wz, H, W), 'test bug: the case no longer reaches the edge it is there for'
    g = seed(33, list(BWD_CASES).index(tag), salt)
    z, x = xcorr_operands(g, nz, nx, C, Hz, Wz, H, W, zmax, xmax)
    go = odd_over(g, (nx, 1, H - Hz + 1, W - Wz + 1), gmax, den)
    return (nz, nx, Hz, Wz, H, W, C, scale), z, x, go, bwd_reference(z, x, go, scale, 1.0 / den)


def run_bwd(be, dims, z, x, go, want_dz=True, want_dx=True):
    nz, nx, Hz, Wz, H, W, C, scale = dims
    dz = nan_like((nz, Hz, Wz, C), CPU) if want_dz else None
    dx = nan_like((nx, H, W, C), CPU) if want_dx else None
    be.hostlib.xcorr_bwd(nhwc16(z), nhwc16(x), go, dz, dx, nz, nx, Hz, Wz, H, W, C, scale, None)
    return dz, dx


@pytest.mark.parametrize('tag', list(BWD_CASES))
def test_xcorr_bwd(backend, tag):
    """dz and dx == the bf16 rounding of the float64 gradient.  dx covers the four borders and corners of every shape (only part
    of the (u, v) window is valid there; assert_bits says whether the mismatches lie on the border)"""
    rounds_dz, rounds_dx, ties = BWD_CASES[tag][12:]
    dims, z, x, go, (rz, rx) = bwd_case(tag)
    sz, sx = rounded_share(rz), rounded_share(rx)
    tz, tx = float(is_tie(rz).double().mean()), float(is_tie(rx).double().mean())
    print(f'xcorr_bwd {tag}: not bf16 values: dz {sz:.3f} (ties {tz:.3f}), dx {sx:.3f} (ties {tx:.3f})')
    if rounds_dz:
        assert sz > 0.10, 'test bug: the rounding of the stored dz is hardly exercised'
    if rounds_dx:
        assert sx > 0.10, 'test bug: the rounding of the stored dx is hardly exercised'
    if ties:
        assert bool(is_tie(rz).any()) and bool(is_tie(rx).any()), 'test bug: no exact bf16 tie in the reference'
    dz, dx = run_bwd(backend, dims, z, x, go)
    assert_bits(dz, expect_bf16(rz), f'xcorr_bwd {tag}: dz')
    assert_bits(dx, expect_bf16(rx), f'xcorr_bwd {tag}: dx')


@pytest.mark.parametrize('which', ['dx_only', 'dz_only'])
def test_xcorr_bwd_single_output(backend, which):
    """dz = NULL or dx = NULL: the other gradient is written and is correct.  8-bit operands on both sides: more than 10 % of
    either exact gradient is no bf16 value"""
    dims, z, x, go, (rz, rx) = bwd_case('non_square', salt=1)
    if which == 'dx_only':
        assert rounded_share(rx) > 0.10, 'test bug: the rounding of the stored dx is hardly exercised'
        dz, dx = run_bwd(backend, dims, z, x, go, want_dz=False)
        assert dz is None
        assert_bits(dx, expect_bf16(rx), 'xcorr_bwd without dz: dx')
    else:
        assert rounded_share(rz) > 0.10, 'test bug: the rounding of the stored dz is hardly exercised'
        dz, dx = run_bwd(backend, dims, z, x, go, want_dx=False)
        assert dx is None
        assert_bits(dz, expect_bf16(rz), 'xcorr_bwd without dx: dz')


def test_xcorr_bwd_refuses_4097_responses(backend):
    """17 x 241 = 4097 response elements: one past the staging buffer.  The shape error and nothing written; every buffer has its
    full size, so a launch that was wrongly accepted would stay in bounds"""
    dev = backend.dev
    nz = nx = Hz = Wz = 1
    H, W, C = 17, 241, 8
    assert (H - Hz + 1) * (W - Wz + 1) == 4097
    z, x = torch.ones(nz, Hz, Wz, C, dtype=BF16, device=dev), torch.ones(nx, H, W, C, dtype=BF16, device=dev)
    go = torch.ones(nx, 1, H, W, device=dev)
    dz, dx = nan_like(z.shape, dev), nan_like(x.shape, dev)
    got = call_raw(backend, 'xcorr_bwd', (z, x, go, dz, dx, nz, nx, Hz, Wz, H, W, C, 1.0, None))
    assert got == (SHAPE_ERR, 'xcorr_bwd: response map larger than 4096 elements')
    assert all_nan(dz, dx)


# ---------------------------------------------------------------------------------------------- 3. probe losses
LABELS = ('three_values', 'no_positive', 'no_negative', 'all_positive')
LOSS_MODES = [(0, 0.5), (0, 1.0), (1, 1.0), (1, 1.5), (1, 2.0)]      # (mode, neg_weight | gamma)
LOSS_SCALE = 0.25


def loss_operands(n, labels):
    """logits N(0, 3^2) with +-30 on the first elements of every label value; labels drawn per element"""
    g = seed(34, n, LABELS.index(labels))
    x = (torch.randn(n, generator=g) * 3).float()
    r = torch.rand(n, generator=g)
    t = {'three_values': torch.where(r < 0.2, 1.0, torch.where(r < 0.5, 0.5, 0.0)), 'no_positive': torch.where(r < 0.4, 0.5, 0.0),
         'no_negative': torch.where(r < 0.4, 1.0, 0.5), 'all_positive': torch.ones(n)}[labels].float()
    for value in t.unique():
        idx = (t == value).nonzero()[:, 0]
        assert idx.numel() >= 4
        x[idx[0]], x[idx[1]] = 30.0, -30.0
    present = set(t.unique().tolist())
    assert present == {'three_values': {0.0, 0.5, 1.0}, 'no_positive': {0.0, 0.5}, 'no_negative': {0.5, 1.0}, 'all_positive': {1.0}}[labels]
    return x, t


def loss_oracle(x, t, mode, param, dtype):
    x = x.detach().clone().to(dtype).requires_grad_(True)
    loss = SO.balanced_loss(x, t.to(dtype), param) if mode == 0 else SO.focal_loss(x, t.to(dtype), param)
    loss.backward()
    return loss.detach().double(), x.grad.double()


@pytest.mark.parametrize('labels', LABELS)
@pytest.mark.parametrize('n', [100, 256, 257, 1000])
@pytest.mark.parametrize('mode,param', LOSS_MODES)
def test_siamfc_loss(backend, mode, param, n, labels):
    """bounds: 4 x the error of the fp32 oracle against the float64 oracle plus one fp32 ulp (module docstring)"""
    lib = backend.hostlib
    x, t = loss_operands(n, labels)
    l64, g64 = loss_oracle(x, t, mode, param, F64)
    l32, g32 = loss_oracle(x, t, mode, param, F32)
    assert bool(torch.isfinite(l64)) and bool(torch.isfinite(g64).all()) and bool(torch.isfinite(l32)) and bool(torch.isfinite(g32).all())
    gmax = float(g64.abs().max())
    e_l, e_g = float((l32 - l64).abs()), float((g32 - g64).abs().max()) / gmax
    tol_l = 4 * e_l + float(one_ulp(l64.float().double()))
    tol_g = 4 * e_g + 2.0 ** -23

    loss, grad = nan_like((1,), CPU, F32), nan_like((n,), CPU, F32)
    lib.siamfc_loss(x, t, loss, grad, n, mode, param, 1.0, None)
    loss_only = nan_like((1,), CPU, F32)
    lib.siamfc_loss(x, t, loss_only, None, n, mode, param, 1.0, None)
    loss_s, grad_s = nan_like((1,), CPU, F32), nan_like((n,), CPU, F32)
    lib.siamfc_loss(x, t, loss_s, grad_s, n, mode, param, LOSS_SCALE, None)

    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
    d_l, d_g = float((loss.double()[0] - l64).abs()), float((grad.double() - g64).abs().max()) / gmax
    print(f'siamfc_loss mode {mode} param {param} n {n} {labels}: loss {float(l64):.6f} fp32 oracle off {e_l:.3e} kernel off {d_l:.3e} '
          f'({d_l / tol_l:.2f} of the bound); grad / max|grad| fp32 oracle off {e_g:.3e} kernel off {d_g:.3e} ({d_g / tol_g:.2f} of the bound)')
    assert d_l <= tol_l, f'loss {float(loss)} against {float(l64)}: off by {d_l}, allowed {tol_l} (fp32 oracle: {e_l})'
    assert d_g <= tol_g, f'gradient off by {d_g} of its largest element, allowed {tol_g} (fp32 oracle: {e_g})'
    assert same_bits(loss_only, loss), 'the loss without grad differs from the loss with grad'
    assert same_bits(loss_s, loss), 'scale changes the loss'
    assert same_bits(grad_s, grad * LOSS_SCALE), 'a power-of-two scale does not scale the gradient exactly'


@pytest.mark.parametrize('n,mode', [(0, 0), (0, 1), (8, 2), (8, -1)])
def test_siamfc_loss_refuses(backend, n, mode):
    dev = backend.dev
    x, t = torch.zeros(8, device=dev), torch.ones(8, device=dev)
    loss, grad = nan_like((1,), dev, F32), nan_like((8,), dev, F32)
    got = call_raw(backend, 'siamfc_loss', (x, t, loss, grad, n, mode, 1.0, 1.0, None))
    assert got == (ARG_ERR, 'siamfc_loss: n >= 1, mode 0 (balanced) or 1 (focal)')
    assert all_nan(loss, grad)


# ---------------------------------------------------------------------------------------------- 4. Adam
GUARD = 256


def guarded(live):
    """[n] values followed by GUARD NaNs"""
    return torch.cat([live.float(), torch.full((GUARD,), float('nan'))]).contiguous()


@pytest.mark.parametrize('wd', [0.0, 0.25])
@pytest.mark.parametrize('k', [-3, 0, 5])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 1000])
def test_adam_first_step_exact(backend, n, k, wd):
    """the recipe of the module docstring: p, m and v of one step for equality, the guard untouched"""
    b1, b2, lr, eps = 0.5, 0.75, 2.0 ** -3, 2.0 ** k
    i = torch.arange(n, dtype=torch.int64)
    p0 = ((i * 7) % 129 - 64).double() / 8                              # multiples of 1/8 in [-8, 8]
    sign = (1 - 2 * ((i * 5 + i // 3) % 2)).double()
    geff = sign * 3 * 2.0 ** k                                          # g + wd p
    g0 = geff - wd * p0
    m64, v64 = (1 - b1) * geff, (1 - b2) * geff * geff
    root, bc1, bc2s = v64.sqrt(), 1 - b1, np.sqrt(1 - b2)
    den = root / bc2s + eps
    quot = m64 / den
    upd = (lr / bc1) * quot
    p64 = p0 - upd
    fp32_exact(p0=p0, g=g0, wd_p=wd * p0, g_eff=geff, m=m64, g2=geff * geff, v=v64, root=root, over_bc2s=root / bc2s, den=den,
               quot=quot, step=lr / bc1, upd=upd, p=p64, bc1=bc1, bc2s=bc2s)
    assert torch.equal(den, torch.full_like(den, 4 * 2.0 ** k)) and torch.equal(upd, sign * 3 / 32)
    p, gr, m, v = guarded(p0), guarded(g0), guarded(torch.zeros(n)), guarded(torch.zeros(n))
    backend.hostlib.adam_step(p, gr, m, v, n, lr, b1, b2, eps, wd, 1, None)
    what = f'adam_step n={n} eps=2^{k} wd={wd}'
    assert_exact(m[:n], m64.float(), what + ': m', ('element',))
    assert_exact(v[:n], v64.float(), what + ': v', ('element',))
    assert_exact(p[:n], p64.float(), what + ': p', ('element',))
    assert all_nan(p[n:], m[n:], v[n:]), what + ': the guard past n was written'
    assert_exact(gr[:n], g0.float(), what + ': g (an input)', ('element',))


@pytest.mark.parametrize('n', [257, 1000])
def test_adam_default_steps_bound(backend, n):
    """steps 2 to 4 after a first one, default hyper-parameters: m, v and the update p_after - p_before against the float64
    formula from the stored state, to the bounds of the module docstring"""
    f = lambda a: float(np.float32(a))      # noqa: E731  the C ABI takes floats
    b1, b2, lr, eps = f(0.9), f(0.999), f(1e-3), f(1e-8)
    gen = seed(35, n)
    p = guarded(torch.randn(n, generator=gen) * 0.01)
    m, v = guarded(torch.zeros(n)), guarded(torch.zeros(n))
    worst = dict(m=0.0, v=0.0, update=0.0)
    for t in range(1, 5):
        gr = guarded(torch.randn(n, generator=gen))
        p0, m0, v0, g = p[:n].double(), m[:n].double(), v[:n].double(), gr[:n].double()
        backend.hostlib.adam_step(p, gr, m, v, n, lr, b1, b2, eps, 0.0, t, None)
        assert all_nan(p[n:], m[n:], v[n:])
        if t == 1:
            continue
        m64 = b1 * m0 + (1 - b1) * g
        v64 = b2 * v0 + (1 - b2) * g * g
        bound_m = 1.001 * U * ((b1 * m0).abs() + ((1 - b1) * g).abs() + m64.abs())
        bound_v = 1.001 * U * (b2 * v0 + 2 * (1 - b2) * g * g + v64)
        ms, vs = m[:n].double(), v[:n].double()                      # the stored state: what the update is formed from
        u64 = lr / (1 - b1 ** t) * ms / (vs.sqrt() / np.sqrt(1 - b2 ** t) + eps)
        c1, c2 = b1 ** t / (1 - b1 ** t), b2 ** t / (1 - b2 ** t)
        bound_u = 1.001 * (U * (2 * c1 + c2 + 9.5) * u64.abs() + U * (p0 - u64).abs())
        for name, err, bound in (('m', (ms - m64).abs(), bound_m), ('v', (vs - v64).abs(), bound_v),
                                 ('update', ((p[:n].double() - p0) + u64).abs(), bound_u)):
            frac = float((err / bound).max())
            worst[name] = max(worst[name], frac)
            assert bool((err <= bound).all()), f'adam_step n={n} step {t}: {name} is off by up to {frac} of the bound'
    print(f'adam_step n={n}, steps 2-4: worst error / bound m {worst["m"]:.3f}, v {worst["v"]:.3f}, update {worst["update"]:.3f}')


def test_adam_refuses_step_0(backend):
    dev = backend.dev
    p, m, v = (nan_like((8,), dev, F32) for _ in range(3))
    g = torch.ones(8, device=dev)
    assert call_raw(backend, 'adam_step', (p, g, m, v, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None)) == (ARG_ERR, 'adam_step: step >= 1')
    assert all_nan(p, m, v)


# ---------------------------------------------------------------------------------------------- 5. head_loss_backward
class NoLaunch:
    def __getattr__(self, name):
        raise AssertionError(f'{name} was reached before the label count was checked')


@pytest.mark.parametrize('head_type', ['SiamFC', 'SiamConvFC'])
def test_head_loss_backward_refuses_labels_of_another_size(backend, head_type):
    """labels built for another response size would be read past their end by the loss kernel: ValueError before any launch"""
    import vfs_amd
    from vfs_amd import siamfc as SF
    dev = backend.dev
    head = (vfs_amd.SiamFC() if head_type == 'SiamFC' else vfs_amd.SiamConvFC(64, 64)).to(dev)
    zf, xf = torch.ones(2, 64, 3, 2, device=dev), torch.ones(4, 64, 6, 7, device=dev)          # responses [4, 1, 4, 6]
    good = SF.create_labels((4, 1, 4, 6), 16, 0, 8, dev)
    lib = backend.eng.lib
    backend.eng.lib = NoLaunch()
    try:
        for size in ((4, 1, 4, 5), (2, 1, 4, 6), (4, 1, 5, 6)):
            with pytest.raises(ValueError, match='labels'):
                SF.head_loss_backward(head, zf, xf, SF.create_labels(size, 16, 0, 8, dev), 'balance', backward=False)
    finally:
        backend.eng.lib = lib
    loss, resp = SF.head_loss_backward(head, zf, xf, good, 'balance', backward=False)      # the right count passes
    assert tuple(resp.shape) == (4, 1, 4, 6) and bool(torch.isfinite(loss).all())


# ---------------------------------------------------------------------------------------------- 6. the head on the engine's unit path
HEAD_SCALE = 0.01
SIDES = ('z', 'x')


def head_operands(cin, cout):
    """features z [2,3,3,cin] / x [4,5,7,cin] NHWC bf16, labels for the [4,1,3,5] responses, and per side (weight, bias) with the
    (weight, bias) gradients the backward starts from; cout = None: no convs (SiamFC)"""
    from vfs_amd import siamfc as SF
    g = seed(36, cin, cout or 0)
    z, x = torch.randn(2, 3, 3, cin, generator=g).to(BF16), torch.randn(4, 5, 7, cin, generator=g).to(BF16)
    labels = SF.create_labels((4, 1, 3, 5), 16, 0, 8, CPU)
    assert set(labels.unique().tolist()) == {0.0, 1.0}, 'test bug: the labels lack a class'
    if cout is None:
        return z, x, labels, None, None
    weights = {side: (torch.randn(cout, cin, 1, 1, generator=g) * 0.1, torch.randn(cout, generator=g) * 0.1) for side in SIDES}
    start = {side: (torch.randn(cout, cin, 1, 1, generator=g), torch.randn(cout, generator=g)) for side in SIDES}
    return z, x, labels, weights, start


def head_direct(be, z, x, labels, weights, start, loss):
    """the head's forward and backward as plain library calls -> dict of CPU tensors"""
    from tests.test_emu_conv import pack
    from vfs_amd.packing import wgrad_splits
    lib = be.hostlib
    feats, conv, wds = dict(z=z, x=x), dict(z=z, x=x), {}
    for side in SIDES if weights is not None else ():
        w, b = weights[side]
        wf, wds[side] = (t.cpu() for t in pack(be, w))
        n, h, wi, cin = feats[side].shape
        conv[side] = nan_like((n, h, wi, w.shape[0]), CPU)
        lib.conv_fwd(feats[side], wf, conv[side], b, None, n, h, wi, cin, h, wi, w.shape[0], 1, 1, 1, 0, None)
    zc, xc = conv['z'], conv['x']
    nz, hz, wz, c = zc.shape
    nx, h, w, _ = xc.shape
    out = dict(resp=nan_like((nx, 1, h - hz + 1, w - wz + 1), CPU, F32), loss=nan_like((1,), CPU, F32))
    lib.xcorr_fwd(zc, xc, out['resp'], nz, nx, hz, wz, h, w, c, HEAD_SCALE, None)
    g = nan_like(out['resp'].shape, CPU, F32)
    mode = {'balance': 0, 'focal': 1}[loss]
    lib.siamfc_loss(out['resp'], labels, out['loss'], g, g.numel(), mode, 1.0 if mode == 0 else 2.0, 1.0, None)
    d = dict(z=nan_like(zc.shape, CPU), x=nan_like(xc.shape, CPU))
    lib.xcorr_bwd(zc, xc, g, d['z'], d['x'], nz, nx, hz, wz, h, w, c, HEAD_SCALE, None)
    for side in SIDES:
        if weights is None:
            out['d' + side] = d[side]
            continue
        n, hh, ww, cin = feats[side].shape
        M, cout = n * hh * ww, weights[side][0].shape[0]
        nsplit, pps = wgrad_splits(M, cout, cin)
        gw, gb = (t.clone() for t in start[side])
        lib.conv_wgrad(d[side], feats[side], nan_like((nsplit * cout * cin,), CPU, F32), gw, n, hh, ww, cin, hh, ww, cout, 1, 1, 1, 0,
                       nsplit, pps, None)
        lib.bias_grad(d[side], gb, M, cout, None)
        out['d' + side] = nan_like(feats[side].shape, CPU)
        lib.conv_dgrad(d[side], wds[side], out['d' + side], None, n, hh, ww, cin, hh, ww, cout, 1, 1, 1, 0, None)
        out[side + '.weight.grad'], out[side + '.bias.grad'] = gw, gb
    return out


_HEAD_REFS = {}


def head_reference(be, cin, cout, loss):
    """(operands, head_direct's result), computed once per backend and case"""
    key = (be.name, cin, cout, loss)
    if key not in _HEAD_REFS:
        ops = head_operands(cin, cout)
        _HEAD_REFS[key] = (ops, head_direct(be, *ops, loss))
    return _HEAD_REFS[key]


def head_module(be, cin, cout, weights, start):
    """vfs_amd.SiamConvFC (SiamFC for cout = None) holding `weights`, every .grad at its `start` value"""
    import vfs_amd
    if cout is None:
        return vfs_amd.SiamFC(out_scale=HEAD_SCALE)
    head = vfs_amd.SiamConvFC(cin, cout, out_scale=HEAD_SCALE)
    with torch.no_grad():
        for side in SIDES:
            conv = getattr(head, side + '_convs')[0]
            conv.weight.copy_(weights[side][0])
            conv.bias.copy_(weights[side][1])
    head.to(be.dev)
    for side in SIDES:
        conv = getattr(head, side + '_convs')[0]
        conv.weight.grad, conv.bias.grad = (t.clone().to(be.dev) for t in start[side])
    return head


def head_engine(be, head, z, x, labels, loss):
    """head_loss_backward_nhwc(feat_grads=True) -> the dict head_direct returns"""
    from vfs_amd import siamfc as SF
    dev = be.dev
    loss_t, resp, dz, dx = SF.head_loss_backward_nhwc(head, z.to(dev), x.to(dev), labels.to(dev), loss, feat_grads=True)
    out = dict(loss=loss_t, resp=resp, dz=dz, dx=dx)
    for side in SIDES if hasattr(head, 'z_convs') else ():
        conv = getattr(head, side + '_convs')[0]
        out[side + '.weight.grad'], out[side + '.bias.grad'] = conv.weight.grad, conv.bias.grad
    return {k: v.cpu() for k, v in out.items()}


def assert_same(got, want, what, skip=()):
    assert sorted(got) == sorted(want)
    for k in want:
        if k not in skip:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), f'{what}: {k} differs from the direct launches'
    assert bool(torch.isfinite(torch.cat([v.float().flatten() for v in want.values()])).all()), 'test bug: the reference is not finite'


@pytest.mark.parametrize('loss', ['balance', 'focal'])
@pytest.mark.parametrize('cin,cout', [(64, 64), (128, 64), (64, None)], ids=['c64_64', 'c128_64', 'no_convs'])
def test_head_backward_equals_direct_launches(backend, cin, cout, loss):
    (z, x, labels, weights, start), want = head_reference(backend, cin, cout, loss)
    if start is not None:
        assert all(not torch.equal(want[s + k], start[s][i]) for s in SIDES for i, k in enumerate(('.weight.grad', '.bias.grad'))), \
            'test bug: a gradient did not move from its starting value'
    got = head_engine(backend, head_module(backend, cin, cout, weights, start), z, x, labels, loss)
    assert_same(got, want, f'head {cin} -> {cout} {loss}')


def test_head_backward_frozen_conv(backend):
    """x_convs[0].weight.requires_grad = False: its .grad is left alone, every other result is what the direct launches give"""
    (z, x, labels, weights, start), want = head_reference(backend, 64, 64, 'focal')
    head = head_module(backend, 64, 64, weights, start)
    head.x_convs[0].weight.requires_grad_(False)
    kept = head.x_convs[0].weight.grad
    got = head_engine(backend, head, z, x, labels, 'focal')
    assert head.x_convs[0].weight.grad is kept and torch.equal(got['x.weight.grad'], start['x'][0])
    assert_same(got, want, 'head with a frozen x conv', skip=('x.weight.grad',))


class CountPacks:
    """the engine's library with vfs_pack_weights launches counted"""

    def __init__(self, lib):
        self._lib, self.packs = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != 'pack_weights':
            return fn

        def counted(*args):
            self.packs += 1
            return fn(*args)
        return counted


def test_head_packs_once_per_epoch(backend):
    """one pack launch per conv and parameter epoch; one more, once, when the first backward asks for the dgrad packing"""
    from vfs_amd.engine import bump_params_epoch
    (z, x, labels, weights, start), _ = head_reference(backend, 64, 64, 'focal')
    head = head_module(backend, 64, 64, weights, start)
    zf, xf = (t.float().permute(0, 3, 1, 2).to(backend.dev) for t in (z, x))
    lib = backend.eng.lib
    backend.eng.lib = count = CountPacks(lib)
    try:
        with torch.no_grad():
            head(zf, xf)
            head(zf, xf)
        head_engine(backend, head, z, x, labels, 'focal')
        assert 2 <= count.packs <= 4, count.packs      # two convs: wf each, and at most one repack each for wd
        seen = count.packs
        with torch.no_grad():
            head(zf, xf)
        head_engine(backend, head, z, x, labels, 'focal')
        assert count.packs == seen, 'a repack within one parameter epoch'
        bump_params_epoch()
        with torch.no_grad():
            head(zf, xf)
        head_engine(backend, head, z, x, labels, 'focal')
        assert count.packs == seen + 2, 'not exactly one pack launch per conv after the epoch moved'
    finally:
        backend.eng.lib = lib


@pytest.mark.parametrize('name', ['Adam', 'ParamSGD'])
def test_probe_optimizer_state(backend, name):
    """two steps on two tensors: state_dict keys and values, and the parameters, equal a loop of adam_step / sgd_step launches"""
    from vfs_amd import siamfc as SF
    from vfs_amd.engine import params_epoch
    g = seed(37)
    dev, lib = backend.dev, backend.hostlib
    init = [torch.randn(5, 3, generator=g), torch.randn(7, generator=g)]
    grads = [[torch.randn(p.shape, generator=g) for p in init] for _ in range(2)]
    params = [torch.nn.Parameter(p.clone().to(dev)) for p in init]
    if name == 'Adam':
        hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1)
        want_state = [dict(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p)) for p in init]
    else:
        hyper = dict(lr=0.1, momentum=0.9, weight_decay=5e-4)
        want_state = [dict(momentum_buffer=torch.zeros_like(p)) for p in init]
    opt = getattr(SF, name)(params, **hyper)
    want = [p.clone() for p in init]
    epoch = params_epoch()
    for step in range(2):
        for p, gr in zip(params, grads[step]):
            p.grad = gr.clone().to(dev)
        opt.step()
        for p, gr, st in zip(want, grads[step], want_state):
            if name == 'Adam':
                st['step'] += 1
                lib.adam_step(p, gr, st['exp_avg'], st['exp_avg_sq'], p.numel(), hyper['lr'], *hyper['betas'], hyper['eps'],
                              hyper['weight_decay'], st['step'], None)
            else:
                lib.sgd_step(p, gr, st['momentum_buffer'], p.numel(), hyper['lr'], hyper['momentum'], hyper['weight_decay'], None, None)
    assert params_epoch() == epoch + 2      # every step tells the caches of derived weights
    sd = opt.state_dict()
    assert sorted(sd) == ['param_groups', 'state'] and sorted(sd['state']) == [0, 1]
    assert len(sd['param_groups']) == 1 and sd['param_groups'][0]['params'] == [0, 1]
    assert {k: sd['param_groups'][0][k] for k in hyper} == hyper
    for i, st in enumerate(want_state):
        assert list(sd['state'][i]) == list(st)
        for k, v in st.items():
            got = sd['state'][i][k]
            assert (got == v) if k == 'step' else torch.equal(got.cpu(), v), (i, k)
        assert torch.equal(params[i].detach().cpu(), want[i]), i
