"""Exact-operand parity of the BatchNorm, stem-pooling and small reduction kernels (csrc/bn.hip, vfs_stem.h, the pooling and
bias-gradient kernels of csrc/misc.hip) against a float64 reference computed from the definitions in include/vfs_hip.h: every
stored value is compared for equality; the one toleranced quantity is running_var (below).

The kernels read bf16 tensors and fp32 parameters and compute in fp32 (the row reductions in fp64).  With integer tensors and
dyadic parameters every product, partial sum and coefficient they form is fp32-representable whatever the summation order, the
FMA contraction or the slab walk, so the only correct fp32 output is the exact value and the only correct bf16 output its
round-to-nearest-even.  Each case asserts that precondition on its own data before it calls a kernel (`fp32_exact`).

Regimes:
  apply (vfs_bn_act / _mask)   x, res, rres integers in [-255, 255], scale / rscale in +-{1/2, 1, 2}, shift / rshift in eighths:
               x scale + shift + res + rres rscale + rshift is a multiple of 1/8 below 2^11 (14 bits) - exact in fp32, mostly NOT
               bf16-representable, so the stored value must be its RNE rounding; the mask must be that of the reference y.  A
               constructed block in which EVERY fp32 value is an exact bf16 tie (+-(257 + 2 j)) separates RNE from truncation,
               round-half-away and round-half-up.
  backward     g in [-4, 4], x in [-8, 8], a ~45 % mask (stored y, bit-packed, or recomputed from x scale + shift), scale in
               +-{1/2, 1, 2}, invstd in {1/4, 1/2, 1, 2}, mean in halves in [-4, 4]; count a power of two (its own argument), so
               (float)(1 / count) is exact.  S1 = sum g mask and S2 = sum g mask xhat are sums of multiples of 1/8; m1, m2,
               B = -scale invstd m2, D = scale (mean invstd m2 - m1), B x + D and dx = scale (g mask - m1 - xhat m2) all
               round-trip through fp32 (asserted).  vfs_bn_bwd_apply / _apply_fin / vfs_stem_pool_bn_bwd_apply get integer sums
               in [-2 count, 2 count] (directly, or as integer partial rows that add up to them): m1, m2 are multiples of
               1 / count in [-2, 2], and most dx values need more than bf16's eight bits.  vfs_bn_bwd_apply_raw and the row
               kernels form S1 / S2 from the tensors themselves.
  statistics   per channel half the rows of a group hold m + s, half m - s (shuffled), m an integer, s in {1/2, 1, 2, 4}; eps = 0,
               count = mpg = a power of two: mean = m, var = s^2, invstd = 1 / s, scale = gamma / s and shift = beta - m scale are
               exact, as is running_mean (momentum 1/4, start in quarters).  running_var multiplies by count / (count - 1): the
               kernel's fp64 expression is reproduced and ONE fp32 ulp of the expected value is allowed (double rounding of an
               emulated fmaf) - the only tolerance in this file.
  reductions   integer fp32 rows: the fp64 column sums, and the `+=` of their fp32 cast onto integer dgamma / dbeta, are exact.
  stem pool    (one case apart, test_stem_maxpool_pools_the_stored_bf16_activation, rounds the activation: taps that differ in
               fp32 and agree in bf16.)  x in [-6, 6], scale in +-{1/2, 1, 2}, shift in halves: bf16(relu(x scale + shift)) is a small
               multiple of 1/2, equal activations inside a window are the rule, and the code must be the FIRST maximum in
               ascending tap order k = 3 dy + dx (0xFF where the pooled value is not positive).  Gradients gp in [-4, 4]: ga (up
               to four windows) and every partial sum are small exact numbers.
Every group gets parameters of its own, so that a wrong group index shows.  Outputs are pre-filled with NaN (0xAA for bytes).

Geometry: GEOMS are the smallest (G, mpg, C) that reach each branch of slab_geom / slab_grid and of the four-row trips; WIDE
run the >= 128-channel streaming slabs (`bn_wide_min_mb` = 0) and, with the option at its default, the 64-channel slabs.

Not covered here: vfs_linear_bn_act and the _xchg entry points (statistics out of a GEMM / two processes), and
vfs_stem_wgrad_fused (left to its existing chain-against-chain test).

backend=emu: host build through the fiber emulator; backend=gpu: libvfs_hip.so on the MI355X."""
import contextlib
import ctypes

import pytest
import torch

from tests.emu_util import pack_relu_mask
from tests.test_conv_exact import assert_bits, expect_bf16, ints, is_tie, nan_like

BF16 = torch.bfloat16
F64 = torch.float64
CPU = torch.device('cpu')

#        (G, mpg, C)         what it reaches
GEOMS = [(2, 300, 64),     # three blocks per group, ragged last block and trip
         (3, 130, 192),    # three slabs
         (2, 1030, 8),     # second block at C = 8
         (1, 260, 32),     # second block at C = 32
         (2, 9, 2048),     # many slabs, tiny group
         (2, 1, 64)]       # single-pixel group
WIDE = [(2, 100, 128), (2, 72, 256), (1, 50, 512), (2, 20, 1024)]
SLABS = [(g, False) for g in GEOMS + WIDE] + [(g, True) for g in WIDE]
SLAB_IDS = [f'{G}x{mpg}x{C}{"-wide" if w else ""}' for (G, mpg, C), w in SLABS]


# ---------------------------------------------------------------------------------------------- helpers
def option(lib, name):
    """current value of an A/B knob (csrc/vfs_options.h: the process-global int behind vfs_set_option)"""
    return ctypes.c_int.in_dll(lib.dll, 'vfs_option_' + name).value


def slab_wide_ok(C):
    """mirror of bn.hip slab_wide_ok: the channel counts the streaming slabs take"""
    return C >= 128 and (((512 % C == 0 or C % 64 == 0) and 256 % (C >> 3) == 0) if C <= 512 else C % 512 == 0)


@contextlib.contextmanager
def wide_slabs(lib, on, C=0):
    """on: `bn_wide_min_mb` = 0 - the plain launches stream whole pixel rows on >= 128 channels whatever the tensor size; the
    previous value comes back afterwards.  Asserts what the launcher's choice depends on besides: `bn_wide` on, C a streaming
    width.  off: nothing is touched, and the (small) tensors of this file must be below the threshold in force."""
    if not on:
        assert option(lib, 'bn_wide_min_mb') >= 8, 'the narrow cases of this file need the streaming threshold above their tensor sizes'
        yield
        return
    assert option(lib, 'bn_wide') == 1 and slab_wide_ok(C), 'test bug: this case would not take the streaming slabs'
    before = option(lib, 'bn_wide_min_mb')
    lib.set_option(b'bn_wide_min_mb', 0)
    try:
        assert option(lib, 'bn_wide_min_mb') == 0
        yield
    finally:
        lib.set_option(b'bn_wide_min_mb', before)


def fp32_exact(**vals):
    """precondition: every named intermediate round-trips through fp32"""
    for name, v in vals.items():
        v = torch.as_tensor(v, dtype=F64)
        assert torch.equal(v.float().double(), v), f'test bug: {name} does not round-trip through fp32'


def bf16_exact(**vals):
    for name, v in vals.items():
        assert torch.equal(v.to(BF16).double(), v.double()), f'test bug: {name} is not bf16-representable'


def rounded_share(t64):
    """share of the values that bf16 cannot hold"""
    return float((expect_bf16(t64).double() != t64).double().mean())


def pow2(g, shape, lo, hi):
    return 2.0 ** ints(g, shape, lo, hi)


def pm(g, shape):
    return ints(g, shape, 0, 1) * 2 - 1


def rows_of(p, mpg):
    """[G][C] parameter -> [G * mpg][C], one row per pixel"""
    return p.repeat_interleave(mpg, 0)


def bytes_like(n):
    return torch.full((n,), 0xAA, dtype=torch.uint8)


def bwd_params(g, G, C):
    """bnp [G][4][C] = {scale, shift, mean, invstd}: dyadic, different in every group; scale is NOT gamma * invstd here - the
    backward kernels take the four rows as given"""
    scale = pm(g, (G, C)) * pow2(g, (G, C), -1, 1)
    shift = ints(g, (G, C), -8, 8) / 2
    mean = ints(g, (G, C), -8, 8) / 2
    inv = pow2(g, (G, C), -2, 1)
    return torch.stack([scale, shift, mean, inv], 1).contiguous()


def bwd_operands(g, G, mpg, C):
    M = G * mpg
    return ints(g, (M, C), -4, 4), ints(g, (M, C), -8, 8), bwd_params(g, G, C)


def mask_modes(g, x, bnp, mpg):
    """(name, y operand, relu argument, float64 mask [M][C]): stored activation, its bit-packed mask, recomputed from x"""
    M, C = x.shape
    ysrc = ints(g, (M, C), -3, 3)
    stored = (ysrc > 0).double()
    recomputed = ((x.double() * rows_of(bnp[:, 0], mpg).double() + rows_of(bnp[:, 1], mpg).double()) > 0).double()
    for m in (stored, recomputed):
        assert 0.2 < float(m.mean()) < 0.8
    return [('stored y', ysrc.to(BF16), 0, stored), ('bit-packed mask', pack_relu_mask(ysrc), 2, stored),
            ('mask from x scale + shift', None, 1, recomputed), ('no mask', None, 0, torch.ones(M, C, dtype=F64))]


def row_terms(gy, x, mask, bnp, mpg):
    """the two summands of the backward statistics per element, float64 [M][C]: g mask and g mask xhat"""
    t1 = gy.double() * mask
    xhat = (x.double() - rows_of(bnp[:, 2], mpg).double()) * rows_of(bnp[:, 3], mpg).double()
    t2 = t1 * xhat
    fp32_exact(xhat=xhat, g_mask_xhat=t2)
    return t1, t2


def block_sums(t1, t2, ppb):
    """[M / ppb][2][C] float64 sums over linear pixel ranges; asserts that every partial sum in any order is representable"""
    M, C = t1.shape
    assert M % ppb == 0
    assert ppb * 8 * float(t2.abs().max().clamp_min(1)) < 2 ** 24 and ppb * float(t1.abs().max().clamp_min(1)) < 2 ** 24
    assert torch.equal(t2 * 8, (t2 * 8).round())
    return torch.stack([t1.reshape(M // ppb, ppb, C).sum(1), t2.reshape(M // ppb, ppb, C).sum(1)], 1)


def dyadic_sums(g, G, C, count):
    """S1, S2 [G][2][C] float64: integers in [-2 count, 2 count], so that S / count is a multiple of 1 / count in [-2, 2]"""
    assert count >= 64 and count & (count - 1) == 0
    return ints(g, (G, 2, C), -2 * count, 2 * count).double()


def bwd_ref(gy, x, mask, bnp, sums, count, mpg):
    """dx = scale (g mask - S1 / count - xhat S2 / count) and g mask, float64 [M][C], from vfs_bn_bwd_apply's definition; asserts
    that the coefficients the kernels form (m1, m2, B, D, B x + D) and dx are fp32-representable"""
    assert count & (count - 1) == 0
    A, mean, inv = (bnp[:, i].double() for i in (0, 2, 3))
    S1, S2 = sums[:, 0], sums[:, 1]
    m1, m2 = S1 / count, S2 / count
    B = -A * inv * m2
    D = A * (mean * inv * m2 - m1)
    gm = gy.double() * mask
    xd = x.double()
    e = lambda p: rows_of(p, mpg)
    bxd = e(B) * xd + e(D)
    dx = e(A) * (gm - e(m1) - (xd - e(mean)) * e(inv) * e(m2))
    fp32_exact(S1=S1, S2=S2, m1=m1, m2=m2, A_inv=A * inv, mean_inv=mean * inv, mean_inv_m2=mean * inv * m2, B=B, D=D, Bx_plus_D=bxd, dx=dx)
    assert torch.equal(dx, e(A) * gm + bxd), 'test bug: the float64 reference itself is not exact'
    return dx, gm


def rows_with_sum(g, S, bpg):
    """integer fp32 rows [G * bpg][2][C] whose sum over the bpg rows of group gi is S[gi] (S integer-valued)"""
    G, _, C = S.shape
    assert torch.equal(S, S.round())
    r = ints(g, (G, bpg, 2, C), -50, 50).double()
    r[:, -1] = S - r[:, :-1].sum(1)
    fp32_exact(rows=r)
    return r.reshape(G * bpg, 2, C).float().contiguous()


def seed(*k):
    s = 0
    for v in k:
        s = s * 1009 + int(v)
    return torch.Generator().manual_seed(s)


# ---------------------------------------------------------------------------------------------- 1. bn_act / bn_act_mask
def act_operands(g, G, mpg, C):
    M = G * mpg
    x, res, rres = (ints(g, (M, C), -255, 255) for _ in range(3))
    mk = lambda: torch.stack([pm(g, (G, C)) * pow2(g, (G, C), -1, 1), ints(g, (G, C), -64, 64) / 8,
                              ints(g, (G, C), -8, 8) / 2, pow2(g, (G, C), -2, 1)], 1).contiguous()
    return x, res, rres, mk(), mk()


def act_ref(x, bnp, res, rres, rbnp, mpg, relu):
    e = lambda p: rows_of(p, mpg).double()
    v = x.double() * e(bnp[:, 0]) + e(bnp[:, 1])
    fp32_exact(x_scale_shift=v)
    if res is not None:
        v = v + res.double()
    if rres is not None:
        fp32_exact(shift_plus_rshift=bnp[:, 1].double() + rbnp[:, 1].double(), rres_rscale=rres.double() * e(rbnp[:, 0]))
        v = v + rres.double() * e(rbnp[:, 0]) + e(rbnp[:, 1])
    fp32_exact(sum=v)
    assert float(v.abs().max()) * 8 < 2 ** 24 and torch.equal(v * 8, (v * 8).round())      # any association of the adds is exact
    return torch.relu(v) if relu else v


@pytest.mark.parametrize('geom,wide', SLABS, ids=SLAB_IDS)
def test_bn_act_and_mask(backend, geom, wide):
    """y and the bit-packed mask of vfs_bn_act_mask for the three operand combinations (res; rres with its own BatchNorm;
    neither), each with and without ReLU, and vfs_bn_act (no mask output)"""
    lib = backend.hostlib
    G, mpg, C = geom
    M = G * mpg
    g = seed(1, G, mpg, C)
    x, res, rres, bnp, rbnp = act_operands(g, G, mpg, C)
    B = lambda t: None if t is None else t.to(BF16)
    with wide_slabs(backend.lib, wide, C):
        for r, rr in ((res, None), (None, rres), (None, None)):
            for relu in (1, 0):
                ref = act_ref(x, bnp, r, rr, rbnp, mpg, relu)
                if M * C >= 4096:
                    assert rounded_share(ref) > 0.1, 'test bug: the rounding is hardly exercised'
                what = f'bn_act_mask, res={r is not None}, rres={rr is not None}, relu={relu}'
                y, mb = nan_like((M, C), CPU), bytes_like(M * C // 8)
                lib.bn_act_mask(B(x), bnp, B(r), B(rr), rbnp if rr is not None else None, y, mb, M, C, mpg, relu, None)
                assert_bits(y, expect_bf16(ref), what + ': y')
                assert_bits(mb, pack_relu_mask(expect_bf16(ref)), what + ': mask bytes')
        ref = act_ref(x, bnp, res, None, None, mpg, 1)
        y = nan_like((M, C), CPU)
        lib.bn_act(B(x), bnp, B(res), None, None, y, M, C, mpg, 1, None)
        assert_bits(y, expect_bf16(ref), 'bn_act, res, relu')


@pytest.mark.parametrize('via', ['res', 'rres', 'scale'])
@pytest.mark.parametrize('C,wide', [(64, False), (256, True)])
def test_bn_act_tie_block(backend, via, C, wide):
    """every fp32 value is sigma (257 + 2 j), j < 128: an exact tie between two bf16 values (spacing 2) - RNE alone passes.
    The odd part arrives through the residual, through the raw residual with scale 1/2 and an odd shift sum, or the block is
    formed by the scale alone (x = sigma (257 + 2 j) / 2 is not representable, so there x = sigma 128, scale 2, shift +-(1 + 2 j))"""
    lib = backend.hostlib
    mpg, G = 96, 2
    M = G * mpg
    p, c = torch.arange(M)[:, None], torch.arange(C)[None, :]
    j = ((p * 7 + c) % 128).double()
    sigma = (1.0 - 2.0 * ((p // 3 + c // 5) % 2)).double().expand(M, C)
    ref = sigma * (257 + 2 * j)
    assert bool(is_tie(ref).all())
    up = expect_bf16(ref).double().abs() > ref.abs()
    assert 0.4 < float(up.double().mean()) < 0.6, 'test bug: RNE must round about half of the ties up'
    zeros = torch.zeros(G, C)
    res = rres = rbnp = None
    if via == 'res':
        x, res = sigma * 256, sigma * (1 + 2 * j)
        bnp = torch.stack([zeros + 1, zeros, zeros, zeros + 1], 1).contiguous()
    elif via == 'rres':
        x, rres = sigma * 128, sigma * (2 + 4 * j) - 2 * 3
        bnp = torch.stack([zeros + 2, zeros - 5, zeros, zeros + 1], 1).contiguous()
        rbnp = torch.stack([zeros + 0.5, zeros + 8, zeros, zeros + 1], 1).contiguous()       # 2 x - 5 + rres / 2 + 8 = 2 x + sigma (1 + 2 j)
        bf16_exact(rres=rres)
    else:
        # scale alone: per-channel sign and j (sigma and j must not depend on the pixel then)
        jc = (c % 128).double().expand(M, C)
        sc = (1.0 - 2.0 * ((c // 5) % 2)).double().expand(M, C)
        ref = sc * (257 + 2 * jc)
        assert bool(is_tie(ref).all())
        x = torch.full((M, C), 128.0, dtype=F64)
        bnp = torch.stack([(2 * sc[0]).float().expand(G, C), (sc[0] * (1 + 2 * jc[0])).float().expand(G, C), zeros, zeros + 1], 1).contiguous()
    bf16_exact(x=x)
    got_ref = act_ref(x, bnp, res, rres, rbnp, mpg, 0)
    assert torch.equal(got_ref, ref)
    B = lambda t: None if t is None else t.to(BF16)
    y, mb = nan_like((M, C), CPU), bytes_like(M * C // 8)
    with wide_slabs(backend.lib, wide, C):
        lib.bn_act_mask(B(x), bnp, B(res), B(rres), rbnp, y, mb, M, C, mpg, 0, None)
    assert_bits(y, expect_bf16(ref), f'bn_act tie block through {via}')
    assert_bits(mb, pack_relu_mask(expect_bf16(ref)), f'bn_act tie block through {via}: mask bytes')


# ---------------------------------------------------------------------------------------------- 2. bn_bwd_reduce
def small_ppb(mpg):
    """a caller ppb that divides mpg (the largest proper divisor, at most mpg / 2)"""
    for d in range(2, mpg + 1):
        if mpg % d == 0:
            return mpg // d
    return mpg


@pytest.mark.parametrize('G,mpg,C', GEOMS + WIDE[:2])
def test_bn_bwd_reduce_rows(backend, G, mpg, C):
    """every partial row [nblk][2][C] against the float64 sums over its own pixel range: ppb = mpg and a proper divisor"""
    lib = backend.hostlib
    M = G * mpg
    g = seed(2, G, mpg, C)
    gy, x, bnp = bwd_operands(g, G, mpg, C)
    for name, ym, relu, mask in mask_modes(g, x, bnp, mpg):
        t1, t2 = row_terms(gy, x, mask, bnp, mpg)
        for ppb in sorted({mpg, small_ppb(mpg)}):
            want = block_sums(t1, t2, ppb)
            part = nan_like((M // ppb, 2, C), CPU, torch.float32)
            lib.bn_bwd_reduce(gy.to(BF16), ym, x.to(BF16), bnp, part, M, C, mpg, ppb, relu, None)
            assert_bits(part, want.float(), f'bn_bwd_reduce, {name}, ppb={ppb}: partial rows [block][S1 S2][channel]')


# ---------------------------------------------------------------------------------------------- 3. bn_bwd_apply
@pytest.mark.parametrize('geom,wide', SLABS, ids=SLAB_IDS)
def test_bn_bwd_apply(backend, geom, wide):
    """dx and gm with the sums supplied: narrow and wide slabs, every mask mode; count is a power of two of its own"""
    lib = backend.hostlib
    G, mpg, C = geom
    M = G * mpg
    g = seed(3, G, mpg, C)
    gy, x, bnp = bwd_operands(g, G, mpg, C)
    count = 64
    sums = dyadic_sums(g, G, C, count)
    with wide_slabs(backend.lib, wide, C):
        for name, ym, relu, mask in mask_modes(g, x, bnp, mpg):
            dxr, gmr = bwd_ref(gy, x, mask, bnp, sums, count, mpg)
            if M * C >= 4096:
                assert rounded_share(dxr) > 0.1, 'test bug: the rounding is hardly exercised'
            dx, gm = nan_like((M, C), CPU), nan_like((M, C), CPU)
            lib.bn_bwd_apply(gy.to(BF16), ym, x.to(BF16), bnp, sums.clone(), dx, gm, M, C, mpg, float(count), relu, None)
            assert_bits(dx, expect_bf16(dxr), f'bn_bwd_apply, {name}: dx')
            assert_bits(gm, expect_bf16(gmr), f'bn_bwd_apply, {name}: gm')
        dx = nan_like((M, C), CPU)
        name, ym, relu, mask = mask_modes(g, x, bnp, mpg)[1]
        lib.bn_bwd_apply(gy.to(BF16), ym, x.to(BF16), bnp, sums.clone(), dx, None, M, C, mpg, float(count), relu, None)
        assert_bits(dx, expect_bf16(bwd_ref(gy, x, mask, bnp, sums, count, mpg)[0]), 'bn_bwd_apply without gm: dx')


# ---------------------------------------------------------------------------------------------- 4. bn_bwd_apply_fin
@pytest.mark.parametrize('bpg', [1, 5, 21])      # the 4-row tail alone, one 16-row trip short, one trip and a tail
@pytest.mark.parametrize('G,mpg,C', GEOMS + WIDE[:1])
def test_bn_bwd_apply_fin(backend, G, mpg, C, bpg):
    """integer partial rows that add up to integer sums in [-2 count, 2 count]: sums, dx, gm and the `+=` onto integer dgamma / dbeta"""
    lib = backend.hostlib
    M = G * mpg
    g = seed(4, G, mpg, C, bpg)
    gy, x, bnp = bwd_operands(g, G, mpg, C)
    count = 128
    sums = dyadic_sums(g, G, C, count)
    part = rows_with_sum(g, sums, bpg)
    dg0, db0 = ints(g, (C,), -9, 9), ints(g, (C,), -9, 9)
    wantg, wantb = dg0.double() + sums[:, 1].sum(0), db0.double() + sums[:, 0].sum(0)
    fp32_exact(dgamma=wantg, dbeta=wantb, S2_total=sums[:, 1].sum(0), S1_total=sums[:, 0].sum(0))
    for name, ym, relu, mask in mask_modes(g, x, bnp, mpg)[:3 if bpg > 1 else 4]:
        dxr, gmr = bwd_ref(gy, x, mask, bnp, sums, count, mpg)
        if M * C >= 4096:
            assert rounded_share(dxr) > 0.1, 'test bug: the rounding is hardly exercised'
        dx, gm = nan_like((M, C), CPU), nan_like((M, C), CPU)
        bs = nan_like((G, 2, C), CPU, F64)
        dg, db = dg0.clone(), db0.clone()
        lib.bn_bwd_apply_fin(gy.to(BF16), ym, x.to(BF16), bnp, part, bpg, bs, dg, db, dx, gm, M, C, mpg, float(count), relu, None)
        what = f'bn_bwd_apply_fin, {name}'
        assert_bits(bs, sums, what + ': sums')
        assert_bits(dx, expect_bf16(dxr), what + ': dx')
        assert_bits(gm, expect_bf16(gmr), what + ': gm')
        assert_bits(dg, wantg.float(), what + ': dgamma')
        assert_bits(db, wantb.float(), what + ': dbeta')


# ---------------------------------------------------------------------------------------------- 5. bn_bwd_apply_raw
@pytest.mark.parametrize('C', [32, 64, 128])
@pytest.mark.parametrize('mpg,count', [(9, 16), (32, 32), (100, 128), (512, 512)])
def test_bn_bwd_apply_raw(backend, mpg, count, C):
    """one statistics row per group, formed by the launch itself from (g, x, mask): sums, dx, gm, dgamma, dbeta"""
    lib = backend.hostlib
    G = 2
    M = G * mpg
    g = seed(5, mpg, C)
    gy, x, bnp = bwd_operands(g, G, mpg, C)
    dg0, db0 = ints(g, (C,), -9, 9), ints(g, (C,), -9, 9)
    for name, ym, relu, mask in mask_modes(g, x, bnp, mpg)[:3]:
        t1, t2 = row_terms(gy, x, mask, bnp, mpg)
        sums = block_sums(t1, t2, mpg)                           # [G][2][C]
        dxr, gmr = bwd_ref(gy, x, mask, bnp, sums, count, mpg)
        wantg, wantb = dg0.double() + sums[:, 1].sum(0), db0.double() + sums[:, 0].sum(0)
        fp32_exact(dgamma=wantg, dbeta=wantb, S2_total=sums[:, 1].sum(0), S1_total=sums[:, 0].sum(0))
        if mpg >= 32:
            assert rounded_share(dxr) > 0.1, 'test bug: the rounding is hardly exercised'
        dx, gm = nan_like((M, C), CPU), nan_like((M, C), CPU)
        bs = nan_like((G, 2, C), CPU, F64)
        dg, db = dg0.clone(), db0.clone()
        lib.bn_bwd_apply_raw(gy.to(BF16), ym, x.to(BF16), bnp, bs, dg, db, dx, gm, M, C, mpg, float(count), relu, None)
        what = f'bn_bwd_apply_raw, {name}'
        assert_bits(bs, sums, what + ': sums')
        assert_bits(dx, expect_bf16(dxr), what + ': dx')
        assert_bits(gm, expect_bf16(gmr), what + ': gm')
        assert_bits(dg, wantg.float(), what + ': dgamma')
        assert_bits(db, wantb.float(), what + ': dbeta')


# ---------------------------------------------------------------------------------------------- 6. forward statistics
MOM = 0.25


def stats_data(g, G, mpg, C):
    """x [G * mpg][C] with per (group, channel) half the rows m + s, half m - s; m, s [G][C]"""
    assert mpg % 2 == 0
    m, s = ints(g, (G, C), -8, 8).double(), pow2(g, (G, C), -1, 2).double()
    half = torch.cat([torch.ones(mpg // 2), -torch.ones(mpg // 2)]).double()
    perm = torch.rand(G, mpg, C, generator=g).argsort(1)
    x = m[:, None, :] + half[perm] * s[:, None, :]
    bf16_exact(x=x)
    return x.reshape(G * mpg, C), m, s


def one_ulp(want):
    """one fp32 ulp of `want` (float64 tensor of fp32 values)"""
    return torch.ldexp(torch.ones_like(want), torch.frexp(want).exponent - 24)


def stats_expected(m, s, gamma, beta, rm0, rv0, count):
    """sums [G][2][C], bnp [G][4][C] (all exact) and the running statistics after the G group-by-group updates"""
    G, C = m.shape
    sums = torch.stack([count * m, count * (m * m + s * s)], 1)
    scale = gamma.double() / s
    bnp = torch.stack([scale, beta.double() - m * scale, m, 1 / s], 1)
    fp32_exact(bnp=bnp, sums=sums)
    rm, rv = rm0.double(), rv0.double()
    for gi in range(G):
        rm = MOM * m[gi] + (1 - MOM) * rm
        fp32_exact(running_mean=rm, keep_rm=(1 - MOM) * rm)
        var = s[gi] * s[gi]
        unbiased = var * (count / (count - 1.0)) if count > 1 else var             # the kernel's float64 expression
        rv = (MOM * unbiased.float().double() + ((1 - MOM) * rv).float().double()).float().double()
    return sums, bnp, rm, rv


def check_stats(what, got, want):
    sums, bnp, rm, rv = got
    wsums, wbnp, wrm, wrv = want
    assert_bits(sums, wsums, what + ': sums')
    for i, row in enumerate(('scale', 'shift', 'mean', 'invstd')):
        assert_bits(bnp[:, i], wbnp[:, i].float(), what + f': bnp row {row}')
    assert_bits(rm, wrm.float(), what + ': running_mean')
    err = (rv.double() - wrv).abs()
    assert bool((err <= one_ulp(wrv)).all()), f'{what}: running_var is off by up to {float((err / one_ulp(wrv)).max())} ulp'


@pytest.mark.parametrize('G,mpg,C,ppr', [(2, 64, 64, 16), (3, 16, 192, 8), (1, 128, 32, 32), (2, 8, 8, 8), (2, 32, 2048, 32),
                                         (2, 256, 128, 16), (2, 512, 40, 4)])
def test_forward_statistics(backend, G, mpg, C, ppr):
    """vfs_bn_stats_raw_finalize, vfs_bn_stats_finalize, vfs_bn_reduce_partials + vfs_bn_finalize, vfs_bn_act_fin and
    vfs_bn_act_fin_mask on statistics that are exact: sums, bnp, running_mean, y and the mask bit for bit; running_var to
    one fp32 ulp.  (2, 512, 40, 4): 128 rows per group (the ticket path of the reductions), a partial 32-channel block -
    C = 40 is no slab width, so the apply launches are left out there."""
    lib = backend.hostlib
    M, bpg = G * mpg, mpg // ppr
    g = seed(6, G, mpg, C)
    x, m, s = stats_data(g, G, mpg, C)
    gamma = (pm(g, (C,)) * pow2(g, (C,), -1, 1)).float()
    beta = (ints(g, (C,), -16, 16) / 4).float()
    rm0, rv0 = ints(g, (C,), -8, 8) / 4, ints(g, (C,), 1, 8) / 4
    count = mpg
    want = stats_expected(m, s, gamma, beta, rm0, rv0, count)
    part64 = torch.stack([x.reshape(G * bpg, ppr, C).sum(1), (x * x).reshape(G * bpg, ppr, C).sum(1)], 1)
    fp32_exact(partial_rows=part64)
    part = part64.float().contiguous()
    scratch = torch.zeros(32 + G * 128 * 2 * C, dtype=F64)
    fresh = lambda: (nan_like((G, 2, C), CPU, F64), nan_like((G, 4, C), CPU, torch.float32), rm0.clone(), rv0.clone())

    sums, bnp, rm, rv = fresh()
    lib.bn_stats_raw_finalize(x.to(BF16), sums, gamma, beta, bnp, rm, rv, G, mpg, C, float(count), 0.0, MOM, None)
    check_stats('bn_stats_raw_finalize', (sums, bnp, rm, rv), want)

    sums, bnp, rm, rv = fresh()
    lib.bn_stats_finalize(part, sums, scratch, gamma, beta, bnp, rm, rv, G, bpg, C, float(count), 0.0, MOM, None)
    check_stats('bn_stats_finalize', (sums, bnp, rm, rv), want)
    assert int(scratch[:32].view(torch.int32).abs().sum()) == 0

    sums, bnp, rm, rv = fresh()
    lib.bn_reduce_partials(part, sums, scratch, G, bpg, C, None)
    lib.bn_finalize(sums, gamma, beta, bnp, rm, rv, G, C, float(count), 0.0, MOM, None)
    check_stats('bn_reduce_partials + bn_finalize', (sums, bnp, rm, rv), want)
    assert int(scratch[:32].view(torch.int32).abs().sum()) == 0
    if C == 40:
        return

    res = ints(g, (M, C), -255, 255)
    for relu in (0, 1):
        e = lambda p: rows_of(p, mpg)
        v = x * e(want[1][:, 0]) + e(want[1][:, 1])
        fp32_exact(x_scale_shift=v, y=v + res.double())
        ref = v + res.double()
        ref = torch.relu(ref) if relu else ref
        if relu == 0 and M * C >= 4096:
            assert rounded_share(ref) > 0.1, 'test bug: the rounding is hardly exercised'
        sums, bnp, rm, rv = fresh()
        y = nan_like((M, C), CPU)
        lib.bn_act_fin(x.to(BF16), part, bpg, gamma, beta, bnp, sums, rm, rv, res.to(BF16), None, None, y, M, C, mpg, relu, float(count),
                       0.0, MOM, None)
        check_stats(f'bn_act_fin, relu={relu}', (sums, bnp, rm, rv), want)
        assert_bits(y, expect_bf16(ref), f'bn_act_fin, relu={relu}: y')
        sums, bnp, rm, rv = fresh()
        y, mb = nan_like((M, C), CPU), bytes_like(M * C // 8)
        lib.bn_act_fin_mask(x.to(BF16), part, bpg, gamma, beta, bnp, sums, rm, rv, res.to(BF16), None, None, y, mb, M, C, mpg, relu,
                            float(count), 0.0, MOM, None)
        check_stats(f'bn_act_fin_mask, relu={relu}', (sums, bnp, rm, rv), want)
        assert_bits(y, expect_bf16(ref), f'bn_act_fin_mask, relu={relu}: y')
        assert_bits(mb, pack_relu_mask(expect_bf16(ref)), f'bn_act_fin_mask, relu={relu}: mask bytes')


# ---------------------------------------------------------------------------------------------- 7. reduction tails
@pytest.mark.parametrize('C', [40, 72])
@pytest.mark.parametrize('bpg', [1, 8, 9, 33, 64, 65, 300])
def test_reduction_tails(backend, bpg, C):
    """integer rows through vfs_bn_reduce_partials, vfs_bn_stats_finalize and vfs_bn_bwd_sums_paramgrad: the 8-row and 32-row
    loops, the ticket path above 64 rows, a partial 32-channel block; twice on the same scratch"""
    lib = backend.hostlib
    G = 2
    g = seed(7, bpg, C)
    part = ints(g, (G * bpg, 2, C), -1000, 1000)
    part[:, 1] = part[:, 1].abs()                             # (a sum of squares is not negative)
    want = part.double().reshape(G, bpg, 2, C).sum(1)
    dg0, db0 = ints(g, (C,), -9, 9), ints(g, (C,), -9, 9)
    wantg, wantb = dg0.double() + want[:, 1].sum(0), db0.double() + want[:, 0].sum(0)
    fp32_exact(dgamma=wantg, dbeta=wantb, column_sums=want, totals=want.sum(0))
    scratch = torch.zeros(32 + G * 128 * 2 * C, dtype=F64)
    tickets_zero = lambda: int(scratch[:32].view(torch.int32).abs().sum()) == 0
    gamma, beta = torch.ones(C), torch.zeros(C)
    for rep in range(2):
        sums = nan_like((G, 2, C), CPU, F64)
        lib.bn_reduce_partials(part, sums, scratch, G, bpg, C, None)
        assert torch.equal(sums, want), f'bn_reduce_partials, launch {rep}'
        assert tickets_zero()
        sums = nan_like((G, 2, C), CPU, F64)
        lib.bn_stats_finalize(part, sums, scratch, gamma, beta, torch.zeros(G, 4, C), torch.zeros(C), torch.ones(C), G, bpg, C,
                              float(bpg * 128), 1e-5, 0.1, None)
        assert torch.equal(sums, want), f'bn_stats_finalize, launch {rep}'
        assert tickets_zero()
        sums = nan_like((G, 2, C), CPU, F64)
        dg, db = dg0.clone(), db0.clone()
        lib.bn_bwd_sums_paramgrad(part, sums, scratch, dg, db, G, bpg, C, None)
        assert torch.equal(sums, want), f'bn_bwd_sums_paramgrad, launch {rep}'
        assert tickets_zero()
        assert_bits(dg, wantg.float(), f'bn_bwd_sums_paramgrad, launch {rep}: dgamma')
        assert_bits(db, wantb.float(), f'bn_bwd_sums_paramgrad, launch {rep}: dbeta')
    sums = nan_like((G, 2, C), CPU, F64)
    lib.bn_reduce_partials(part, sums, None, G, bpg, C, None)          # without scratch: the plain row kernel
    assert torch.equal(sums, want), 'bn_reduce_partials without scratch'


# ---------------------------------------------------------------------------------------------- 8. stem pooling
def pooled_size(H, W):
    return (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1


def stem_lin(x, bnp, npg):
    """x scale + shift, float64 [N][H][W][C], image n with the parameters of group n // npg"""
    gi = torch.arange(x.shape[0]) // npg
    lin = x.double() * bnp[gi, 0].double()[:, None, None, :] + bnp[gi, 1].double()[:, None, None, :]
    fp32_exact(x_scale_shift=lin)
    return lin


def pool_ref(x, bnp, npg, stored=True):
    """float64 reference of vfs_bn_relu_maxpool on x [N][H][W][C]: activation = bf16(relu(x scale + shift)), pooled maximum over
    the valid taps of the 3x3 / stride 2 / pad 1 window, code = FIRST tap in ascending k = 3 dy + dx that holds it (0xFF where
    the pooled value is not positive), xpool = raw x at that tap.  stored=False is NOT the operation: it pools the fp32
    activation (a case uses it to show that its data tell the two apart)"""
    N, H, W, C = x.shape
    Hp, Wp = pooled_size(H, W)
    xd = x.double()
    act = torch.relu(stem_lin(x, bnp, npg))
    if stored:
        act = expect_bf16(act).double()
    ninf = float('-inf')
    apad = torch.full((N, 2 * Hp + 1, 2 * Wp + 1, C), ninf, dtype=F64)
    xpad = torch.zeros(N, 2 * Hp + 1, 2 * Wp + 1, C, dtype=F64)
    apad[:, 1:H + 1, 1:W + 1] = act
    xpad[:, 1:H + 1, 1:W + 1] = xd
    best = torch.full((N, Hp, Wp, C), ninf, dtype=F64)
    code = torch.full((N, Hp, Wp, C), 255, dtype=torch.int64)
    xat = torch.zeros(N, Hp, Wp, C, dtype=F64)
    ties = 0
    for k in range(9):
        dy, dx = k // 3, k % 3
        tap = apad[:, dy:dy + 2 * Hp:2, dx:dx + 2 * Wp:2]
        ties += int(((tap == best) & (tap > 0)).sum())
        better = tap > best                        # strictly: among equal activations the earlier tap stays
        best = torch.where(better, tap, best)
        code = torch.where(better, torch.full_like(code, k), code)
        xat = torch.where(better, xpad[:, dy:dy + 2 * Hp:2, dx:dx + 2 * Wp:2], xat)
    assert bool((best >= 0).all())
    code = torch.where(best > 0, code, torch.full_like(code, 255))
    return best, code.to(torch.uint8), xat, ties


def unpool_ref(gp, code, H, W):
    """ga [N][H][W][C] float64: every pooled gradient added at the position its code names"""
    N, Hp, Wp, C = gp.shape
    gpad = torch.zeros(N, 2 * Hp + 1, 2 * Wp + 1, C, dtype=F64)
    for k in range(9):
        dy, dx = k // 3, k % 3
        gpad[:, dy:dy + 2 * Hp:2, dx:dx + 2 * Wp:2] += gp.double() * (code == k)
    ga = gpad[:, 1:H + 1, 1:W + 1]
    assert float(gpad.abs().sum()) == float(ga.abs().sum()), 'test bug: a code names a tap outside the map'
    return ga.contiguous()


def stem_params(g, G, C):
    scale = pm(g, (G, C)) * pow2(g, (G, C), -1, 1)
    return torch.stack([scale, ints(g, (G, C), -14, 2) / 2, ints(g, (G, C), -8, 8) / 2, pow2(g, (G, C), -2, 1)], 1).contiguous()


STEM_SHAPES = [(3, 2, 9, 11), (2, 1, 10, 12), (1, 1, 2, 3)]      # (N, npg, H, W); the last group of the first is ragged


@pytest.mark.parametrize('C', [64, 8, 24])
@pytest.mark.parametrize('N,npg,H,W', STEM_SHAPES)
def test_stem_maxpool_forward_and_unpool(backend, N, npg, H, W, C):
    """vfs_bn_relu_maxpool: y, idx, xpool (where the code is a tap); vfs_maxpool_relu_bwd on the REFERENCE codes: ga"""
    lib = backend.hostlib
    g = seed(8, N, H, C)
    G = (N + npg - 1) // npg
    x = ints(g, (N, H, W, C), -6, 6)
    bnp = stem_params(g, G, C)
    Hp, Wp = pooled_size(H, W)
    yr, coder, xatr, ties = pool_ref(x, bnp, npg)
    if H > 2:
        assert ties > 0.1 * yr.numel(), 'test bug: equal activations inside a window are rare'
        assert 0.05 < float((coder == 255).double().mean()) < 0.9
    for with_xpool in (True, False):
        y, idx = nan_like((N, Hp, Wp, C), CPU), bytes_like(N * Hp * Wp * C).reshape(N, Hp, Wp, C)
        xp = nan_like((N, Hp, Wp, C), CPU) if with_xpool else None
        lib.bn_relu_maxpool(x.to(BF16), bnp, y, idx, xp, N, H, W, C, Hp, Wp, npg, None)
        what = f'bn_relu_maxpool{" with xpool" if with_xpool else ""}'
        assert_bits(y, expect_bf16(yr), what + ': y', pixels=False)
        assert_bits(idx, coder, what + ': argmax code', pixels=False)
        if with_xpool:
            tap = coder != 255
            assert_bits(torch.where(tap, xp.double(), torch.zeros((), dtype=F64)), torch.where(tap, xatr, torch.zeros((), dtype=F64)),
                        what + ': xpool where the code is a tap', pixels=False)
            assert bool(torch.isfinite(xp.float()).all())
    gp = ints(g, (N, Hp, Wp, C), -4, 4)
    gar = unpool_ref(gp, coder, H, W)
    ga = nan_like((N, H, W, C), CPU)
    lib.maxpool_relu_bwd(gp.to(BF16), expect_bf16(yr), coder, ga, N, H, W, C, Hp, Wp, None)
    assert_bits(ga, expect_bf16(gar), 'maxpool_relu_bwd: ga', pixels=False)


@pytest.mark.parametrize('C', [64, 8])
def test_stem_maxpool_pools_the_stored_bf16_activation(backend, C):
    """the rounding regime of the pooling kernel: |x| in [192, 255], scale in +-{1/2, 1, 2}, shift = |scale| [300, 420] plus
    eighths - x scale + shift is exact in fp32 (a multiple of 1/8 below 2^11) and needs more than eight bits; the taps on the
    positive side land in [512 |scale|, 1024 |scale|), where bf16 is spaced 4 |scale| and x scale moves in steps of |scale|.
    Taps then often differ in fp32 but round to the same bf16 value, and the code must name the FIRST tap that holds the rounded
    maximum: a kernel that pooled the fp32 activation and rounded afterwards would store the same y and other codes / xpool"""
    lib = backend.hostlib
    N, npg, H, W = 3, 2, 9, 11
    g = seed(13, C)
    G = 2
    x = pm(g, (N, H, W, C)) * ints(g, (N, H, W, C), 192, 255)
    scale = pm(g, (G, C)) * pow2(g, (G, C), -1, 1)
    shift = scale.abs() * ints(g, (G, C), 300, 420) + ints(g, (G, C), -4, 4) / 8
    bnp = torch.stack([scale, shift, torch.zeros(G, C), torch.ones(G, C)], 1).contiguous()
    bf16_exact(x=x)
    Hp, Wp = pooled_size(H, W)
    pre = torch.relu(stem_lin(x, bnp, npg))
    assert rounded_share(pre) > 0.1, 'test bug: the rounding of the activation is hardly exercised'
    yr, coder, xatr, _ = pool_ref(x, bnp, npg)
    y32, code32, xat32, _ = pool_ref(x, bnp, npg, stored=False)
    assert torch.equal(expect_bf16(y32), expect_bf16(yr))            # rounding is monotone: y cannot tell the two apart
    apart = (code32 != coder) & (coder != 255)                        # windows whose fp32 maximum is a LATER tap than the first rounded one
    assert float(apart.double().mean()) > 0.02 and bool((xat32 != xatr)[apart].all()), 'test bug: pooling before the rounding would pass'
    y, idx = nan_like((N, Hp, Wp, C), CPU), bytes_like(N * Hp * Wp * C).reshape(N, Hp, Wp, C)
    xp = nan_like((N, Hp, Wp, C), CPU)
    lib.bn_relu_maxpool(x.to(BF16), bnp, y, idx, xp, N, H, W, C, Hp, Wp, npg, None)
    assert_bits(y, expect_bf16(yr), 'bn_relu_maxpool, rounding regime: y', pixels=False)
    assert_bits(idx, coder, 'bn_relu_maxpool, rounding regime: argmax code', pixels=False)
    tap = coder != 255
    assert_bits(torch.where(tap, xp.double(), torch.zeros((), dtype=F64)), torch.where(tap, xatr, torch.zeros((), dtype=F64)),
                'bn_relu_maxpool, rounding regime: xpool where the code is a tap', pixels=False)


@pytest.mark.parametrize('C', [64, 8])
@pytest.mark.parametrize('N,npg,H,W,ppbs', [(3, 2, 9, 11, (20, 60)), (2, 1, 10, 12, (15, 30)), (1, 1, 2, 3, (1, 2))])
def test_stem_pool_bn_bwd_reduce(backend, N, npg, H, W, ppbs, C):
    """both `xpool` modes: every partial row [block][2][C] against the float64 sums over its own pooled-pixel range"""
    lib = backend.hostlib
    g = seed(9, N, H, C)
    G = (N + npg - 1) // npg
    x = ints(g, (N, H, W, C), -6, 6)
    bnp = stem_params(g, G, C)
    Hp, Wp = pooled_size(H, W)
    P = N * Hp * Wp
    yr, coder, xatr, _ = pool_ref(x, bnp, npg)
    gp = ints(g, (N, Hp, Wp, C), -4, 4)
    gi = torch.arange(N) // npg
    t1 = gp.double() * (coder != 255)
    xhat = (xatr - bnp[gi, 2].double()[:, None, None, :]) * bnp[gi, 3].double()[:, None, None, :]
    t2 = t1 * xhat
    fp32_exact(xhat=xhat, g_xhat=t2)
    t1, t2 = t1.reshape(P, C), t2.reshape(P, C)
    for ppb in ppbs:
        assert (npg * Hp * Wp) % ppb == 0
        nblk = (P + ppb - 1) // ppb
        assert ppb * 8 * float(t2.abs().max().clamp_min(1)) < 2 ** 24
        want = torch.stack([torch.stack([t[b * ppb:(b + 1) * ppb].sum(0) for t in (t1, t2)]) for b in range(nblk)])
        for mode, xp in (('gather from x', None), ('xpool stream', xatr.to(BF16))):
            part = nan_like((nblk, 2, C), CPU, torch.float32)
            lib.stem_pool_bn_bwd_reduce(gp.to(BF16), expect_bf16(yr), coder, x.to(BF16), xp, bnp, part, N, H, W, C, Hp, Wp, npg, ppb, None)
            assert_bits(part, want.float(), f'stem_pool_bn_bwd_reduce, {mode}, ppb={ppb}: partial rows')


@pytest.mark.parametrize('N,npg,H,W', STEM_SHAPES)
def test_stem_pool_bn_bwd_apply(backend, N, npg, H, W):
    """dx = scale (ga - S1 / count - xhat S2 / count) with ga rebuilt from the pooled tensors; sums supplied"""
    lib = backend.hostlib
    C = 64
    g = seed(10, N, H)
    G = (N + npg - 1) // npg
    x = ints(g, (N, H, W, C), -6, 6)
    bnp = stem_params(g, G, C)
    Hp, Wp = pooled_size(H, W)
    yr, coder, _, _ = pool_ref(x, bnp, npg)
    gp = ints(g, (N, Hp, Wp, C), -4, 4)
    gar = unpool_ref(gp, coder, H, W)
    bf16_exact(ga=gar)
    count = 64
    sums = dyadic_sums(g, G, C, count)
    # one "group" per image for the shared reference: image n takes the parameters and sums of group n // npg
    gi = torch.arange(N) // npg
    dxr, _ = bwd_ref(gar.reshape(N * H * W, C), x.reshape(N * H * W, C), torch.ones(N * H * W, C, dtype=F64), bnp[gi], sums[gi], count, H * W)
    if H > 2:
        assert rounded_share(dxr) > 0.1, 'test bug: the rounding is hardly exercised'
    dx = nan_like((N, H, W, C), CPU)
    lib.stem_pool_bn_bwd_apply(gp.to(BF16), expect_bf16(yr), coder, x.to(BF16), bnp, sums.clone(), dx, N, H, W, C, Hp, Wp, npg, float(count), None)
    assert_bits(dx, expect_bf16(dxr.reshape(N, H, W, C)), 'stem_pool_bn_bwd_apply: dx')


# ---------------------------------------------------------------------------------------------- 9. small ops
@pytest.mark.parametrize('HW', [1, 4, 16])
@pytest.mark.parametrize('N,C', [(3, 72), (5, 2048)])
def test_avgpool(backend, N, C, HW):
    """HW a power of two: the mean is exact in fp32 (sum below 2^12, in sixteenths) and y its RNE rounding; the backward's
    g / HW is a bf16 value"""
    lib = backend.hostlib
    g = seed(11, N, C, HW)
    x = ints(g, (N, HW, C), -255, 255)
    mean = x.double().sum(1) / HW
    fp32_exact(mean=mean)
    if HW > 1:
        assert rounded_share(mean) > 0.1, 'test bug: the rounding is hardly exercised'
    y = nan_like((N, C), CPU)
    lib.avgpool_fwd(x.to(BF16), y, N, HW, C, None)
    assert_bits(y, expect_bf16(mean), 'avgpool_fwd')
    gy = ints(g, (N, C), -255, 255)
    gx = nan_like((N, HW, C), CPU)
    lib.avgpool_bwd(gy.to(BF16), gx, N, HW, C, None)
    assert_bits(gx, expect_bf16((gy.double() / HW)[:, None, :].expand(N, HW, C)), 'avgpool_bwd')


@pytest.mark.parametrize('M', [1, 7, 300])
@pytest.mark.parametrize('C', [72, 256])
def test_bias_grad(backend, M, C):
    lib = backend.hostlib
    g = seed(12, M, C)
    dy = ints(g, (M, C), -255, 255)
    db0 = ints(g, (C,), -9, 9)
    want = db0.double() + dy.double().sum(0)
    assert M * 255 + 9 < 2 ** 24
    db = db0.clone()
    lib.bias_grad(dy.to(BF16), db, M, C, None)
    assert_bits(db, want.float(), 'bias_grad onto a non-zero start')
