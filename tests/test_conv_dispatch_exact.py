"""Exact-operand parity of the convolution kernel instances that only LARGE problems select, reached on small shapes by setting
the dispatchers' options: the bodies of tests/test_conv_exact.py and tests/test_conv_dilated_bwd.py run again, unchanged, under
the settings that move a small shape to the instance a bench-size layer runs.  No tolerance anywhere: a bf16 output is the RNE
rounding of the float64 result, an fp32 output (weight-gradient slices, statistics rows) the float64 result itself
(assert_bits, under the exact_ok / small_ok preconditions the bodies assert on their own data).

The dispatchers choose by tile count (csrc/conv_igemm.hip vfs_conv_igemm_tiling, conv_halo.hip launch_halo, conv_wgrad.hip
launch_wgrad, conv_dilated.hip), so with default options every small shape lands in the small-problem instance:
  wide      128-channel implicit-GEMM tile: Cout % 128 == 0 and tiles128 >= igemm_narrow_below (default 513 tiles)
  non-deep  the two-stage 128-channel halo schedule: tiles * ncb > halo_deep_max (default 256)
  XCD order the tile remap is the identity below 9 workgroups (and off below 16 weight-gradient blocks); a grid of >= 9
            workgroups that is no multiple of 8 makes the eight ranges unequal - a remap that is no bijection drops or doubles
            a tile there.  Each such case runs with the remap on and off: both must be the float64 result
Every case evaluates the predicate of the instance it names on its own geometry and the options in force BEFORE it launches,
from the plan queries where the library answers (vfs_conv_plan, vfs_conv_wgrad_plan, vfs_conv_dgrad_ds_plan), else from the
documented rule; a failing predicate is a test bug.  An autouse fixture checks after every test that every option is back at
its default; test_every_option_is_swept_somewhere fails when an option exists that no kernel launch of the suite runs under.

backend=emu: host build through the fiber emulator; backend=gpu: libvfs_hip.so on the MI355X."""
import contextlib
import ctypes

import pytest
import torch

import tests.test_bn_exact as bn_exact
import tests.test_conv_exact as conv_exact
import tests.test_exact_f32 as exact_f32
import tests.test_labelprop2 as labelprop2
from tests.emu_util import nhwc
from tests.test_conv_dilated_bwd import CASES as DIL_CASES, run_dilated_backward_exact_operands
from tests.test_conv_exact import (REGIMES, assert_bits, exact_ok, expect_bf16, nan_like, nhwc64, operands, out_size, run_dgrad,
                                   run_dgrad_masked_add_and_fused_bn_rows, run_dilated_forward, run_folded_input_batchnorm, run_fwd,
                                   run_splitk, run_tie_block, run_wgrad, small_ok)
from tests.test_downsample_dgrad_compact import options, plan as ds_plan
from tests.test_emu_conv import pack
from tests.test_host_abi import OPTION_DEFAULTS
from vfs_amd.packing import conv_plan, wgrad_halo_tiles

BF16 = torch.bfloat16
FORCE = dict(OPTION_DEFAULTS)      # the options in force, as this file set them


@contextlib.contextmanager
def setting(be, **values):
    """options(...) of tests/test_downsample_dgrad_compact.py with the defaults of OPTION_DEFAULTS; FORCE follows, and on the
    emulator the library's own `vfs_option_<name>` must show the value"""
    assert all(FORCE[n] == OPTION_DEFAULTS[n] for n in values), 'test bug: an option is set twice'
    with options(be.lib, tuple((n.encode(), v, OPTION_DEFAULTS[n]) for n, v in values.items())):
        FORCE.update(values)
        try:
            if be.name == 'emu':
                for n, v in values.items():
                    assert ctypes.c_int.in_dll(be.lib.dll, 'vfs_option_' + n).value == v, n
            yield
        finally:
            FORCE.update({n: OPTION_DEFAULTS[n] for n in values})


@pytest.fixture(autouse=True)
def every_option_back_at_its_default(request):
    be = request.getfixturevalue('backend') if 'backend' in request.fixturenames else None      # (set up first: torn down last)
    yield
    assert FORCE == OPTION_DEFAULTS
    if be is None:
        return
    if be.name == 'emu':
        now = {n: ctypes.c_int.in_dll(be.lib.dll, 'vfs_option_' + n).value for n in OPTION_DEFAULTS}
        assert now == OPTION_DEFAULTS, {n: v for n, v in now.items() if v != OPTION_DEFAULTS[n]}
    else:
        for n, v in OPTION_DEFAULTS.items():
            be.lib.set_option(n.encode(), v)


# ---------------------------------------------------------------------------------------------- the dispatchers' predicates
def cdiv(a, b):
    return (a + b - 1) // b


def igemm_tile(M, C):
    """channel tile of an implicit-GEMM launch producing [M][C] (vfs_conv_igemm_tiling; conv_dilated.hip has the same rule)"""
    wide = C % 128 == 0 and FORCE['igemm_bc'] != 64 and cdiv(M, 128) * cdiv(C, 128) >= FORCE['igemm_narrow_below']
    return 128 if wide else 64


def reaches_wide(M, C):
    assert C % 128 == 0 and cdiv(M, 128) * cdiv(C, 128) >= FORCE['igemm_narrow_below'] and igemm_tile(M, C) == 128, \
        f'test bug: [{M}][{C}] does not reach the 128-channel tile under igemm_narrow_below={FORCE["igemm_narrow_below"]}'


def ring_launch(M, C, Ktot, fused_bn=False):
    """does a 1x1 / stride-1 launch producing [M][C] take the pure-GEMM DMA ring (vfs_conv_igemm_tiling)?  fused_bn: the launch
    emits BatchNorm-backward rows, which ride the ring only with igemm_ring_fbn"""
    tiles = cdiv(M, 128) * cdiv(C, igemm_tile(M, C))
    return 0 < FORCE['igemm_ring_tiles'] and tiles <= FORCE['igemm_ring_tiles'] and Ktot >= 256 and (not fused_bn or FORCE['igemm_ring_fbn'] != 0)


def reaches_ring(M, C, Ktot):
    assert ring_launch(M, C, Ktot), f'test bug: [{M}][{C}], K = {Ktot} is no ring launch'


def unequal_xcd_ranges(grid):
    assert grid >= 9 and grid % 8 != 0, f'test bug: a grid of {grid} workgroups does not make the XCD ranges unequal'


def halo_launch(be, N, H, W, Cin, Cout, dgrad):
    """(channel tile, workgroups) of the 3x3 halo launch, from vfs_conv_plan: its statistics rows are tiles x pairs of pixel
    waves - one pair per tile with the 128-channel tile, two with the 64-channel tile (conv_halo.hip vfs_conv_halo_stats_rows)"""
    p = conv_plan(N, 1, H, W, Cin, Cout, 3, 1, 1, H, W, dgrad=dgrad, lib=be.lib)
    assert p.halo and p.rows, 'test bug: the halo kernel does not take this shape'
    prod = Cin if dgrad else Cout
    bc = 128 if prod % 128 == 0 else 64
    return bc, p.rows // (1 if bc == 128 else 2) * (prod // bc)


def reaches_non_deep(be, N, H, W, Cin, Cout, dgrad):
    bc, grid = halo_launch(be, N, H, W, Cin, Cout, dgrad)
    assert bc == 128 and grid > FORCE['halo_deep_max'], f'test bug: {grid} workgroups of {bc} channels stay on the deep schedule'
    return grid


def wgrad_swizzled(tiles, nsplit):
    """the weight-gradient kernels' remap switches on with more than one tile per split and >= 16 blocks (launch_wgrad,
    vfs_wgrad_halo_dispatch, launch_wgrad_dil); the grid must make it matter whether wgrad_xcd is on or off: with the option
    off the same grid runs in plain order, the twin of the case with the remap on"""
    blocks = tiles * nsplit
    assert tiles > 1 and blocks >= 16 and blocks % 8 != 0, f'test bug: {tiles} tiles x {nsplit} splits: the remap is off or a bijection by construction'


def generic_wgrad_tiles(Cin, Cout, k):
    return cdiv(k * k * Cin, 128) * (Cout // (128 if Cout % 128 == 0 else 64))


# ---------------------------------------------------------------------------------------------- 1. the wide implicit-GEMM tile
#   N, H, W, Cin, Cout, k, stride, pad
WIDE_FWD = [(2, 9, 11, 64, 128, 3, 2, 1),       # 3x3 / stride 2
            (2, 8, 8, 64, 256, 1, 2, 0),        # 1x1 / stride 2, two channel tiles
            (3, 7, 7, 64, 128, 3, 1, 1),        # 3x3 / stride 1 gather (halo = 0), ragged M = 147
            (1, 12, 12, 64, 256, 1, 1, 0)]      # pure GEMM, two channel tiles, ragged last pixel tile (M = 144)
WIDE_DGRAD = [(3, 7, 7, 128, 64, 3, 1, 1),      # stride-1 3x3 (halo = 0), 128 produced channels
              (3, 7, 7, 128, 64, 1, 1, 0),      # stride-1 1x1
              (2, 9, 11, 128, 64, 3, 2, 1),     # stride 2 on an odd map: four unequal parity classes
              (1, 12, 12, 256, 64, 1, 1, 0)]    # two channel tiles, ragged M = 144


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout,k,stride,pad', WIDE_FWD)
def test_wide_forward(backend, regime, N, H, W, Cin, Cout, k, stride, pad):
    Ho, Wo = out_size(H, W, k, stride, pad)
    with setting(backend, igemm_narrow_below=0, halo=0):
        reaches_wide(N * Ho * Wo, Cout)
        run_fwd(backend, regime, N, H, W, Cin, Cout, k, stride, pad)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout,k,stride,pad', WIDE_DGRAD)
def test_wide_dgrad(backend, regime, N, H, W, Cin, Cout, k, stride, pad):
    if stride == 2:
        assert len({((H - ph + 1) // 2) * ((W - pw + 1) // 2) for ph in (0, 1) for pw in (0, 1)}) == 4, 'test bug: equal parity classes'
    with setting(backend, igemm_narrow_below=0, halo=0):
        reaches_wide(N * H * W, Cin)
        run_dgrad(backend, regime, N, H, W, Cin, Cout, k, stride, pad)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout,k,ring_fbn', [
    (2, 8, 16, 128, 64, 1, 1),       # one K-step: register pipeline
    (3, 7, 7, 128, 256, 1, 1),       # K = 256, ragged M: every launch on the DMA ring
    (3, 7, 7, 128, 256, 1, 0),       # the same with igemm_ring_fbn = 0: the masked add on the ring, the two launches with fused rows on the register pipeline
    (2, 8, 16, 128, 64, 3, 1)])      # 3x3 gather (halo = 0)
def test_wide_dgrad_masked_add_and_fused_bn_rows(backend, regime, N, H, W, Cin, Cout, k, ring_fbn):
    opts = dict(igemm_narrow_below=0, halo=0)
    if ring_fbn != OPTION_DEFAULTS['igemm_ring_fbn']:
        opts['igemm_ring_fbn'] = ring_fbn
    with setting(backend, **opts):
        M = N * H * W
        reaches_wide(M, Cin)
        pure = k == 1
        assert (pure and ring_launch(M, Cin, k * k * Cout)) == (Cout >= 256), 'test bug: conv_dgrad_maskadd is not on the instance the case names'
        assert (pure and ring_launch(M, Cin, k * k * Cout, fused_bn=True)) == (Cout >= 256 and ring_fbn == 1), \
            'test bug: conv_dgrad_bn / conv_dgrad_bn_maskadd are not on the instance the case names'
        run_dgrad_masked_add_and_fused_bn_rows(backend, regime, N, H, W, Cin, Cout, k)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('M,Cin,Cout', [(64, 512, 256), (8, 1024, 128), (40, 512, 512)])
def test_wide_splitk(backend, regime, M, Cin, Cout):
    with setting(backend, igemm_narrow_below=0):
        reaches_wide(M, Cout)
        reaches_wide(M, Cin)
        run_splitk(backend, regime, M, Cin, Cout)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout,G,k', [(2, 8, 16, 64, 256, 2, 1), (4, 8, 8, 128, 512, 2, 1), (2, 16, 16, 256, 128, 1, 1)])
def test_wide_folded_input_batchnorm(backend, regime, N, H, W, Cin, Cout, G, k):
    with setting(backend, igemm_narrow_below=0):
        reaches_wide(N * H * W, Cout)
        run_folded_input_batchnorm(backend, regime, N, H, W, Cin, Cout, G, k)


@pytest.mark.parametrize('regime', REGIMES)
def test_wide_dilated_forward_and_backward(backend, regime):
    """conv_fwd_dilated producing 128 channels; conv_dgrad_dilated producing 128 channels (DIL_CASES[1]: Cin = 128)"""
    N, H, W, Cin, Cout, stride, dil = 2, 12, 16, 64, 128, 1, 2
    with setting(backend, igemm_narrow_below=0):
        reaches_wide(N * H * W, Cout)
        run_dilated_forward(backend, regime, N, H, W, Cin, Cout, stride, dil)
        N, H, W, Cin, Cout, stride, dil = DIL_CASES[1]
        reaches_wide(N * H * W, Cin)
        run_dilated_backward_exact_operands(backend, DIL_CASES[1], regime)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('onek', [3, 0])
@pytest.mark.parametrize('N,H,W,Cin,Cout', [(1, 12, 12, 64, 256), (1, 12, 12, 256, 128)])
def test_wide_single_and_double_buffer_pipeline(backend, regime, onek, N, H, W, Cin, Cout):
    """1x1 on the register pipelines (igemm_ring_tiles = 0): igemm_onek = 3 (single buffer) / 0 (double buffer), one and four K-steps"""
    opts = dict(igemm_narrow_below=0, igemm_ring_tiles=0)
    if onek != OPTION_DEFAULTS['igemm_onek']:
        opts['igemm_onek'] = onek
    with setting(backend, **opts):
        reaches_wide(N * H * W, Cout)
        run_fwd(backend, regime, N, H, W, Cin, Cout, 1, 1, 0)
        if Cin % 128 == 0:
            reaches_wide(N * H * W, Cin)
            run_dgrad(backend, regime, N, H, W, Cin, Cout, 1, 1, 0)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('pipe', [5, 3, 4])
@pytest.mark.parametrize('N,H,W,Cin,Cout', [(2, 8, 8, 256, 256), (1, 5, 5, 384, 128)])      # 4 K-steps in both directions; 6 forward, ragged tile
def test_wide_ring_pipes(backend, regime, pipe, N, H, W, Cin, Cout):
    """the pure-GEMM DMA ring: PIPE 5 (32x32x16 MFMAs, default), 3 (igemm_ring_mfma32 = 0), 4 (igemm_ring_upfront = 1)"""
    opts = {5: {}, 3: dict(igemm_ring_mfma32=0), 4: dict(igemm_ring_upfront=1)}[pipe]
    with setting(backend, igemm_narrow_below=0, **opts):
        reaches_wide(N * H * W, Cout)
        reaches_ring(N * H * W, Cout, Cin)
        run_fwd(backend, regime, N, H, W, Cin, Cout, 1, 1, 0)
        if Cout >= 256:
            reaches_wide(N * H * W, Cin)
            reaches_ring(N * H * W, Cin, Cout)
            run_dgrad(backend, regime, N, H, W, Cin, Cout, 1, 1, 0)


@pytest.mark.parametrize('K', [64, 256])
@pytest.mark.parametrize('half', [0.0, 0.5, -0.5])
def test_wide_tie_block(backend, K, half):
    with setting(backend, igemm_narrow_below=0):
        reaches_wide(3 * 7 * 7, 256)
        run_tie_block(backend, K, half)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('xcd', [1, 0])
def test_wide_ten_tiles_xcd_order(backend, regime, xcd):
    """5 pixel blocks x 2 channel tiles = 10 workgroups: XCD ranges of 2, 2, 1, 1, 1, 1, 1, 1 tiles; remap on and off"""
    N, H, W = 1, 24, 24
    opts = dict(igemm_narrow_below=0)
    if xcd != OPTION_DEFAULTS['igemm_xcd']:
        opts['igemm_xcd'] = xcd
    with setting(backend, **opts):
        assert 512 < N * H * W <= 640
        reaches_wide(N * H * W, 256)
        unequal_xcd_ranges(cdiv(N * H * W, 128) * (256 // 128))
        run_fwd(backend, regime, N, H, W, 64, 256, 1, 1, 0)
        run_dgrad(backend, regime, N, H, W, 256, 64, 1, 1, 0)


@pytest.mark.parametrize('regime', REGIMES)
def test_igemm_bc_64_on_a_wide_eligible_case(backend, regime):
    N, H, W = 1, 12, 12
    with setting(backend, igemm_narrow_below=0, igemm_bc=64):
        assert cdiv(N * H * W, 128) * 2 >= FORCE['igemm_narrow_below'] and igemm_tile(N * H * W, 256) == 64
        run_fwd(backend, regime, N, H, W, 64, 256, 1, 1, 0)
        run_dgrad(backend, regime, N, H, W, 256, 64, 1, 1, 0)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout', [(2, 8, 8, 128, 64),         # one K-step: register pipeline
                                            (3, 6, 10, 128, 256)])      # K = 256: the DMA ring, ragged 128-pixel tile
def test_wide_quarter_grid_dgrad(backend, regime, N, H, W, Cin, Cout):
    """vfs_conv_dgrad_ds (the 1x1 / stride-2 dgrad on the quarter grid) with the residual add, compact and scattering form"""
    lib, d, dev = backend.lib, backend.d, backend.dev
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    g = torch.Generator().manual_seed(N + H + Cout)
    _, w, _, dy, add = operands(regime, g, N, H, W, Cin, Cout, 1, Ho, Wo)
    exact_ok(Cout, dy, w)
    _, wd = pack(backend, w)
    addq = nhwc(add)[:, ::2, ::2].contiguous()
    ref = torch.einsum('nohw,oi->nhwi', dy.double(), w[:, :, 0, 0].double()) + addq.double()
    small_ok(regime, ref)
    want = expect_bf16(ref)
    with setting(backend, igemm_narrow_below=0):
        wide, ring = ds_plan(lib, 1, N, H, W, Cin, Cout)
        assert wide and ring == (Cout >= 256), 'test bug: vfs_conv_dgrad_ds_plan does not name the instance this case is for'
        compact = nan_like((N, Ho, Wo, Cin), dev)
        lib.conv_dgrad_ds(d(nhwc(dy)), wd, compact, d(addq), 1, N, H, W, Cin, Ho, Wo, Cout, None)
        assert_bits(compact, want, 'conv_dgrad_ds, compact')
        dense = d(nhwc(add))
        lib.conv_dgrad_ds(d(nhwc(dy)), wd, dense, dense, 0, N, H, W, Cin, Ho, Wo, Cout, None)
    dense = dense.cpu()
    assert_bits(dense[:, ::2, ::2].contiguous(), want, 'conv_dgrad_ds, scattering in place')
    odd = torch.ones(H, W, dtype=torch.bool)
    odd[::2, ::2] = False
    assert torch.equal(dense[:, odd].float(), nhwc(add)[:, odd].float()), 'a pixel off the strided grid changed'


# ---------------------------------------------------------------------------------------------- 2. the non-deep halo schedule
#   N, H, W, C64, C128: the forward runs C64 -> C128, the backward cases C128 -> C64, so that both PRODUCE 128 channels
NON_DEEP = [(1, 16, 32, 128, 128),      # even 8x16 tiling, two channel chunks
            (2, 14, 14, 64, 128),       # ragged tiles
            (4, 7, 7, 64, 128)]         # whole 7x7 images in pairs


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,C64,C128', NON_DEEP)
def test_non_deep_halo_forward_and_dgrad(backend, regime, N, H, W, C64, C128):
    """forward with statistics rows and dgrad with the residual add"""
    with setting(backend, halo_deep_max=0):
        reaches_non_deep(backend, N, H, W, C64, C128, False)
        run_fwd(backend, regime, N, H, W, C64, C128, 3, 1, 1)
        reaches_non_deep(backend, N, H, W, C128, C64, True)
        run_dgrad(backend, regime, N, H, W, C128, C64, 3, 1, 1)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,C64,C128', NON_DEEP)
def test_non_deep_halo_masked_add_and_fused_bn_rows(backend, regime, N, H, W, C64, C128):
    with setting(backend, halo_deep_max=0):
        reaches_non_deep(backend, N, H, W, C128, C64, True)
        run_dgrad_masked_add_and_fused_bn_rows(backend, regime, N, H, W, C128, C64, 3)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('xcd', [1, 0])
@pytest.mark.parametrize('N,H,W,Cin,Cout', [(5, 14, 14, 64, 128),       # 128-channel kernel, 5 x 2 ragged 8x16 tiles
                                            (5, 16, 32, 64, 64)])       # 64-channel kernel, 5 x 2 tiles of 16x16
def test_halo_ten_tiles_xcd_order(backend, regime, xcd, N, H, W, Cin, Cout):
    opts = dict(halo_deep_max=0)
    if xcd != OPTION_DEFAULTS['halo_xcd']:
        opts['halo_xcd'] = xcd
    with setting(backend, **opts):
        bc, grid = halo_launch(backend, N, H, W, Cin, Cout, False)
        assert bc == Cout and grid == 10
        unequal_xcd_ranges(grid)
        if bc == 128:
            reaches_non_deep(backend, N, H, W, Cin, Cout, False)
        run_fwd(backend, regime, N, H, W, Cin, Cout, 3, 1, 1)
        bc, grid = halo_launch(backend, N, H, W, Cout, Cin, True)
        assert bc == Cout and grid == 10
        run_dgrad(backend, regime, N, H, W, Cout, Cin, 3, 1, 1)


# ---------------------------------------------------------------------------------------------- 3. weight gradient
def wgrad_both_orders(be, regime, N, H, W, Cin, Cout, k, stride, pad, nsplit, pps, tiles, eff_nsplit, halo):
    g = torch.Generator().manual_seed(N * 100 + H + Cout + 3)
    Ho, Wo = out_size(H, W, k, stride, pad)
    x, _, _, dy, _ = operands(regime, g, N, H, W, Cin, Cout, k, Ho, Wo)
    assert nsplit * pps >= N * Ho * Wo
    for xcd in (1, 0):
        with setting(be, **({} if xcd else dict(wgrad_xcd=0))):
            wgrad_swizzled(tiles, eff_nsplit)
            run_wgrad(be, regime, x, dy, k, stride, pad, nsplit, pps, halo)


@pytest.mark.parametrize('regime', REGIMES)
def test_wgrad_generic_kernel_xcd_order(backend, regime):
    """3x3 / stride 2 on an odd map (no linear addressing): 5 k-tiles x 4 splits = 20 blocks; the last split lies past M = 180"""
    N, H, W, Cin, Cout = 6, 9, 11, 64, 64
    assert not wgrad_halo_tiles(N, H, W, Cin, Cout, 3, 2, 1, lib=backend.lib)
    wgrad_both_orders(backend, regime, N, H, W, Cin, Cout, 3, 2, 1, 4, 64, generic_wgrad_tiles(Cin, Cout, 3), 4, False)


@pytest.mark.parametrize('regime', REGIMES)
def test_wgrad_ring_kernel_xcd_order(backend, regime):
    """1x1 / stride 1, Cin and Cout multiples of 128: the LDS-DMA ring (and, with wgrad_ring = 0, the linear register-staged
    kernel) on 2 x 2 tiles x 5 splits = 20 blocks"""
    N, H, W, Cin, Cout = 1, 40, 8, 256, 256
    assert (Cin >> 7) * (Cout >> 7) == generic_wgrad_tiles(Cin, Cout, 1) == 4
    wgrad_both_orders(backend, regime, N, H, W, Cin, Cout, 1, 1, 0, 5, 64, 4, 5, False)


@pytest.mark.parametrize('regime', REGIMES)
def test_wgrad_halo_kernel_xcd_order(backend, regime):
    """3x3 / stride 1: 2 x 2 blocks of 64 x 64 channels x 5 spatial tiles (one per split) = 20 blocks"""
    N, H, W, Cin, Cout = 5, 8, 16, 128, 128
    ntiles = wgrad_halo_tiles(N, H, W, Cin, Cout, 3, 1, 1, lib=backend.lib)
    assert ntiles == 5, 'test bug: vfs_conv_wgrad_plan does not send this shape to the halo kernel on five tiles'
    # vfs_wgrad_halo_dispatch: nsplit = min(offered, ntiles), tiles per split = ceil(ntiles / nsplit), effective splits =
    # ceil(ntiles / tiles per split) - offering ntiles splits gives one tile per split and ntiles effective splits
    wgrad_both_orders(backend, regime, N, H, W, Cin, Cout, 3, 1, 1, ntiles, 128, (Cin >> 6) * (Cout >> 6), ntiles, True)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('xcd', [1, 0])
def test_wgrad_dilated_kernel_xcd_order(backend, regime, xcd):
    """DIL_CASES[4]: M = 297 in 128-pixel splits, one more split than M needs: 5 k-tiles x 4 splits = 20 blocks"""
    N, H, W, Cin, Cout, stride, dil = DIL_CASES[4]
    assert stride == 1 and cdiv(N * H * W, 128) + 1 == 4
    with setting(backend, **({} if xcd else dict(wgrad_xcd=0))):
        wgrad_swizzled(generic_wgrad_tiles(Cin, Cout, 3), 4)
        run_dilated_backward_exact_operands(backend, DIL_CASES[4], regime)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout,k,stride,pad', [(3, 7, 7, 128, 64, 1, 1, 0), (2, 8, 8, 256, 256, 1, 1, 0)])
def test_wgrad_without_linear_addressing(backend, regime, N, H, W, Cin, Cout, k, stride, pad):
    """wgrad_lin = 0: a 1x1 / stride-1 layer on the gathering kernel (no linear kernel, no ring)"""
    with setting(backend, wgrad_lin=0):
        conv_exact.test_wgrad(backend, regime, N, H, W, Cin, Cout, k, stride, pad)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout,k,stride,pad', [(2, 16, 16, 64, 128, 3, 2, 1), (4, 8, 8, 128, 128, 1, 2, 0)])
def test_wgrad_without_row_linear_addressing(backend, regime, N, H, W, Cin, Cout, k, stride, pad):
    """wgrad_lin2 = 0: the evenly tiled stride-2 layers on the gathering kernel"""
    Ho, Wo = out_size(H, W, k, stride, pad)
    assert H == stride * Ho and W == stride * Wo and Wo % 4 == 0 and 64 % Wo == 0, 'test bug: no LIN = 2 shape'
    with setting(backend, wgrad_lin2=0):
        conv_exact.test_wgrad(backend, regime, N, H, W, Cin, Cout, k, stride, pad)


# ---------------------------------------------------------------------------------------------- 4. the gathering DMA ring
#   forward N, H, W, Cin, Cout, stride; dgrad: the same geometry with the channel counts swapped (produces Cout channels)
def reaches_gather_ring(Mcls, C, bc, Ktot, classes=1):
    """conv_igemm.hip vfs_conv_igemm_dispatch `gring`: a gathered problem with Ktot >= 256 and at most igemm_ring_gather tiles
    (stride-2 dgrad: four parity classes of at most Mcls pixels each)"""
    tiles = cdiv(Mcls, 128) * cdiv(C, bc) * classes
    assert Ktot >= 256 and 0 < tiles <= FORCE['igemm_ring_gather'], f'test bug: {tiles} tiles, K = {Ktot}: no gathering ring'


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('C', [64, 128])
def test_gather_ring_forward_3x3_stride2(backend, regime, C):
    N, H, W, Cin = 2, 9, 11, 64
    with setting(backend, igemm_ring_gather=4096, igemm_narrow_below=0):
        assert igemm_tile(N * 5 * 6, C) == C
        reaches_gather_ring(N * 5 * 6, C, C, 9 * Cin)
        run_fwd(backend, regime, N, H, W, Cin, C, 3, 2, 1)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('C', [64, 128])
def test_gather_ring_dgrad_3x3_stride1(backend, regime, C):
    N, H, W, Cout = 3, 7, 7, 64
    with setting(backend, igemm_ring_gather=4096, igemm_narrow_below=0, halo=0):
        assert igemm_tile(N * H * W, C) == C
        reaches_gather_ring(N * H * W, C, C, 9 * Cout)
        run_dgrad(backend, regime, N, H, W, C, Cout, 3, 1, 1)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('C', [64, 128])
def test_gather_ring_dgrad_3x3_stride2(backend, regime, C):
    N, H, W, Cout = 2, 9, 11, 64
    with setting(backend, igemm_ring_gather=4096, igemm_narrow_below=0):
        assert igemm_tile(N * H * W, C) == C
        reaches_gather_ring(N * 5 * 6, C, C, 9 * Cout, classes=4)
        run_dgrad(backend, regime, N, H, W, C, Cout, 3, 2, 1)


# ---------------------------------------------------------------------------------------------- 5. the remaining options
@pytest.mark.parametrize('bpg', [65, 300])
@pytest.mark.parametrize('opts', [dict(bn_ticket=0), dict(bn_chunk_rows=16), dict(bn_chunk_rows=300)], ids=lambda o: '-'.join(f'{n}{v}' for n, v in o.items()))
def test_bn_reduction_tails_without_tickets_and_other_chunks(backend, bpg, opts):
    """more than 64 rows per group: the chunked single-launch reduction with 16- and 300-row chunks, and the two-launch form"""
    with setting(backend, **opts):
        for C in (40, 72):
            bn_exact.test_reduction_tails(backend, bpg, C)


@pytest.mark.parametrize('target', [1, 7])
@pytest.mark.parametrize('case', [exact_f32.LP_CASES[0], exact_f32.LP_CASES[3]], ids=['five_keys_12x16', 'two_keys_20x28'])
def test_labelprop_f32_key_frame_splits(backend, target, case):
    """lpx_target = 1: every key frame in one workgroup row; 7: ceil(7 / tiles) splits (2 and 1 on these maps)"""
    with setting(backend, lpx_target=target):
        exact_f32.run_labelprop_f32(backend, **case)


def test_labelprop_two_pass_entry_without_the_two_pass_kernels(backend):
    """lp2 = 0: vfs_labelprop_f32_2pass runs the dense kernel on a 256-channel bank - the same bits"""
    c = dict(labelprop2.CASES[1])
    with setting(backend, lp2=0):
        feats, seg = labelprop2._features(c.pop('T'), c['H'], c['W'], c.pop('C'), c.pop('CO'), seed=7)
        labelprop2.run_2pass(backend, feats, seg, expect_fallback=None, **c)


@pytest.mark.parametrize('fpb', [1, 4])
def test_labelprop_two_pass_frames_per_workgroup(backend, fpb):
    """lp2_fpb: 11 key frames, one and four per workgroup"""
    with setting(backend, lp2_fpb=fpb):
        labelprop2.test_two_pass_equals_oracle(backend, labelprop2.CASES[6])


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('N,H,W,Cin,Cout', [(2, 14, 14, 64, 128),       # 77 % full 8x16 tiles
                                            (4, 7, 7, 64, 128)])        # 7x7 images: 77 % of an 8x8 tile
def test_halo_min_fill_sends_ragged_maps_to_the_gather_kernels(backend, regime, N, H, W, Cin, Cout):
    lib = backend.lib
    assert conv_plan(N, 1, H, W, Cin, Cout, 3, 1, 1, H, W, lib=lib).halo and wgrad_halo_tiles(N, H, W, Cin, Cout, 3, 1, 1, lib=lib)
    with setting(backend, halo_min_fill=100):
        assert not conv_plan(N, 1, H, W, Cin, Cout, 3, 1, 1, H, W, lib=lib).halo
        assert not conv_plan(N, 1, H, W, Cout, Cin, 3, 1, 1, H, W, dgrad=True, lib=lib).halo
        assert not wgrad_halo_tiles(N, H, W, Cin, Cout, 3, 1, 1, lib=lib)
        run_fwd(backend, regime, N, H, W, Cin, Cout, 3, 1, 1)
        run_dgrad(backend, regime, N, H, W, Cout, Cin, 3, 1, 1)
        conv_exact.test_wgrad(backend, regime, N, H, W, Cin, Cout, 3, 1, 1)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('min_tiles', [4, 5])
def test_persistent_pointwise_kernel_from_a_tile_count_on(backend, regime, min_tiles):
    """igemm_pw = 1 takes the persistent 1x1 kernel from igemm_pw_min_tiles 128-channel tiles on (conv_pw.hip
    vfs_conv_pw_eligible): [144][256] is 2 x 2 = 4 tiles - persistent with a threshold of 4, implicit-GEMM with 5"""
    N, H, W = 1, 12, 12
    with setting(backend, igemm_pw=1, igemm_pw_min_tiles=min_tiles):
        assert (cdiv(N * H * W, 128) * (256 // 128) >= FORCE['igemm_pw_min_tiles']) == (min_tiles == 4)
        run_fwd(backend, regime, N, H, W, 64, 256, 1, 1, 0)
        run_dgrad(backend, regime, N, H, W, 256, 64, 1, 1, 0)


# ---------------------------------------------------------------------------------------------- completeness
# option -> the tests of this file whose kernel launches run under a non-default value of it
SWEPT = {
    'halo': ['test_wide_forward', 'test_wide_dgrad', 'test_wide_dgrad_masked_add_and_fused_bn_rows', 'test_gather_ring_dgrad_3x3_stride1'],
    'halo_min_fill': ['test_halo_min_fill_sends_ragged_maps_to_the_gather_kernels'],
    'halo_deep_max': ['test_non_deep_halo_forward_and_dgrad', 'test_non_deep_halo_masked_add_and_fused_bn_rows', 'test_halo_ten_tiles_xcd_order'],
    'halo_xcd': ['test_halo_ten_tiles_xcd_order'],
    'bn_ticket': ['test_bn_reduction_tails_without_tickets_and_other_chunks'],
    'bn_chunk_rows': ['test_bn_reduction_tails_without_tickets_and_other_chunks'],
    'igemm_bc': ['test_igemm_bc_64_on_a_wide_eligible_case'],
    'igemm_xcd': ['test_wide_ten_tiles_xcd_order'],
    'igemm_narrow_below': ['test_wide_forward', 'test_wide_dgrad', 'test_wide_dgrad_masked_add_and_fused_bn_rows', 'test_wide_splitk',
                           'test_wide_folded_input_batchnorm', 'test_wide_dilated_forward_and_backward',
                           'test_wide_single_and_double_buffer_pipeline', 'test_wide_ring_pipes', 'test_wide_tie_block',
                           'test_wide_ten_tiles_xcd_order', 'test_wide_quarter_grid_dgrad'],
    'igemm_onek': ['test_wide_single_and_double_buffer_pipeline'],
    'igemm_ring_tiles': ['test_wide_single_and_double_buffer_pipeline'],
    'igemm_ring_fbn': ['test_wide_dgrad_masked_add_and_fused_bn_rows'],
    'igemm_ring_mfma32': ['test_wide_ring_pipes'],
    'igemm_ring_upfront': ['test_wide_ring_pipes'],
    'igemm_ring_gather': ['test_gather_ring_forward_3x3_stride2', 'test_gather_ring_dgrad_3x3_stride1', 'test_gather_ring_dgrad_3x3_stride2'],
    'igemm_pw_min_tiles': ['test_persistent_pointwise_kernel_from_a_tile_count_on'],
    'wgrad_lin': ['test_wgrad_without_linear_addressing'],
    'wgrad_lin2': ['test_wgrad_without_row_linear_addressing'],
    'wgrad_xcd': ['test_wgrad_generic_kernel_xcd_order', 'test_wgrad_ring_kernel_xcd_order', 'test_wgrad_halo_kernel_xcd_order',
                  'test_wgrad_dilated_kernel_xcd_order'],
    'lpx_target': ['test_labelprop_f32_key_frame_splits'],
    'lp2': ['test_labelprop_two_pass_entry_without_the_two_pass_kernels'],
    'lp2_fpb': ['test_labelprop_two_pass_frames_per_workgroup'],
}
# option -> the test file whose kernel launches already run under a non-default value, or the reason why none does
WHAT_IF = 'a what-if knob: gives wrong results by design'
ELSEWHERE = {
    'stem_direct': 'test_conv_exact.py', 'stem_blocks': 'test_conv_exact.py', 'igemm_mfma_stats': 'test_conv_exact.py',
    'igemm_skinny': 'test_conv_exact.py', 'igemm_pw': 'test_conv_exact.py', 'wgrad_ring': 'test_conv_exact.py',
    'bn_wide': 'test_emu_bn.py', 'bn_wide_min_mb': 'test_bn_exact.py',
    'lpx_wgs': 'test_exact_f32.py', 'lpx_minb': 'test_exact_f32.py', 'conv_f32_variant': 'test_exact_f32.py',
    'lp2_trim': 'test_labelprop2.py', 'lp2_xcd': 'test_labelprop2.py', 'lp2_cap': 'test_labelprop2.py',
    'igemm_ds_quarter': 'test_downsample_dgrad_compact.py',
    'lp2_dbg': WHAT_IF, 'conv_f32_dbg': WHAT_IF,
}


def library_option_table():
    """name -> default of every X(name, default) line of csrc/vfs_options.h, the one list the library's switchboard is built from"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'vfs_amd', 'csrc', 'vfs_options.h')).read()
    return {n: int(v) for n, v in re.findall(r'^\s*X\((\w+),\s*(-?\d+)\)', src, re.M)}


def check_option_tables(swept, elsewhere):
    import inspect
    import os
    import re
    import sys
    table = library_option_table()
    assert len(table) >= 39 and table == OPTION_DEFAULTS, f'OPTION_DEFAULTS is not the option table of csrc/vfs_options.h: {sorted(set(table.items()) ^ set(OPTION_DEFAULTS.items()))}'
    assert set(swept) | set(elsewhere) == set(table), sorted(set(table) ^ (set(swept) | set(elsewhere)))
    here = sys.modules[__name__]
    for name, tests in swept.items():
        assert tests, name
        for t in tests:
            src = inspect.getsource(getattr(here, t))
            if 'wgrad_both_orders(' in src:
                src += inspect.getsource(wgrad_both_orders)
            assert re.search(rf"\b{name}(=|'\] = )", src), f'{t} does not set {name}'
    for name, where in elsewhere.items():
        if where == WHAT_IF:
            assert name.endswith('_dbg'), f'{name}: only the *_dbg knobs may go without a kernel test'
            continue
        src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), where)).read()
        assert f"set_option(b'{name}'" in src or re.search(rf"options\([^\n]*\(b'{name}', ", src), f'{where} does not set {name}'


def test_every_option_is_swept_somewhere():
    """every name of the option table is set by a test of this file that launches kernels under it (SWEPT) or by the named
    test file (ELSEWHERE); an option added without a kernel test - or an entry removed from either table - fails here"""
    check_option_tables(SWEPT, ELSEWHERE)
    for table in (SWEPT, ELSEWHERE):
        for name in table:
            less = {n: v for n, v in table.items() if n != name}
            with pytest.raises(AssertionError):
                check_option_tables(*((less, ELSEWHERE) if table is SWEPT else (SWEPT, less)))
