"""The tiling plan is the library's: what vfs_conv_plan / vfs_conv_wgrad_plan / vfs_stem_plan answer is what the launches
do, under the default options and under the A/B switches that move a layer to another kernel family (halo = 0,
halo_min_fill = 100).  Exact operands (tests/test_conv_exact.py, regime A): every row sum has one correct value.

Every statistics buffer is sized from the shapes alone for the LARGER of the two row layouts (spatial tiles, linear
128-pixel blocks) plus a guard row and pre-filled with NaN, so a query that disagrees with the kernel fails an assertion
and never writes out of bounds.

backend=emu: host build through the fiber emulator; backend=gpu: libvfs_hip.so on the MI355X."""
import pytest
import torch
import torch.nn.functional as F

from tests.emu_util import nhwc
from tests.test_conv_exact import (BF16, assert_bits, bn_rows_check, check_stats_rows, exact_ok, expect_bf16, im2col64, ints, nan_like,
                                   nhwc64, oihw, operands, out_size, small_ok)
from tests.test_emu_conv import pack
from vfs_amd.packing import conv_plan, stem_stats_rows, wgrad_halo_tiles, wgrad_splits

OPTION_DEFAULTS = dict(halo=1, halo_min_fill=70, stem_direct=1)
OPTIONS = [pytest.param({}, id='default'), pytest.param(dict(halo=0), id='halo=0'), pytest.param(dict(halo_min_fill=100), id='halo_min_fill=100')]
SHAPES = [  # N, H, W, Cin, Cout, k, stride, pad
    (3, 14, 14, 64, 128, 3, 1, 1),      # ragged 8x16 tiles: 6 tile rows, 5 linear ones
    (4, 8, 8, 64, 128, 3, 1, 1),        # whole images in pairs
    (2, 16, 16, 64, 64, 3, 1, 1),       # 16x16 tiles
    (2, 7, 7, 64, 128, 3, 1, 1),        # 7x7: whole images in pairs at 70 % fill, 38 % of an 8x16 tile (never taken) at 100 %
    (2, 9, 7, 64, 64, 1, 1, 0),         # 1x1
    (2, 16, 16, 64, 128, 3, 2, 1),      # stride 2
]


class options:
    """the A/B switches of one case, back at their defaults afterwards"""

    def __init__(self, lib, opts):
        self.lib, self.opts = lib, opts

    def __enter__(self):
        for name, value in self.opts.items():
            self.lib.set_option(name.encode(), value)

    def __exit__(self, *exc):
        for name in self.opts:
            self.lib.set_option(name.encode(), OPTION_DEFAULTS[name])


def row_cap(N, Ho, Wo):
    """rows of the larger layout for an [N,Ho,Wo] output - 8x16 tiles, 16x16 tiles of two rows, linear blocks - plus the guard"""
    return max(N * ((Ho + 7) // 8) * ((Wo + 15) // 16), N * ((Ho + 15) // 16) * ((Wo + 15) // 16) * 2, (N * Ho * Wo + 127) // 128) + 1


def check_written(buf, rows, what):
    """exactly the first `rows` rows of the NaN-filled buffer were written; the guard row and everything beyond were not"""
    st = buf.cpu()
    assert rows is not None and 0 < rows < st.shape[0], f'{what}: queried {rows} rows, buffer of {st.shape[0]}'
    assert bool(torch.isfinite(st[:rows]).all()), f'{what}: unwritten values in the {rows} queried rows'
    assert bool(torch.isnan(st[rows:]).all()), f'{what}: rows written beyond the {rows} queried'
    return st[:rows]


@pytest.mark.parametrize('opts', OPTIONS)
@pytest.mark.parametrize('N,H,W,Cin,Cout,k,stride,pad', SHAPES)
def test_forward_writes_the_queried_rows(backend, opts, N, H, W, Cin, Cout, k, stride, pad):
    lib, d, dev = backend.lib, backend.d, backend.dev
    g = torch.Generator().manual_seed(N * 100 + H + Cout)
    Ho, Wo = out_size(H, W, k, stride, pad)
    x, w, _, _, _ = operands('A', g, N, H, W, Cin, Cout, k, Ho, Wo)
    exact_ok(k * k * Cin, x, w)
    wf, _ = pack(backend, w)
    ref = nhwc64(F.conv2d(x.double(), w.double(), None, stride, pad))
    small_ok('A', ref)
    want = expect_bf16(ref)
    y, stats = nan_like((N, Ho, Wo, Cout), dev), nan_like((row_cap(N, Ho, Wo), 2, Cout), dev, torch.float32)
    with options(lib, opts):
        plan = conv_plan(N, 1, H, W, Cin, Cout, k, stride, pad, Ho, Wo, lib=lib)
        lib.conv_fwd(d(nhwc(x)), wf, y, None, stats, N, H, W, Cin, Ho, Wo, Cout, k, k, stride, pad, None)
    what = f'conv_fwd under {opts or "the default options"}'
    assert_bits(y, want, what)
    if (N, H, W) == (3, 14, 14):      # 3 x ceil(14 / 8) x ceil(14 / 16) tiles, ceil(588 / 128) linear blocks
        assert (plan.halo, plan.rows) == ((True, 6) if not opts else (False, 5))
    st = check_written(stats, plan.rows, what)
    check_stats_rows('A', st, want.double().reshape(-1, Cout), not plan.halo, 1, what)


@pytest.mark.parametrize('opts', OPTIONS)
@pytest.mark.parametrize('N,H,W,Cin,Cout,k,stride,pad', [s for s in SHAPES if s[6] == 1])
def test_dgrad_bn_writes_the_queried_rows(backend, opts, N, H, W, Cin, Cout, k, stride, pad):
    """the BatchNorm-backward rows of vfs_conv_dgrad_bn (mask recomputed from x scale + shift; dyadic parameters, invstd = 1)"""
    lib, d, dev = backend.lib, backend.d, backend.dev
    g = torch.Generator().manual_seed(N * 13 + H + Cin + k)
    _, w, _, dy, _ = operands('A', g, N, H, W, Cin, Cout, k, H, W)
    exact_ok(k * k * Cout, dy, w)
    _, wd = pack(backend, w)
    ref = nhwc64(torch.nn.grad.conv2d_input((N, Cin, H, W), w.double(), dy.double(), 1, pad))
    small_ok('A', ref)
    want = expect_bf16(ref)
    M = N * H * W
    x = ints(g, (N, H, W, Cin), -3, 3)
    scale = 2.0 ** ints(g, (Cin,), -1, 1)
    shift, mean = ints(g, (Cin,), -4, 4) / 2, ints(g, (Cin,), -4, 4) / 2
    bnp = torch.stack([scale, shift, mean, torch.ones(Cin)], 0).reshape(1, 4, Cin).contiguous()
    dx, part = nan_like((N, H, W, Cin), dev), nan_like((row_cap(N, H, W), 2, Cin), dev, torch.float32)
    with options(lib, opts):
        plan = conv_plan(N, 1, H, W, Cin, Cout, k, 1, pad, H, W, dgrad=True, lib=lib)
        lib.conv_dgrad_bn(d(nhwc(dy)), wd, dx, None, d(x.to(BF16)), None, d(bnp), part, M, 1, N, H, W, Cin, H, W, Cout, k, k, 1, pad, None)
    what = f'conv_dgrad_bn under {opts or "the default options"}'
    assert_bits(dx, want, what)
    rows = check_written(part, plan.rows, what)
    xq = x.double().reshape(M, Cin)
    relu = ((xq * scale.double() + shift.double()) > 0).double()
    bn_rows_check('A', rows, want.double().reshape(M, Cin), xq, mean.double(), relu, not plan.halo, what)


@pytest.mark.parametrize('opts', OPTIONS)
@pytest.mark.parametrize('N,H,W,Cin,Cout,k,stride,pad', SHAPES)
def test_wgrad_takes_the_plan_offered_from_the_query(backend, opts, N, H, W, Cin, Cout, k, stride, pad):
    """vfs_conv_wgrad on the split plan that wgrad_splits builds from vfs_conv_wgrad_plan's answer: the exact gradient; the
    generic kernel (no halo tiles) wrote every slice as the sum over its linear pixel range, the halo kernel took every offered
    split (a tile count other than the kernel's own would leave offered slices unwritten) and the slices add up"""
    lib, d, dev = backend.lib, backend.d, backend.dev
    g = torch.Generator().manual_seed(N * 100 + H + Cout + 2)
    Ho, Wo = out_size(H, W, k, stride, pad)
    x, _, _, dy, _ = operands('A', g, N, H, W, Cin, Cout, k, Ho, Wo)
    M, Ktot = N * Ho * Wo, k * k * Cin
    exact_ok(M, x, dy)
    grad0 = ints(g, (Cout, Cin, k, k), -5, 5)
    with options(lib, opts):
        ntiles = wgrad_halo_tiles(N, H, W, Cin, Cout, k, stride, pad, lib=lib)
        nsplit, pps = wgrad_splits(M, Cout, Ktot, target_blocks=12, halo_geom=(N, H, W, Cin) if ntiles else None, lib=lib)
        partial, grad = nan_like((nsplit, Cout, Ktot), dev, torch.float32), d(grad0.clone())
        lib.conv_wgrad(d(nhwc(dy)), d(nhwc(x)), partial, grad, N, H, W, Cin, Ho, Wo, Cout, k, k, stride, pad, nsplit, pps, None)
    what = f'conv_wgrad under {opts or "the default options"}, {ntiles} halo tiles'
    if k != 3 or stride != 1 or opts.get('halo') == 0:
        assert ntiles == 0, what
    cols, dym = im2col64(x, k, stride, pad), nhwc64(dy.double()).reshape(M, Cout)
    dw = dym.t() @ cols
    assert_bits(grad, (grad0.double() + oihw(dw, Cout, Cin, k)).float(), what, pixels=False)
    p = partial.cpu()
    if ntiles:
        assert nsplit <= ntiles and bool(torch.isfinite(p).all()), f'{what}: an offered split was not taken'
        assert_bits(p.double().sum(0), dw, f'{what}: sum of the slices')
    else:
        slices = torch.stack([dym[s * pps:(s + 1) * pps].t() @ cols[s * pps:(s + 1) * pps] for s in range(nsplit)])
        assert_bits(p, slices.float(), f'{what}: slices over linear pixel ranges')


@pytest.mark.parametrize('opts', [pytest.param({}, id='default'), pytest.param(dict(stem_direct=0), id='stem_direct=0')])
def test_stem_writes_the_queried_rows(backend, opts):
    """vfs_stem_fwd: one row per 8x16 tile from the direct kernel, one per 128 pixels on the implicit-GEMM path"""
    lib, d, dev = backend.lib, backend.d, backend.dev
    g = torch.Generator().manual_seed(7)
    N, H, W = 2, 20, 18
    x = ints(g, (N, 3, H, W), -2, 2)
    w = (ints(g, (64, 3, 7, 7), 0, 1) * 2 - 1) * (torch.rand(64, 3, 7, 7, generator=g) < 0.25)
    wf, _ = pack(backend, w, stem=True)
    Ho, Wo = out_size(H, W, 7, 2, 3)
    x4 = torch.zeros(N, H, W, 4, dtype=BF16)
    x4[..., :3] = x.permute(0, 2, 3, 1)
    ref = nhwc64(F.conv2d(x.double(), w.double(), None, 2, 3))
    small_ok('A', ref)
    want = expect_bf16(ref)
    y, stats = nan_like((N, Ho, Wo, 64), dev), nan_like((row_cap(N, Ho, Wo), 2, 64), dev, torch.float32)
    with options(lib, opts):
        rows = stem_stats_rows(N, 1, H, W, Ho, Wo, lib=lib)
        lib.stem_fwd(d(x4), wf, y, stats, N, H, W, Ho, Wo, None)
    what = f'stem_fwd under {opts or "the default options"}'
    assert_bits(y, want, what)
    assert rows == (N * 2 * 1 if not opts else (N * Ho * Wo + 127) // 128)      # 10 x 9 outputs: two 8x16 tiles per image; 180 pixels
    st = check_written(stats, rows, what)
    check_stats_rows('A', st, want.double().reshape(-1, 64), bool(opts), 1, what)


def test_engine_statistics_follow_the_library_with_halo_off(backend):
    """Engine.conv_fwd + bn_act on a 3x3 unit whose launch leaves the halo kernels (halo = 0): 5 linear rows where the halo
    kernel writes 6 tile rows.  The engine sizes the row buffer and tells bn_act how many rows to sum from the library's
    answer, so the finished sums are those of the stored output (a host that counted 6 would add a row nobody wrote)."""
    from vfs_amd.engine import ConvUnit
    eng, lib, dev = backend.eng, backend.lib, backend.dev
    N, H, W, Cin, Cout = 3, 14, 14, 64, 128
    g = torch.Generator().manual_seed(314)
    x, w, _, _, _ = operands('A', g, N, H, W, Cin, Cout, 3, H, W)
    bn = torch.nn.BatchNorm2d(Cout).to(dev).train()
    u = eng.register(ConvUnit('plan_test.conv', torch.nn.Parameter(w.to(dev)), None, bn, 3, 1, 1))
    eng.pack_weights()
    eng.ws('ws.stats', 8 * 2 * Cout, torch.float32, dev).fill_(float('nan'))      # the row workspace starts out unwritten
    with options(lib, dict(halo=0)):
        raw, Ho, Wo, fin = eng.conv_fwd(u, nhwc(x).to(dev), N, H, W, 1, True, defer_fin=True)
        eng.bn_act(u, raw, N * Ho * Wo, 1, True, True, fin=fin)
    yq = raw.float().cpu().double().reshape(-1, Cout)
    assert_bits(raw, expect_bf16(nhwc64(F.conv2d(x.double(), w.double(), None, 1, 1))), 'Engine.conv_fwd with halo = 0')
    assert float(yq.abs().max()) ** 2 * yq.shape[0] < 2 ** 24      # every partial sum is exact in fp32
    sums = u.sums.cpu()
    assert_bits(sums[0, 0], yq.sum(0), 'sums of the unit')
    assert_bits(sums[0, 1], (yq * yq).sum(0), 'sums of squares of the unit')
