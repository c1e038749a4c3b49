"""The dgrad of a 1x1 / stride-2 / pad-0 convolution (ResNet's downsample branch) on the quarter grid: vfs_conv_dgrad_ds and
the routing of vfs_conv_dgrad_maskadd (option igemm_ds_quarter) against the dense stride-2 dgrad on the same bf16 operands.

Where the gradients meet.  At a stage entry the engine runs the residual branch's first dgrad into `gin` and then the downsample
dgrad with add = gin, g_out = gin (ResNet._block_bwd): the downsample dgrad ITSELF is the join, in place, and no other epilogue
ever adds its result.  So the quarter-grid form keeps that shape: the pure GEMM over the N * ceil(H/2) * ceil(W/2) pixels of dy
reads `add` and writes `dx` at the even-even pixels of the dense tensor and touches nothing else; the three parity classes
without a tap, whose workgroups only copied `add` onto itself, are gone.  The join carries no ReLU mask and no fused
BatchNorm-backward statistics (a stride-2 dgrad never emitted rows; the engine passes the downsample unit no add_mask), so the
mask / statistics variants have no quarter-grid counterpart: a masked call stays on the dense path, which a case below pins.

Summation order.  The dense classes run the 16x16x32-MFMA K loop, one K-step after the other.  The quarter grid runs the
instance a 1x1 / stride-1 dgrad of the same M, K, Cout gets (vfs_conv_dgrad_ds_plan): the register pipelines and the PIPE 3
ring have the same MFMA shape and K order - bit equality is required there - while the default ring (32x32x16 MFMAs, taken for
K >= 256: cases b and d) sums a K-step in another order.  There both results are held against the float64 product of the same
bf16 operands: the quarter grid's largest error may exceed the dense path's by at most one bf16 rounding of the output
(2^-8 of the largest |reference|).  Case (d) is a shape the plan sends to the ring with more K-steps than ring stages."""
import pytest
import torch

from tests.emu_util import nhwc, rb
from tests.test_emu_conv import pack
from vfs_amd.engine import ConvUnit
from vfs_amd.resnet import BasicBlock, ConvBN, ResNet

BF16 = torch.bfloat16

#        N, H,  W,  Cin, Cout
CASES = {'a': (2, 8, 8, 64, 128),
         'b': (3, 6, 10, 128, 256),      # 15 quarter-grid pixels per image, ragged 128-pixel tile; K = 256: the DMA ring
         'c': (1, 7, 9, 64, 64),         # odd sizes: ceil(H / 2), last row and column
         'd': (2, 16, 16, 128, 512)}     # ring with 8 K-steps (more than its stages), a full 128-pixel tile
# option settings that move a launch to another instance of the kernel: (name, value, default)
VARIANTS = {'default': (), 'pipe0': ((b'igemm_onek', 0, 3),), 'ring3': ((b'igemm_ring_mfma32', 0, 1),),
            'wide': ((b'igemm_narrow_below', 0, 513),), 'noring': ((b'igemm_ring_tiles', 0, 512),)}
RUNS = [(c, 'default') for c in CASES] + [('a', 'pipe0'), ('d', 'wide'), ('b', 'ring3'), ('b', 'wide'), ('b', 'noring'), ('c', 'pipe0')]


class options:
    def __init__(self, lib, settings):
        self.lib, self.settings = lib, settings

    def __enter__(self):
        for name, value, _ in self.settings:
            self.lib.set_option(name, value)

    def __exit__(self, *exc):
        for name, _, default in self.settings:
            self.lib.set_option(name, default)


def plan(lib, compact, N, H, W, Cin, Cout):
    out = torch.zeros(2, dtype=torch.int32)
    lib.conv_dgrad_ds_plan(compact, N, H, W, Cin, (H + 1) // 2, (W + 1) // 2, Cout, out[0:], out[1:])
    wide, ring = out.tolist()
    return bool(wide), bool(ring)


def operands(be, case):
    N, H, W, Cin, Cout = CASES[case]
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    g = torch.Generator().manual_seed(N * 101 + H * 7 + Cin + Cout)
    w = rb(torch.randn(Cout, Cin, 1, 1, generator=g) * (2.0 / Cout) ** 0.5)
    dy = rb(torch.randn(N, Cout, Ho, Wo, generator=g))
    gin = rb(torch.randn(N, H, W, Cin, generator=g)).to(BF16)
    _, wd = pack(be, w)
    ref = torch.einsum('nohw,oi->nhwi', dy.double(), w[:, :, 0, 0].double())      # [N,Ho,Wo,Cin], exact products of the bf16 operands
    return (N, H, W, Cin, Cout, Ho, Wo), be.d(nhwc(dy)), wd, gin, ref


def same_order(lib, variant, dims):
    """does the quarter-grid launch sum in the order of the dense parity-class kernel?  (everything but the 32x32x16-MFMA ring)"""
    N, H, W, Cin, Cout, Ho, Wo = dims
    _, ring = plan(lib, 0, N, H, W, Cin, Cout)
    return not ring or variant == 'ring3'


def check(got, dense, ref, exact, what):
    """got, dense: [N,Ho,Wo,Cin] bf16 results of the two paths; ref: float64.  Prints the figures, then asserts"""
    eg, ed = float((got.double() - ref).abs().max()), float((dense.double() - ref).abs().max())
    eps = float(ref.abs().max()) * 2.0 ** -8
    ndiff = int((got.double() != dense.double()).sum())
    print(f'{what}: max error quarter grid {eg:.4e}, dense {ed:.4e}, one bf16 rounding {eps:.4e}, {ndiff} of {got.numel()} values differ')
    assert torch.isfinite(got.float()).all(), what
    assert eg <= ed + eps, f'{what}: quarter grid {eg} > dense {ed} + {eps}'
    if exact:
        assert ndiff == 0, f'{what}: same summation order, yet {ndiff} values differ'


@pytest.mark.parametrize('case,variant', RUNS)
def test_quarter_grid_dgrad_against_dense_stride2_dgrad(backend, case, variant):
    """no add: every even-even pixel of the dense result equals the compact tensor (bit for bit where the order is the same, within
    the bound otherwise), every other pixel of the dense result is exactly zero; the scattering form writes the same values to the
    even-even pixels of a dense tensor and leaves every other pixel as it was"""
    lib, dev = backend.lib, backend.dev
    dims, dy, wd, _, ref = operands(backend, case)
    N, H, W, Cin, Cout, Ho, Wo = dims
    with options(lib, VARIANTS[variant]):
        wide, ring = plan(lib, 0, N, H, W, Cin, Cout)
        if case in ('b', 'd') and variant == 'default':
            assert ring, 'the plan no longer sends K >= 256 downsample shapes to the DMA ring: revisit the cases'
        if variant == 'wide':
            assert wide
        dense = torch.full((N, H, W, Cin), float('nan'), dtype=BF16, device=dev)
        lib.conv_dgrad(dy, wd, dense, None, N, H, W, Cin, Ho, Wo, Cout, 1, 1, 2, 0, None)
        compact = torch.full((N, Ho, Wo, Cin), float('nan'), dtype=BF16, device=dev)
        lib.conv_dgrad_ds(dy, wd, compact, None, 1, N, H, W, Cin, Ho, Wo, Cout, None)
        scat = torch.full((N, H, W, Cin), 7.0, dtype=BF16, device=dev)
        lib.conv_dgrad_ds(dy, wd, scat, None, 0, N, H, W, Cin, Ho, Wo, Cout, None)
        exact = same_order(lib, variant, dims)
    dense, compact, scat = dense.cpu(), compact.cpu(), scat.cpu()
    odd = torch.ones(H, W, dtype=torch.bool)
    odd[::2, ::2] = False
    assert (dense[:, odd].float() == 0).all(), 'a pixel off the strided grid received a gradient'
    assert (scat[:, odd].float() == 7.0).all(), 'the scattering epilogue wrote off the strided grid'
    check(compact, dense[:, ::2, ::2], ref, exact, f'{case}/{variant} compact')
    check(scat[:, ::2, ::2], dense[:, ::2, ::2], ref, exact, f'{case}/{variant} scatter')
    # (compact and scatter run one kernel family on one tiling; the ring re-fetches rows past M and masks them in both)
    assert torch.equal(scat[:, ::2, ::2].float(), compact.float())


@pytest.mark.parametrize('case,variant', RUNS)
def test_in_place_join_against_dense_add(backend, case, variant):
    """the stage-entry join: vfs_conv_dgrad_maskadd(add = dx = the residual branch's gradient) with igemm_ds_quarter on (quarter
    grid) and off (four parity classes).  Pixels off the strided grid keep the residual gradient bit for bit on both paths; the
    even-even pixels are equal bit for bit where the summation order is the same, else within the bound (the add happens in fp32
    before the one rounding on both paths, so the reference is product + residual).  The compact form with an add operand of its
    own gives the same values."""
    lib, dev = backend.lib, backend.dev
    dims, dy, wd, gin, ref = operands(backend, case)
    N, H, W, Cin, Cout, Ho, Wo = dims
    res = {}
    with options(lib, VARIANTS[variant]):
        for on in (0, 1):
            with options(lib, ((b'igemm_ds_quarter', on, 1),)):
                dx = gin.clone().to(dev)
                lib.conv_dgrad_maskadd(dy, wd, dx, dx, None, N, H, W, Cin, Ho, Wo, Cout, 1, 1, 2, 0, None)
                res[on] = dx.cpu()
        addc = gin[:, ::2, ::2].contiguous().to(dev)
        compact = torch.full((N, Ho, Wo, Cin), float('nan'), dtype=BF16, device=dev)
        lib.conv_dgrad_ds(dy, wd, compact, addc, 1, N, H, W, Cin, Ho, Wo, Cout, None)
        exact = same_order(lib, variant, dims)
    odd = torch.ones(H, W, dtype=torch.bool)
    odd[::2, ::2] = False
    for on in (0, 1):
        assert torch.equal(res[on][:, odd].float(), gin[:, odd].float()), f'igemm_ds_quarter={on}: a pixel off the strided grid changed'
    want = ref + gin[:, ::2, ::2].double()
    check(res[1][:, ::2, ::2], res[0][:, ::2, ::2], want, exact, f'{case}/{variant} in-place join')
    assert torch.equal(compact.cpu().float(), res[1][:, ::2, ::2].float())


def test_masked_add_stays_on_the_dense_path(backend):
    """a mask-gated add (never passed for a downsample unit) is not routed to the quarter grid: same bits with the option on and off"""
    from tests.emu_util import pack_relu_mask
    lib, dev = backend.lib, backend.dev
    dims, dy, wd, gin, _ = operands(backend, 'a')
    N, H, W, Cin, Cout, Ho, Wo = dims
    y = torch.relu(torch.randn(N, H, W, Cin, generator=torch.Generator().manual_seed(3)))
    bits = pack_relu_mask(y).to(dev)
    res = []
    for on in (0, 1):
        with options(lib, ((b'igemm_ds_quarter', on, 1),)):
            dx = gin.clone().to(dev)
            lib.conv_dgrad_maskadd(dy, wd, dx, dx, bits, N, H, W, Cin, Ho, Wo, Cout, 1, 1, 2, 0, None)
            res.append(dx.cpu())
    assert torch.equal(res[0].float(), res[1].float())
    assert torch.equal(res[0][:, 1::2].float(), torch.where(y > 0, gin.float(), torch.zeros(()))[:, 1::2])


def test_geometry_errors(emu_backend):
    from vfs_amd._lib import VfsError
    lib = emu_backend.lib
    P = torch.zeros(1 << 14, dtype=BF16)
    with pytest.raises(VfsError, match='ceil'):
        lib.conv_dgrad_ds(P, P, P, None, 0, 1, 7, 9, 64, 3, 5, 64, None)      # Ho must be 4
    with pytest.raises(VfsError, match='null operand'):
        lib.conv_dgrad_ds(P, P, None, None, 0, 1, 8, 8, 64, 4, 4, 64, None)


def _stage_entry(be, quarter):
    """forward and backward of ResNet-18's layer2 entry block (64 -> 128 channels, stride 2, 1x1 downsample) through the engine"""
    eng, dev = be.eng, be.dev
    N, H, W, G = 2, 16, 16, 1
    torch.manual_seed(11)
    cfg = dict(type='BN')
    blk = BasicBlock(64, 128, 2, ConvBN(64, 128, 1, 2, 0, cfg, False), cfg).to(dev).train()
    for p in blk.parameters():
        p.grad = torch.zeros_like(p)
    for name, m in [('conv1', blk.conv1), ('conv2', blk.conv2), ('downsample', blk.downsample)]:
        k = m.conv.kernel_size[0]
        m.unit = eng.register(ConvUnit(f'entry{quarter}.{name}', m.conv.weight, None, m.bn, k, m.conv.stride[0], m.conv.padding[0]))
    eng.pack_weights()
    gen = torch.Generator().manual_seed(12)
    x = torch.relu(torch.randn(N, H, W, 64, generator=gen)).to(BF16).to(dev)
    g = torch.randn(N, H // 2, W // 2, 128, generator=gen).to(BF16).to(dev)
    with options(eng.lib, ((b'igemm_ds_quarter', quarter, 1),)):
        _, _, _, bctx = ResNet._block_fwd(None, eng, blk, x, N, H, W, G, True)
        gin, _ = ResNet._block_bwd(None, eng, bctx, g, N, G, next_bn=None, need_input_grad=True)
        eng.wgrad_join(dev)
        if dev.type == 'cuda':
            torch.cuda.synchronize()
    out = {n: p.grad.detach().cpu().clone() for n, p in blk.named_parameters()}
    out['input gradient'] = gin.float().cpu().clone()
    return out


def test_stage_entry_block_through_the_engine(backend):
    """option on against option off at N = 2, 16x16, 64 -> 128 channels, stride 2: the downsample dgrad (K = 128: register pipeline
    on both paths, same summation order) completes the block's input gradient in place - every parameter gradient and the input
    gradient are bit-identical"""
    on, off = _stage_entry(backend, 1), _stage_entry(backend, 0)
    assert set(on) == set(off) and len(on) == 10
    for name in on:
        assert torch.isfinite(on[name]).all() and float(on[name].abs().max()) > 0, name
        assert torch.equal(on[name], off[name]), f'{name}: {int((on[name] != off[name]).sum())} values differ'
