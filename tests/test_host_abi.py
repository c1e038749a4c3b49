"""CPU checks of the boundary: the C-ABI library loads and exports every symbol the header
declares, configs (ours and -- when present -- the reference's own files) build through the
registry with the reference's state_dict names, error behaviour matches the reference's tests."""
import os

import pytest
import torch

import vfs_amd
from vfs_amd import _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CFG = '/root/reference/configs'


def test_library_exports_every_declared_symbol():
    path = build.build_hip()
    protos = _lib.parse_header()
    assert len(protos) >= 25 and 'vfs_conv_fwd' in protos and 'vfs_last_error' in protos
    lib = _lib.VfsLib(path)                     # resolves every prototype or raises
    assert lib.dll.vfs_abi_version() == 3 == _lib.ABI_VERSION
    import subprocess
    syms = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True).stdout
    for name in protos:
        assert f' T {name}' in syms, name


def test_labelprop_workspace_query_is_host_only():
    """vfs_labelprop_workspace_bytes: the size contract of the label propagation workspace (no GPU involved), and its argument check"""
    lib = _lib.VfsLib(build.build_hip())
    n = torch.zeros(1, dtype=torch.int64)
    lib.labelprop_workspace_bytes(60, 107, n)
    assert n.item() == 96 * 60 * 107 * 10 * 8
    with pytest.raises(_lib.VfsError, match='labelprop_workspace_bytes'):
        lib.labelprop_workspace_bytes(0, 107, n)
    with pytest.raises(_lib.VfsError):
        lib.labelprop_workspace_bytes(60, 107, None)


def test_plan_queries_are_host_only():
    """vfs_conv_plan / vfs_conv_wgrad_plan / vfs_stem_plan of the product library answer without a GPU, follow the options in force,
    and refuse a null out-pointer.  3 images of 14 x 14: 3 x 2 x 1 tiles of 8x16 pixels, ceil(588 / 128) = 5 linear blocks"""
    from vfs_amd.packing import conv_plan, stem_stats_rows, wgrad_halo_tiles
    lib = _lib.VfsLib(build.build_hip())
    geom = (3, 14, 14, 64, 128, 3, 1, 1)
    assert conv_plan(3, 1, 14, 14, 64, 128, 3, 1, 1, 14, 14, lib=lib) == (True, 6, False)
    assert conv_plan(3, 1, 14, 14, 64, 128, 3, 1, 1, 14, 14, dgrad=True, lib=lib) == (True, 3 * 1 * 1 * 2, False)      # dx has 64 channels: 16x16 tiles, two rows each
    assert conv_plan(3, 3, 14, 14, 64, 128, 3, 1, 1, 14, 14, lib=lib).rows == 2 and conv_plan(3, 2, 14, 14, 64, 128, 3, 1, 1, 14, 14, lib=lib).rows is None
    assert conv_plan(4, 2, 8, 8, 64, 128, 3, 1, 1, 8, 8, lib=lib) == (True, 1, True) and conv_plan(4, 4, 8, 8, 64, 128, 3, 1, 1, 8, 8, lib=lib).rows is None
    assert conv_plan(2, 1, 16, 16, 64, 128, 3, 2, 1, 8, 8, lib=lib) == (False, 1, False)
    assert conv_plan(2, 1, 16, 16, 64, 128, 3, 2, 1, 8, 8, dgrad=True, lib=lib) == (False, None, False)      # a strided dgrad writes no rows
    assert conv_plan(2, 1, 16, 16, 64, 128, 3, 1, 2, 16, 16, dil=2, lib=lib).halo is False
    assert wgrad_halo_tiles(*geom, lib=lib) == 6 and wgrad_halo_tiles(5, 8, 8, 64, 64, 3, 1, 1, lib=lib) == 3 and wgrad_halo_tiles(2, 16, 16, 64, 128, 3, 2, 1, lib=lib) == 0
    assert stem_stats_rows(4, 2, 64, 64, 32, 32, lib=lib) == 2 * 4 * 2
    for name, value, fwd, tiles, stem in ((b'halo', 0, (False, 5, False), 0, 16), (b'halo_min_fill', 100, (False, 5, False), 0, 16),
                                          (b'stem_direct', 0, (True, 6, False), 6, 2 * 32 * 32 // 128)):
        lib.set_option(name, value)
        try:
            assert conv_plan(3, 1, 14, 14, 64, 128, 3, 1, 1, 14, 14, lib=lib) == fwd, name
            assert wgrad_halo_tiles(*geom, lib=lib) == tiles, name
            assert stem_stats_rows(4, 2, 64, 64, 32, 32, lib=lib) == stem, name
        finally:
            lib.set_option(name, OPTION_DEFAULTS[name.decode()])
    out = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(_lib.VfsError, match='conv_plan: bad argument'):
        lib.conv_plan(0, 3, 14, 14, 64, 14, 14, 128, 3, 3, 1, 1, 1, 1, out, out[1:], None)
    with pytest.raises(_lib.VfsError, match='conv_wgrad_plan: bad argument'):
        lib.conv_wgrad_plan(3, 14, 14, 64, 14, 14, 128, 3, 3, 1, 1, None, out)
    with pytest.raises(_lib.VfsError, match='stem_plan: bad argument'):
        lib.stem_plan(4, 64, 64, 32, 32, 2, None)


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(_lib.VfsError):
        _lib.VfsLib(str(tmp_path / 'libvfs_hip.so'))


@pytest.mark.parametrize('depth', [18, 50])
def test_own_configs_build_with_reference_state_dict_names(depth, golden_dir):
    import numpy as np
    cfg = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', f'vfs_r{depth}.py'))
    model = vfs_amd.build_model(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    g = np.load(os.path.join(golden_dir, f'r{depth}_train.npz'))
    assert list(model.state_dict().keys()) == [str(k) for k in g['keys']]   # captured from the reference
    # init statistics of the reference model (kaiming fan_out convs, BN 1/0, zero-init residual)
    sd = model.state_dict()
    for k, v in sd.items():
        key = 'init/' + k
        if key in g.files and v.numel() > 1:
            m, s = float(v.float().mean()), float(v.float().std())
            rm, rs = g[key]
            if k.endswith('bn.weight') or k.endswith('bn.bias') or 'running' in k:
                assert abs(m - rm) < 1e-6 and abs(s - rs) < 1e-6, k
            elif k.endswith('conv.weight'):
                assert abs(s - rs) < 0.1 * rs + 1e-4, k      # same distribution, different RNG draw
    assert model.intra_video == (depth == 18)


@pytest.mark.skipif(not os.path.isdir(REF_CFG), reason='reference checkout not present')
@pytest.mark.parametrize('name', ['r18_nc_sgd_cos_100e_r2_1xNx8_k400.py', 'r50_nc_sgd_cos_100e_r5_1xNx2_k400.py',
                                  'r18_sgd_cos_100e_r2_1xNx8_k400.py', 'r50_sgd_cos_100e_r5_1xNx2_k400.py'])
def test_reference_configs_load_unchanged(name):
    cfg = vfs_amd.Config.fromfile(os.path.join(REF_CFG, name))
    model = vfs_amd.build_model(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    assert type(model).__name__ == 'SimSiamBaseTracker'
    own = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', 'vfs_r18.py' if name.startswith('r18') else 'vfs_r50.py'))
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items()}
    assert strip(cfg.model) == strip(own.model)
    assert dict(cfg.train_cfg) == dict(own.train_cfg) and dict(cfg.test_cfg) == dict(own.test_cfg)
    assert dict(cfg.optimizer) == dict(own.optimizer)
    # tools/test.py:129-133 rebuilds the model as a VanillaTracker with the test-time strides
    bb = dict(cfg.model['backbone'])
    bb['out_indices'], bb['strides'] = cfg.test_cfg.out_indices, cfg.test_cfg.strides
    vt = vfs_amd.build_model(dict(type='VanillaTracker', backbone=bb), train_cfg=None, test_cfg=cfg.test_cfg)
    assert vt.stride == 8


def test_resnet_constructor_errors_like_the_reference():
    """tests/test_models/test_backbone.py:24-49 of the reference."""
    with pytest.raises(KeyError):
        vfs_amd.ResNet(20)
    with pytest.raises(AssertionError):
        vfs_amd.ResNet(50, num_stages=0)
    with pytest.raises(AssertionError):
        vfs_amd.ResNet(50, num_stages=5)
    with pytest.raises(AssertionError):
        vfs_amd.ResNet(50, strides=(1,), dilations=(1, 1), num_stages=3)
    with pytest.raises(TypeError):
        net = vfs_amd.ResNet(50, pretrained=0)
        net.init_weights()
    net = vfs_amd.ResNet(18, norm_eval=True)
    net.init_weights()
    net.train()
    assert all(not m.training for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    net = vfs_amd.ResNet(50, frozen_stages=1)
    net.train()
    assert not net.conv1.bn.training and all(not p.requires_grad for p in net.layer1.parameters())
    with pytest.raises(KeyError):
        vfs_amd.build_model(dict(type='NoSuchTracker'))


def test_forward_train_asserts_like_the_reference():
    cfg = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', 'vfs_r18.py'))
    model = vfs_amd.build_model(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    with pytest.raises(AssertionError):
        model.forward_train(torch.zeros(2, 3, 3, 1, 32, 32))      # imgs.size(1) must be 2
    with pytest.raises(AssertionError):
        model.forward_train(torch.zeros(2, 2, 3, 32, 32))         # must be 6-D


def test_torchvision_checkpoint_key_mapping(tmp_path):
    """resnet.py:488-523 + tools/convert_weights/convert_to_pretrained.py naming."""
    net = vfs_amd.ResNet(18)
    tv = {}
    for name, m in net.conv_modules():
        cname, bname = (name + '.0', name + '.1') if 'downsample' in name else (name, name.replace('conv', 'bn'))
        tv[cname + '.weight'] = torch.randn_like(m.conv.weight)
        for k in ('weight', 'bias', 'running_mean', 'running_var'):
            tv[f'{bname}.{k}'] = torch.randn(m.bn.num_features)
    f = tmp_path / 'tv.pth'
    torch.save(dict(state_dict=tv), f)
    net2 = vfs_amd.ResNet(18, pretrained=str(f))
    net2.init_weights()
    assert torch.equal(net2.layer2[0].downsample.conv.weight, tv['layer2.0.downsample.0.weight'])
    assert torch.equal(net2.layer3[1].conv2.bn.running_var, tv['layer3.1.bn2.running_var'])
    assert torch.equal(net2.conv1.conv.weight, tv['conv1.weight'])


def test_command_tape_records_and_checks_return_codes():
    """_lib.Tape / TapeLib: calls are recorded with converted arguments, replayed in order, and a failing entry point
    raises both while recording and on replay (host logic only: vfs_set_option launches nothing)"""
    from vfs_amd._lib import Tape, TapeLib, VfsError, get_lib
    lib = get_lib()
    tape = Tape(lib)
    rec = TapeLib(lib, tape)
    seen = []
    rec.set_option(b'halo', 1)
    tape.ops.append((None, seen.append, ('py',)))          # a Python-side action between two C calls
    rec.set_option(b'bn_ticket', 1)
    assert [op[0] for op in tape.ops] == ['set_option', None, 'set_option'] and tape.ops[0][2] == (b'halo', 1)
    tape.replay()
    assert seen == ['py']
    with pytest.raises(VfsError):
        rec.set_option(b'no_such_option', 1)
    with pytest.raises(VfsError):
        tape.replay()                                       # the failing call was recorded too
    with pytest.raises(AttributeError):
        rec.no_such_entry_point


def test_no_compiler_generated_m0_use_in_lds_dma_kernels(tmp_path):
    """advisor r05: vfs_dma16_async_at (csrc/vfs_common.h) writes m0 from inline asm without saving it and declares the clobber,
    which clang warns it cannot honour for a reserved register.  That is safe exactly as long as the COMPILER keeps nothing of its own
    in m0 in those kernels (s_movrel / v_movrel / s_set_gpr_idx indexing, readlane-by-m0, LDS-direct, builtin LDS-DMA).  Build-time
    check: every source that issues LDS-DMA pieces is compiled to gfx950 assembly and each line that mentions m0 must be one of
    ours - `s_mov_b32 m0, <lds address>` in front of a `buffer_load_dword* ... lds`, or the save / restore pair of
    vfs_dma16_async."""
    import re
    import subprocess
    from concurrent.futures import ThreadPoolExecutor
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    srcs = [s for s in build._sources() if re.search(r'vfs_dma16_async', open(s).read())]
    assert len(srcs) >= 4

    def asm(src):
        out = tmp_path / (os.path.basename(src) + '.s')
        subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-w', '-o', str(out), src])
        return src, out.read_text().splitlines()

    with ThreadPoolExecutor(4) as ex:
        for src, lines in ex.map(asm, srcs):
            code = [ln.split(';')[0].strip() for ln in lines]
            code = [c for c in code if c and not c.startswith('.') and not c.endswith(':')]      # instructions only
            mine = 0
            for i, c in enumerate(code):
                if not re.search(r'\bm0\b', c):
                    continue
                nxt, prv = code[i + 1:i + 3], code[max(0, i - 1):i]
                setup = re.match(r's_mov_b32 m0, \S+$', c) and len(nxt) == 2 and nxt[0].startswith('s_nop') and \
                    re.match(r'buffer_load_dword\S* .* lds$', nxt[1])                                          # ours: m0 <- LDS address, s_nop, the DMA piece
                save = re.match(r's_mov_b32 \S+, m0$', c) and nxt and re.match(r's_mov_b32 m0, \S+$', nxt[0])      # vfs_dma16_async: save ...
                restore = re.match(r's_mov_b32 m0, \S+$', c) and prv and re.match(r'buffer_load_dword\S* .* lds$', prv[0])      # ... and restore
                step = re.match(r's_add_u32 m0, m0, 0x[0-9a-f]+$', c) and len(nxt) == 2 and nxt[0].startswith('s_nop') and \
                    re.match(r'buffer_load_dword\S* .* lds$', nxt[1])      # labelprop2.hip: eight pieces of one stage, m0 stepped in place
                assert setup or save or restore or step, f'{os.path.basename(src)}: compiler-generated m0 use: {code[max(0, i - 2):i + 3]}'
                mine += 1
            assert mine > 0, f'{os.path.basename(src)}: no LDS-DMA m0 set-up found (the check looks at the wrong thing)'


# The A/B switchboard of include/vfs_hip_tuning.h as the engine, the tools and the tests use it: every name, with its default.
OPTION_DEFAULTS = dict(
    halo=1, halo_min_fill=70, halo_deep_max=256, halo_xcd=1, stem_direct=1, stem_blocks=0,
    bn_ticket=1, bn_chunk_rows=64, bn_wide=1, bn_wide_min_mb=8,
    igemm_bc=0, igemm_xcd=1, igemm_mfma_stats=1, igemm_narrow_below=513, igemm_onek=3, igemm_ring_tiles=512, igemm_ring_fbn=1,
    igemm_ring_mfma32=1, igemm_ring_gather=0, igemm_ring_upfront=0, igemm_ds_quarter=1, igemm_skinny=1, igemm_pw=0, igemm_pw_min_tiles=192,
    wgrad_lin=1, wgrad_lin2=1, wgrad_ring=1, wgrad_xcd=1,
    lpx_target=0, lpx_wgs=0, lpx_minb=4, lp2=1, lp2_fpb=0, lp2_trim=1, lp2_xcd=-1, lp2_dbg=0, lp2_cap=0,
    conv_f32_variant=0, conv_f32_dbg=0)


def test_option_switchboard_names_defaults_and_setters():
    """vfs_set_option: each of the 39 names is accepted and writes the global `vfs_option_<name>` (set to its default here, so
    nothing leaks into other tests), the two normalising setters keep their rules, an unknown name is an argument error"""
    import ctypes
    from tests.emu_util import emu_lib
    lib = emu_lib()
    assert len(OPTION_DEFAULTS) == 39
    var = lambda name: ctypes.c_int.in_dll(lib.dll, 'vfs_option_' + name).value
    for name, default in OPTION_DEFAULTS.items():
        lib.set_option(name.encode(), default)
        assert var(name) == default, name
    for given, stored in ((0, 64), (-3, 64), (32, 32), (64, 64)):
        lib.set_option(b'bn_chunk_rows', given)
        assert var('bn_chunk_rows') == stored
    for given, stored in ((-5, 0), (5, 16), (16, 16), (200, 200), (0, 0)):
        lib.set_option(b'lp2_cap', given)
        assert var('lp2_cap') == stored
    assert lib.cfunc('set_option')(b'no_such_option', 1) == -3
    assert lib.last_error() == 'vfs_set_option: unknown option'
    with pytest.raises(_lib.VfsError, match='unknown option'):
        lib.set_option(b'', 1)
    assert {n: var(n) for n in OPTION_DEFAULTS} == OPTION_DEFAULTS


SHAPE, ARG = -1, -3


def _argument_error_cases():
    """(id, entry point, arguments, code, message): argument checks of the entry points whose descriptors capi.hip builds with shared
    helpers.  Every case returns before a launch; P stands for any non-null buffer."""
    P = torch.zeros(16384)
    cases = []

    def case(cid, name, args, code, msg):
        cases.append(pytest.param(name, args, code, msg, id=cid))

    # ---- label propagation: (.., workspace, workspace_bytes, qframe, kslot, nkeys, H, W, C, CO, radius, non_mask_len, topk, temperature)
    dense = 96 * 2 * 2 * 10 * 8                                      # vfs_labelprop_workspace_bytes(2, 2)
    two_pass = dense + 16 * 2 * 2 * 8 + (25 * 2 * 2 * 4 + 15) // 16 * 16 + 16      # ..._2pass_workspace_bytes_for(2, 2, 16)
    for who, head, tail, need in (('labelprop', (P, P, P), (), dense), ('labelprop_f32', (P, P, P), (), dense),
                                  ('labelprop_f32_2pass', (P, P, P, P), (1,), two_pass)):
        def lp(ws, nbytes, nkeys, radius, non_mask_len, head=head, tail=tail):
            return head + (ws, nbytes, 3, P, nkeys, 2, 2, 256, 4, radius, non_mask_len, 10, 0.05) + tail + (None,)
        case(f'{who}-nkeys0', who, lp(P, need, 0, 3, 0), SHAPE, f'{who}: 1 <= nkeys <= 64')
        case(f'{who}-nkeys65', who, lp(P, need, 65, 3, 0), SHAPE, f'{who}: 1 <= nkeys <= 64')
        short = f'{who}: workspace smaller than ' + ('vfs_labelprop_f32_2pass_workspace_bytes_for(H, W, 16)' if tail else
                                                     'vfs_labelprop_workspace_bytes(H, W)')
        case(f'{who}-short-workspace', who, lp(P, need - 1, 2, 3, 0), ARG, short)
        case(f'{who}-null-workspace', who, lp(None, need, 2, 3, 0), ARG, short)
        case(f'{who}-non_mask_len', who, lp(P, need, 2, 3, 2), ARG, f'{who}: 0 <= non_mask_len < nkeys')
        case(f'{who}-non_mask_len-negative', who, lp(P, need, 2, 3, -1), ARG, f'{who}: 0 <= non_mask_len < nkeys')
        case(f'{who}-non_mask_len-no-mask', who, lp(P, need, 2, 0, 3), ARG, f'{who}: 0 <= non_mask_len < nkeys')     # radius <= 0: nkeys itself is allowed
    # the two-pass entry checks the key count and non_mask_len BEFORE its workspace; without the split bank it is vfs_labelprop_f32
    case('labelprop_f32_2pass-order', 'labelprop_f32_2pass', (P, P, P, P, None, 0, 3, P, 65, 2, 2, 256, 4, 3, 0, 10, 0.05, 1, None), SHAPE,
         'labelprop_f32_2pass: 1 <= nkeys <= 64')
    case('labelprop_f32_2pass-order2', 'labelprop_f32_2pass', (P, P, P, P, None, 0, 3, P, 2, 2, 2, 256, 4, 3, 2, 10, 0.05, 1, None), ARG,
         'labelprop_f32_2pass: 0 <= non_mask_len < nkeys')
    case('labelprop_f32_2pass-dense-fallback', 'labelprop_f32_2pass', (P, None, P, P, P, dense - 1, 3, P, 2, 2, 2, 256, 4, 3, 0, 10, 0.05, 1, None),
         ARG, 'labelprop_f32: workspace smaller than vfs_labelprop_workspace_bytes(H, W)')

    # ---- BatchNorm apply passes with in-kernel statistics
    def act_fin(M, mpg, partial=P):       # (x, partial, bpg, gamma, beta, bnp, sums, rm, rv, res, rres, rbnp, y, mask, M, C, mpg, relu, count, eps, momentum)
        return (P, partial, 1, P, P, P, P, P, P, None, None, None, P, None, M, 64, mpg, 1, 128.0, 1e-5, 0.1)

    def bwd_fin(M, mpg, partial=P):       # (g, y, x, bnp, partial, bpg, sums, dgamma, dbeta, dx, gm, M, C, mpg, count, relu)
        return (P, P, P, P, partial, 1, P, P, P, P, None, M, 64, mpg, 128.0, 1)

    def xchg(peers=P, state=P, seq=0):    # (peers, rank, world, state, spin_limit, seq)
        return (peers, 0, 2, state, 1000, seq)
    for who, msg, base in (('bn_act_fin_mask', 'bn_act_fin', act_fin), ('bn_bwd_apply_fin', 'bn_bwd_apply_fin', bwd_fin)):
        case(f'{who}-M%mpg', who, base(130, 128) + (None,), SHAPE, f'{msg}: M % mpg')
        case(f'{who}-mpg0', who, base(128, 0) + (None,), SHAPE, f'{msg}: M % mpg')
    case('bn_act_fin-M%mpg', 'bn_act_fin', act_fin(130, 128)[:13] + act_fin(130, 128)[14:] + (None,), SHAPE, 'bn_act_fin: M % mpg')
    for who, base in (('bn_act_fin_xchg', act_fin), ('bn_bwd_apply_fin_xchg', bwd_fin)):
        case(f'{who}-M%mpg', who, base(130, 128) + xchg(seq=-1) + (None,), SHAPE, f'{who}: M % mpg')      # checked before seq
        case(f'{who}-mpg0', who, base(128, 0) + xchg() + (None,), SHAPE, f'{who}: M % mpg')
        case(f'{who}-seq-1', who, base(128, 128) + xchg(peers=None, seq=-1) + (None,), ARG, f'{who}: 0 <= seq < 4095')      # before the null checks
        case(f'{who}-seq4095', who, base(128, 128) + xchg(seq=4095) + (None,), ARG, f'{who}: 0 <= seq < 4095')
        given = f'{who}: statistics rows, peers and state must be given'
        case(f'{who}-null-peers', who, base(128, 128) + xchg(peers=None, seq=4094) + (None,), ARG, given)
        case(f'{who}-null-state', who, base(128, 128) + xchg(state=None) + (None,), ARG, given)
        case(f'{who}-null-rows', who, base(128, 128, partial=None) + xchg() + (None,), ARG, given)

    def bwd_raw(M, mpg):                  # (g, y, x, bnp, sums, dgamma, dbeta, dx, gm, M, C, mpg, count, relu)
        return (P, P, P, P, P, P, P, P, None, M, 64, mpg, 128.0, 1, None)
    one_row = 'bn_bwd_apply_raw: one statistics row per group (mpg <= 512 and gcd(mpg, 512) == mpg or < 16)'
    case('bn_bwd_apply_raw-M%mpg', 'bn_bwd_apply_raw', bwd_raw(130, 128), SHAPE, 'bn_bwd_apply_raw: M % mpg')
    case('bn_bwd_apply_raw-mpg1024', 'bn_bwd_apply_raw', bwd_raw(2048, 1024), SHAPE, one_row)
    case('bn_bwd_apply_raw-mpg48', 'bn_bwd_apply_raw', bwd_raw(96, 48), SHAPE, one_row)      # gcd(48, 512) = 16
    case('bn_bwd_reduce-ppb', 'bn_bwd_reduce', (P, P, P, P, P, 256, 64, 128, 48, 1, None), SHAPE,
         'bn_bwd_reduce: pixels-per-group % pixels-per-block')

    # ---- convolutions: (.., N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad)
    g3 = (2, 16, 16, 64, 16, 16, 64, 3, 3, 1, 1)
    g1 = (2, 16, 16, 64, 16, 16, 64, 1, 1, 1, 0)
    s2 = (2, 16, 16, 64, 8, 8, 64, 3, 3, 2, 1)
    add_mask = 'conv_dgrad: add_mask needs an add operand and Cin % 64 == 0'
    case('conv_dgrad_maskadd-no-add', 'conv_dgrad_maskadd', (P, P, P, None, P) + g3 + (None,), SHAPE, add_mask)
    case('conv_dgrad_maskadd-Cin32', 'conv_dgrad_maskadd', (P, P, P, P, P) + (2, 16, 16, 32, 16, 16, 64, 3, 3, 1, 1, None), SHAPE, add_mask)
    bn = (P, P, P, P, 256, 1)             # (bn_x, bn_y, bnp, bn_partial, bn_mpg, bn_relu)
    case('conv_dgrad_bn-stride2', 'conv_dgrad_bn', (P, P, P, None) + bn + s2 + (None,), SHAPE,
         'conv_dgrad_bn: stride 1 only (strided dgrads run per parity class)')
    case('conv_dgrad_bn_maskadd-stride2', 'conv_dgrad_bn_maskadd', (P, P, P, None, P) + bn + s2 + (None,), SHAPE,      # before the mask check
         'conv_dgrad_bn: stride 1 only (strided dgrads run per parity class)')
    case('conv_dgrad_bn-null-stats', 'conv_dgrad_bn', (P, P, P, None, None, P, P, P, 256, 1) + g3 + (None,), ARG, 'conv_dgrad_bn: null statistics operand')
    case('conv_dgrad_bn-mpg0', 'conv_dgrad_bn', (P, P, P, None, P, P, P, P, 0, 1) + g3 + (None,), ARG, 'conv_dgrad_bn: null statistics operand')
    case('conv_dgrad_bn_maskadd-no-add', 'conv_dgrad_bn_maskadd', (P, P, P, None, P) + bn + g3 + (None,), SHAPE, add_mask)
    groups = 'conv_dgrad_bn: groups must be whole images (tile kernels) / multiples of 128 pixels'
    case('conv_dgrad_bn-groups-tiles', 'conv_dgrad_bn', (P, P, P, None, P, P, P, P, 128, 1) + g3 + (None,), SHAPE, groups)     # 16 x 16 images
    case('conv_dgrad_bn-groups-linear', 'conv_dgrad_bn', (P, P, P, None, P, P, P, P, 64, 1) + g1 + (None,), SHAPE, groups)
    bnin = 'the 3x3/stride-1 halo-tile kernel and the 1x1/stride-1 kernel fold the input BatchNorm'
    case('conv_fwd_bnin-null', 'conv_fwd_bnin', (P, None, 1, P, P, None, P) + g3 + (None,), ARG, 'conv_fwd_bnin: BatchNorm parameters of the input')
    case('conv_fwd_bnin-npg0', 'conv_fwd_bnin', (P, P, 0, P, P, None, P) + g3 + (None,), ARG, 'conv_fwd_bnin: BatchNorm parameters of the input')
    case('conv_fwd_bnin-stride2', 'conv_fwd_bnin', (P, P, 1, P, P, None, P) + s2 + (None,), SHAPE, 'conv_fwd_bnin: ' + bnin)
    case('conv_wgrad_bnin-null', 'conv_wgrad_bnin', (P, P, None, 1, P, P) + g3 + (1, 512, None), ARG, 'conv_wgrad_bnin: BatchNorm parameters of the input')
    case('conv_wgrad_bnin-npg0', 'conv_wgrad_bnin', (P, P, P, 0, P, P) + g3 + (1, 512, None), ARG, 'conv_wgrad_bnin: BatchNorm parameters of the input')
    case('conv_wgrad_bnin-stride2', 'conv_wgrad_bnin', (P, P, P, 1, P, P) + s2 + (1, 128, None), SHAPE, 'conv_wgrad_bnin: ' + bnin)
    case('conv_wgrad_inl-null', 'conv_wgrad_inl', (P, P, None, 0, P, None, P) + g3 + (1, 512, None), ARG,
         'conv_wgrad_inl: partial, grad and tickets must be given')
    case('conv_wgrad_inl-npg0', 'conv_wgrad_inl', (P, P, P, 0, P, P, P) + g3 + (1, 512, None), ARG,
         'conv_wgrad_inl: images per BatchNorm group of the input')
    case('conv_wgrad_inl-bnin-stride2', 'conv_wgrad_inl', (P, P, P, 1, P, P, P) + s2 + (1, 128, None), SHAPE,
         'conv_wgrad_inl: only the 3x3/stride-1 halo-tile kernel folds the input BatchNorm')
    case('conv_fwd_splitk-no-workspace', 'conv_fwd_splitk', (P, P, P, None, None, None, 2) + g1 + (None,), ARG, 'conv_fwd_splitk: workspace')
    case('conv_fwd_splitk-ksplit0', 'conv_fwd_splitk', (P, P, P, None, None, P, 0) + g1 + (None,), ARG, 'conv_fwd_splitk: workspace')
    case('conv_dgrad_splitk-no-workspace', 'conv_dgrad_splitk', (P, P, P, None, None, 2) + s2 + (None,), ARG, 'conv_dgrad_splitk: workspace')
    case('conv_dgrad_splitk-stride2', 'conv_dgrad_splitk', (P, P, P, None, P, 2) + s2 + (None,), SHAPE, 'conv_dgrad_splitk: stride 1 only')
    case('conv_fwd_coarse-null', 'conv_fwd_coarse', (P, P, P, None, P, None, P, 2) + g3 + (None,), ARG,
         'conv_fwd_coarse: stats, stats_coarse, tickets and 1 <= coarse_log2 <= 8')
    case('conv_fwd_coarse-log2', 'conv_fwd_coarse', (P, P, P, None, P, P, P, 9) + g3 + (None,), ARG,
         'conv_fwd_coarse: stats, stats_coarse, tickets and 1 <= coarse_log2 <= 8')
    case('conv_fwd_dilated-dilation0', 'conv_fwd_dilated', (P, P, P, None, None) + g3 + (0, None), ARG, 'conv_fwd_dilated: dilation >= 1')
    case('conv_fwd_dilated-size', 'conv_fwd_dilated', (P, P, P, None, None) + g3 + (2, None), SHAPE,
         'conv_fwd_dilated: output size does not match (H + 2 pad - dilation (K - 1) - 1) / stride + 1')
    case('stem_fwd-odd-width', 'stem_fwd', (P, P, P, None, 1, 32, 33, 16, 16, None), SHAPE, 'stem_fwd: padded width must be even')
    # ---- plan queries: (dgrad, geometry, dilation, G, halo, rows, pairs) / (N, H, Wp, Ho, Wo, G, rows) / (geometry, halo, ntiles)
    for i in range(3):
        outs = tuple(None if j == i else P for j in range(3))
        case(f'conv_plan-null-out{i}', 'conv_plan', (0,) + g3 + (1, 1) + outs, ARG, 'conv_plan: bad argument')
    case('conv_plan-G0', 'conv_plan', (0,) + g3 + (1, 0, P, P, P), ARG, 'conv_plan: bad argument')
    case('conv_plan-dilation0', 'conv_plan', (0,) + g3 + (0, 1, P, P, P), ARG, 'conv_plan: bad argument')
    case('stem_plan-null-out', 'stem_plan', (2, 32, 32, 16, 16, 1, None), ARG, 'stem_plan: bad argument')
    case('stem_plan-G0', 'stem_plan', (2, 32, 32, 16, 16, 0, P), ARG, 'stem_plan: bad argument')
    case('conv_wgrad_plan-null-halo', 'conv_wgrad_plan', g3 + (None, P), ARG, 'conv_wgrad_plan: bad argument')
    case('conv_wgrad_plan-null-ntiles', 'conv_wgrad_plan', g3 + (P, None), ARG, 'conv_wgrad_plan: bad argument')

    # ---- input pipeline: (.., imgs, x4, B, V, T, Hs, Ws, Ho, Wo, Wp, mean x 3, std x 3)
    norm = (123.675, 116.28, 103.53, 58.395, 57.12, 57.375, None)
    for who, head in (('crop_resize_flip_norm', (P, P)), ('crop_resize_flip_photo_norm', (P, P, P, P, 1 << 20))):
        case(f'{who}-null-src', who, (None,) + head + (P, P, 1, 2, 1, 8, 8, 4, 4, 4) + norm, ARG, f'{who}: null buffer')
        case(f'{who}-no-output', who, (P,) + head + (None, None, 1, 2, 1, 8, 8, 4, 4, 4) + norm, ARG, f'{who}: null buffer')
        case(f'{who}-Wp', who, (P,) + head + (None, P, 1, 2, 1, 8, 8, 4, 4, 3) + norm, SHAPE, f'{who}: Wp < Wo')
    photo = 'crop_resize_flip_photo_norm'
    case(f'{photo}-null-photo', photo, (P, P, P, None, P, 1 << 20, P, P, 1, 2, 1, 8, 8, 4, 4, 4) + norm, ARG, f'{photo}: null buffer')
    case(f'{photo}-empty', photo, (P, P, P, P, P, 1 << 20, P, P, 0, 2, 1, 8, 8, 4, 4, 4) + norm, SHAPE, f'{photo}: empty batch')
    case(f'{photo}-workspace', photo, (P, P, P, P, P, 8, P, P, 1, 2, 1, 8, 8, 4, 4, 4) + norm, ARG,
         f'{photo}: workspace smaller than vfs_crop_resize_flip_photo_norm_workspace_bytes')
    case(f'{photo}-null-workspace', photo, (P, P, P, P, None, 1 << 20, P, P, 1, 2, 1, 8, 8, 4, 4, 4) + norm, ARG,
         f'{photo}: workspace smaller than vfs_crop_resize_flip_photo_norm_workspace_bytes')
    return cases


@pytest.mark.parametrize('name,args,code,message', _argument_error_cases())
def test_argument_errors_keep_their_code_and_message(name, args, code, message):
    """the argument checks of the convolution, BatchNorm, label propagation and pipeline entry points: return code and
    vfs_last_error() text, word for word (callers and tests match on both); each returns before anything is launched"""
    from tests.emu_util import emu_lib
    lib = emu_lib()
    fn = lib.cfunc(name)
    assert len(args) == len(lib.protos['vfs_' + name][1]), 'the case does not match the prototype'
    rc = fn(*[a.data_ptr() if hasattr(a, 'data_ptr') else a for a in args])
    assert (rc, lib.last_error()) == (code, message)
