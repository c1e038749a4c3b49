"""The two-pass label propagation at C = 64 and C = 128 (csrc/labelprop2.hip lp2_score_narrow_body: ResNet-18 stages 0 and 1) == the
dense fp32 kernel on the same operands, uint32 views compared for equality.

Smallest shapes at which the narrow pass 1 can go wrong: an 8 x 12 map (two query tiles, key blocks of 64 with a ragged last one) and
9 x 13 (ragged tiles on both axes), 3 classes, topk 10; three key frames, and one key frame under radius 2 (nine in-mask keys at most:
every query sees fewer than ten); no mask and radius 3; non_mask_len 0 and 1; the single-video and the batched entry point;
candidates packed inside the prefilter's margin; the split banks of both producers."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_labelprop2 import _features, _unit_bank, _ws, same_bits
from tests.test_labelprop_batch import Batch, _desc_rows

WIDTHS = [64, 128]
MAPS = [(8, 12), (9, 13)]
CO, TOPK, TEMP = 3, 10, 0.07


def _margin(C):
    """csrc/labelprop2.hip lp2_margin"""
    return 2.0 * (3.0 / 65536.0 + 4.0 * C / 16777216.0) + 1.0 / 2097152.0


def _both(lib, fb, hl, seg, H, W, C, radius, slots, qframe, nml):
    """-> (two-pass, dense, overflow flag of the two-pass call) on the same operands.  Pass 1 must have RUN: it leaves the list lengths
    of every query behind the list area of the workspace (zero-filled here), which the dense kernels never touch"""
    HW = H * W
    ks = (ctypes.c_int * len(slots))(*slots)
    out, dense = torch.full((HW, CO), float('nan')), torch.full((HW, CO), float('nan'))
    ws, dense_bytes = _ws(lib, H, W)
    lib.labelprop_f32_2pass(fb, hl, seg, out, ws, ws.numel() * 4, qframe, ks, len(slots), H, W, C, CO, radius, nml, TOPK, TEMP, 1, None)
    n = torch.zeros(1, dtype=torch.int64)
    lib.labelprop_f32_2pass_workspace_bytes(H, W, n)
    flag = int(ws.view(torch.int32)[(int(n.item()) - 16) // 4])
    off = (dense_bytes + 24 * HW * 192 * 8) // 4      # LP2_MAX_SPLIT x LP2_MAX_CAP entries of 8 bytes per query, then the counts
    counts = ws.view(torch.int32)[off:off + 24 * HW].reshape(24, HW).sum(0)
    assert int(counts.min()) >= 1, 'the two-pass kernels did not run (no candidate lists)'
    ws2 = torch.zeros_like(ws)
    lib.labelprop_f32(fb, seg, dense, ws2, ws2.numel() * 4, qframe, ks, len(slots), H, W, C, CO, radius, nml, TOPK, TEMP, None)
    return out.numpy(), dense.numpy(), flag


def _assert_same_bits(got, want):
    assert not np.isnan(want).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.nanmax(np.abs(got - want)))


@pytest.mark.parametrize('nml', [0, 1])
@pytest.mark.parametrize('radius', [0, 3])
@pytest.mark.parametrize('H,W', MAPS)
@pytest.mark.parametrize('C', WIDTHS)
def test_narrow_two_pass_equals_dense(backend, C, H, W, radius, nml):
    """three key frames, the first one twice (exact ties between its two copies)"""
    lib = backend.hostlib
    feats, seg = _features(3, H, W, C, CO, seed=7 + C)
    fb, hl = _unit_bank(lib, feats)
    got, want, flag = _both(lib, fb, hl, seg, H, W, C, radius, [0, 0, 1], 2, nml)
    _assert_same_bits(got, want)
    assert flag == 0      # the lists held everything: the two-pass kernels produced these bits


@pytest.mark.parametrize('H,W', MAPS)
@pytest.mark.parametrize('C', WIDTHS)
def test_narrow_two_pass_fewer_candidates_than_topk(backend, C, H, W):
    """one key frame under radius 2: nine in-mask keys at most, four in a corner"""
    lib = backend.hostlib
    feats, seg = _features(2, H, W, C, CO, seed=9 + C)
    fb, hl = _unit_bank(lib, feats)
    got, want, flag = _both(lib, fb, hl, seg, H, W, C, 2, [0], 1, 0)
    _assert_same_bits(got, want)
    assert flag == 0


@pytest.mark.parametrize('C', WIDTHS)
def test_narrow_two_pass_near_ties_inside_the_margin(backend, C):
    """every key row is the common row plus a few fp32 ulps, some exact duplicates: the 10th and 11th exact scores of every query
    differ by far less than the prefilter's margin, the split-bf16 scores mostly not at all - the ten survivors and their order
    (score desc, id asc) must be the dense kernel's"""
    lib = backend.hostlib
    T, H, W = 3, 8, 12
    g = torch.Generator().manual_seed(11 + C)
    base = torch.randn(C, generator=g)
    feats = base[None, None, :].repeat(T, H * W, 1)
    feats = feats * (1.0 + torch.randint(-3, 4, feats.shape, generator=g).float() * 2.0 ** -21)
    feats[1, 5] = feats[1, 4]
    feats[0, 17] = feats[1, 17]
    seg = torch.rand(T, H * W, CO, generator=g)
    fb, hl = _unit_bank(lib, feats)
    q = 3 * W + 5      # an inner query: 2 x 25 in-mask keys under radius 3
    keys = np.array([[f, (3 + dy) * W + 5 + dx] for f in (0, 1) for dy in range(-2, 3) for dx in range(-2, 3) if dy * dy + dx * dx < 9])
    exact = np.sort((fb[keys[:, 0], keys[:, 1]].double() @ fb[2, q].double()).numpy())[::-1]
    assert len(exact) > 11 and 0 <= exact[9] - exact[10] < _margin(C) and exact[0] - exact[-1] < _margin(C)
    got, want, flag = _both(lib, fb, hl, seg, H, W, C, 3, [0, 1], 2, 0)
    _assert_same_bits(got, want)
    assert flag == 0
    assert len(np.unique(want.view(np.uint32))) > 10      # (the label rows differ from query to query: the survivors matter)


@pytest.mark.parametrize('nml', [0, 1])
@pytest.mark.parametrize('C', WIDTHS)
def test_narrow_batched_two_pass_equals_dense(backend, C, nml):
    """two slots at different frames with different class counts (and an idle one between them), 9 x 13, radius 3"""
    lib = backend.hostlib
    H, W = 9, 13
    b = Batch(lib, 3, 4, H, W, C, 3, True)
    b.put(0, *_features(4, H, W, C, 3, seed=20 + C))
    b.put(2, *_features(3, H, W, C, 2, seed=21 + C))
    plan = {0: (3, [0, 1, 2]), 2: (2, [0, 0, 1])}
    rows = {n: (q, keys, nml, b.videos[n][1]) for n, (q, keys) in plan.items()}
    for n, (q, keys, _, _) in rows.items():
        b.rows(n, q).fill_(float('nan'))
    nb = torch.zeros(1, dtype=torch.int64)
    lib.labelprop_f32_2pass_batch_workspace_bytes(H, W, 0, 3, nb)
    ws = torch.zeros((int(nb.item()) + 3) // 4)
    lib.labelprop_f32_2pass_batch(b.fb, b.hl, b.sb, ws, ws.numel() * 4, _desc_rows(3, rows), 3, 2, 3, 4, H, W, C, 3, 3, TOPK, TEMP, 1, None)
    assert ws.view(torch.int32)[:3].tolist() == [0, 0, 0]      # no slot overflowed: the two-pass kernels produced these bits
    for n, (q, keys, _, _) in rows.items():
        dense, _, _ = b.single(n, q, keys, 3, TOPK, nml, dense=True)
        single, _, flag = b.single(n, q, keys, 3, TOPK, nml, dense=False)
        assert flag == 0
        _assert_same_bits(b.rows(n, q).numpy(), dense.numpy())
        _assert_same_bits(single.numpy(), dense.numpy())
    assert torch.isnan(b.sb[1]).all()


@pytest.mark.parametrize('C', WIDTHS)
def test_narrow_split_banks_of_both_producers(backend, C):
    """split_rows_bf16x2 and the table-driven ingest write the same unit rows and the same hi / lo split: hi = bf16(x), lo = bf16(x -
    hi), 16 channels of hi then 16 of lo per group"""
    lib = backend.hostlib
    n, HW = 3, 20
    feats, _ = _features(n, 4, 5, C, CO, seed=30 + C)
    fb, hl = _unit_bank(lib, feats)
    hi = fb.to(torch.bfloat16)
    lo = (fb - hi.float()).to(torch.bfloat16)
    want = torch.stack([hi.reshape(n, HW, C // 16, 16), lo.reshape(n, HW, C // 16, 16)], dim=3).reshape(n, HW, 2 * C)
    assert torch.equal(hl.view(torch.int16), want.view(torch.int16))
    bank = torch.zeros(4 * HW, C)
    hl2 = torch.zeros(4 * HW, 2 * C, dtype=torch.bfloat16)
    table = (torch.tensor([3, 0, 2], dtype=torch.int64) * HW)[:, None].repeat(1, 2)      # image i enters position table[i]
    lib.bank_ingest_f32(feats.contiguous(), bank, hl2, table, n, HW, C, 4 * HW, 1, None)
    for i, pos in enumerate((3, 0, 2)):
        assert same_bits(bank[pos * HW:(pos + 1) * HW].numpy(), fb[i].numpy())
        assert torch.equal(hl2[pos * HW:(pos + 1) * HW].view(torch.int16), hl[i].view(torch.int16))


def test_two_pass_ok_names_the_widths(monkeypatch):
    from vfs_amd.labelprop import LP2_NARROW_DEFAULT, two_pass_ok
    assert [two_pass_ok('fp32', True, C, True) for C in (64, 128, 256, 512, 1024, 2048)] == [True] * 5 + [False]
    assert [two_pass_ok('fp32', True, C, False) for C in (64, 128, 256, 2048)] == [False, False, True, False]
    assert two_pass_ok('fp32', True, 64) == LP2_NARROW_DEFAULT
    assert not two_pass_ok('bf16', True, 64, True) and not two_pass_ok('fp32', False, 128, True)
    monkeypatch.setenv('VFS_LP_TWO_PASS', '0')
    assert not two_pass_ok('fp32', True, 64, True)
