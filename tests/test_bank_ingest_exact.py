"""Table-driven ingest of a feature bank (csrc/bank_ingest.hip: vfs_bank_ingest_f32 / vfs_bank_ingest_bf16) against the contiguous
kernels it stands in for, BIT FOR BIT: vfs_l2norm_rows_f32 + vfs_split_rows_bf16x2 (fp32 banks with their hi / lo split copy) and
vfs_l2norm_rows (bf16 banks).  All of them call the row arithmetic of csrc/vfs_rows.h, so what is at stake is the ingest's own part:
the image index on the grid, the destination rows of the table (permuted, with gaps between the images), a row held in registers
between its read and its writes, the exchange between neighbouring lanes in front of the split, the last partial workgroup (four rows
per workgroup: P = 23), and that nothing but the destination rows is written.

Shapes: n = 3 images; P = 24 and 23 rows; C = 64 and 256 with the split (one float4 group per lane, 16 and 64 lanes of a wave busy),
C = 512 with it (two groups per lane), C = 320 without it (a second, partly filled group), C = 64 in bf16.  The first row of image 0
is zero (the eps branch of the norm)."""
import pytest
import torch

SHAPE, ARG = -1, -3      # include/vfs_hip.h VFS_ERR_SHAPE, VFS_ERR_ARG
SENTINEL = -7.25         # exactly representable in bf16


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _feats(n, P, C, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, P, C, generator=g) * torch.logspace(-3, 3, P)[None, :, None]      # rows of very different lengths
    x[0, 0] = 0.0
    return x.to(dtype)


def _layout(n, P):
    """destination rows of the images in the bank and in its split copy: permuted, gaps between and around them -> (table, rows)"""
    rows = 4 * P + 9
    frow = [3 * P + 5, 0, P + 2][:n]
    hrow = [P + 1, 3 * P + 3, 0][:n]
    return torch.tensor(list(zip(frow, hrow)), dtype=torch.int64), rows


def _expect(bank, table, col, want, P):
    """`bank` holds image i of `want` at rows table[i][col] .. + P and the sentinel everywhere else"""
    ref = torch.full_like(bank, SENTINEL)
    for i in range(want.shape[0]):
        r = int(table[i, col])
        ref[r:r + P] = want[i]
    assert torch.equal(bits(bank), bits(ref)), [int((bits(bank[int(table[i, col]):int(table[i, col]) + P]) != bits(want[i])).sum()) for i in range(want.shape[0])]


@pytest.mark.parametrize('P', [24, 23])
@pytest.mark.parametrize('C,split', [(64, True), (256, True), (512, True), (320, False)])
def test_ingest_f32_equals_l2norm_and_split(backend, P, C, split):
    lib = backend.hostlib
    n = 3
    x = _feats(n, P, C, seed=C + P)
    table, rows = _layout(n, P)
    unit = torch.zeros(n, P, C)
    lib.l2norm_rows_f32(x.reshape(-1, C), unit, n * P, C, None)
    assert torch.isfinite(unit).all() and float(unit[0, 0].abs().max()) == 0.0 and abs(float(unit[1, 3].norm()) - 1.0) < 1e-5
    fbank = torch.full((rows, C), SENTINEL)
    hlbank = torch.full((rows, 2 * C), SENTINEL, dtype=torch.bfloat16) if split else None
    lib.bank_ingest_f32(x, fbank, hlbank, table, n, P, C, rows, 1, None)
    _expect(fbank, table, 0, unit, P)
    if split:
        hl = torch.zeros(n, P, 2 * C, dtype=torch.bfloat16)
        lib.split_rows_bf16x2(unit.reshape(-1, C), hl, n * P, C, None)
        assert float(hl.float().abs().max()) > 0.0
        _expect(hlbank, table, 1, hl, P)


@pytest.mark.parametrize('P', [24, 23])
def test_ingest_bf16_equals_l2norm(backend, P):
    lib = backend.hostlib
    n, C = 3, 64
    x = _feats(n, P, C, seed=7 + P, dtype=torch.bfloat16)
    table, rows = _layout(n, P)
    unit = torch.zeros(n, P, C, dtype=torch.bfloat16)
    lib.l2norm_rows(x.reshape(-1, C), unit, n * P, C, None)
    assert abs(float(unit[1, 3].float().norm()) - 1.0) < 2e-2
    fbank = torch.full((rows, C), SENTINEL, dtype=torch.bfloat16)
    lib.bank_ingest_bf16(x, fbank, table, n, P, C, rows, 1, None)
    _expect(fbank, table, 0, unit, P)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_ingest_without_norm_copies(backend, dtype):
    """test_cfg.with_norm=False: the rows as they are, no split copy"""
    lib = backend.hostlib
    n, P, C = 3, 23, 64
    x = _feats(n, P, C, seed=11, dtype=dtype)
    table, rows = _layout(n, P)
    fbank = torch.full((rows, C), SENTINEL, dtype=dtype)
    if dtype == torch.float32:
        lib.bank_ingest_f32(x, fbank, None, table, n, P, C, rows, 0, None)
    else:
        lib.bank_ingest_bf16(x, fbank, table, n, P, C, rows, 0, None)
    _expect(fbank, table, 0, x, P)


def test_ingest_leaves_out_an_image_outside_the_bank(emu_backend):
    """a destination that does not lie inside the bank - a negative row, a last row past the end - in either column: nothing of that
    image is written, the other images are"""
    lib = emu_backend.hostlib
    n, P, C = 3, 23, 64
    x = _feats(n, P, C, seed=13)
    good, rows = _layout(n, P)
    unit = torch.zeros(n, P, C)
    lib.l2norm_rows_f32(x.reshape(-1, C), unit, n * P, C, None)
    hl = torch.zeros(n, P, 2 * C, dtype=torch.bfloat16)
    lib.split_rows_bf16x2(unit.reshape(-1, C), hl, n * P, C, None)
    for col, bad in ((0, -1), (0, rows - P + 1), (1, -5), (1, rows)):
        table = good.clone()
        table[1, col] = bad
        fbank, hlbank = torch.full((rows, C), SENTINEL), torch.full((rows, 2 * C), SENTINEL, dtype=torch.bfloat16)
        lib.bank_ingest_f32(x, fbank, hlbank, table, n, P, C, rows, 1, None)
        _expect(fbank, table[[0, 2]], 0, unit[[0, 2]], P)
        _expect(hlbank, table[[0, 2]], 1, hl[[0, 2]], P)


def call_raw(be, name, args):
    """the entry point without the checking wrapper -> (return code, error text); tensors of `args` live on the backend's device"""
    lib = be.lib
    assert len(args) == len(lib.protos['vfs_' + name][1])
    rc = lib.cfunc(name)(*[a.data_ptr() if hasattr(a, 'data_ptr') else a for a in args])
    if be.dev.type == 'cuda':
        torch.cuda.synchronize()
    return rc, lib.last_error()


def test_ingest_argument_errors(backend):
    n, P, C = 2, 8, 64
    rows = n * P
    d = backend.d
    x, fb, hl = d(torch.zeros(n, P, C)), d(torch.zeros(rows, C)), d(torch.zeros(rows, 2 * C, dtype=torch.bfloat16))
    xb, fbb = d(torch.zeros(n, P, C, dtype=torch.bfloat16)), d(torch.zeros(rows, C, dtype=torch.bfloat16))
    table = d(torch.tensor([[0, 0], [P, P]], dtype=torch.int64))
    off = d(torch.zeros(rows * C + 4))[1:]      # 4 bytes past a 16-byte boundary
    for args, code, text in (
            ((x, fb, hl, table, 0, P, C, rows, 1, None), SHAPE, 'bank_ingest_f32: 1 <= n <= 65535 images'),
            ((x, fb, hl, table, 65536, P, C, rows, 1, None), SHAPE, 'bank_ingest_f32: 1 <= n <= 65535 images'),
            ((x, fb, hl, table, n, 0, C, rows, 1, None), SHAPE, 'bank_ingest_f32: P >= 1'),
            ((x, fb, hl, table, n, P, C, P - 1, 1, None), SHAPE, 'bank_rows >= P'),
            ((x, fb, None, table, n, P, 66, rows, 1, None), SHAPE, 'bank_ingest_f32: C % 4, C <= 2048'),
            ((x, fb, None, table, n, P, 2052, rows, 1, None), SHAPE, 'bank_ingest_f32: C % 4, C <= 2048'),
            ((x, fb, hl, table, n, P, 72, rows, 1, None), SHAPE, 'bank_ingest_f32: C % 16 for the split copy'),
            ((off, fb, hl, table, n, P, C, rows, 1, None), SHAPE, 'bank_ingest_f32: 16-byte aligned'),
            ((x, off, hl, table, n, P, C, rows, 1, None), SHAPE, 'bank_ingest_f32: 16-byte aligned'),
            ((x, fb, hl, table, n, P, C, rows, 0, None), ARG, 'bank_ingest_f32: a split copy is taken of unit rows only'),
            ((None, fb, hl, table, n, P, C, rows, 1, None), ARG, 'bank_ingest_f32: null buffer'),
            ((x, fb, hl, None, n, P, C, rows, 1, None), ARG, 'bank_ingest_f32: null buffer')):
        rc, msg = call_raw(backend, 'bank_ingest_f32', args)
        assert rc == code and text in msg, (args[4:], rc, msg)
    for args, code, text in (
            ((xb, fbb, table, 0, P, C, rows, 1, None), SHAPE, 'bank_ingest_bf16: 1 <= n <= 65535 images'),
            ((xb, fbb, table, n, P, 68, rows, 1, None), SHAPE, 'bank_ingest_bf16: C % 8, C <= 2048'),
            ((xb, None, table, n, P, C, rows, 1, None), ARG, 'bank_ingest_bf16: null buffer')):
        rc, msg = call_raw(backend, 'bank_ingest_bf16', args)
        assert rc == code and text in msg, (args[3:], rc, msg)
    assert float(fb.abs().max()) == 0.0 and float(hl.float().abs().max()) == 0.0 and float(fbb.float().abs().max()) == 0.0      # nothing ran
