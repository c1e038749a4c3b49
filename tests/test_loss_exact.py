"""Exact-operand parity of the loss kernels (cosine_loss_fwd / bwd and loss_means of csrc/misc.hip, csrc/simloss_dense.hip,
csrc/simloss.hip), the bf16 gradient buckets and the capped-grid streaming kernels (sgd_step, sgd_step_clip, scale, scale_by,
f32_to_bf16, imgs_to_nhwc4) against a float64 reference of the plain definition: every stored value is compared for equality;
the few bounded quantities are listed below with their derivation.

Operand recipe.  A row of C channels holds +-1 on its live channels and zeros elsewhere, with a squared norm n2 in {64, 256,
1024} (below 64 channels: a few +-2 among the +-1, n2 = 64).  The norm is a power of two, every dot product an integer, every
cosine a dyadic number with at most 11 bits; the last channel is always live, live positions, signs and n2 are drawn per row,
so the cosines of different (i, j) pairs differ and a wrong pairing, roll, channel guard or norm cannot pass.  Upstream
gradients are non-zero multiples of 1/4.  `weight` is chosen so that the kernel's scale factor is exact: a dyadic where the
position count is a power of two, S x dyadic (count x dyadic in gloss for the pairwise kernels) where it is not.  Every value
the kernels form from such operands is fp32-representable whatever the summation order or contraction, so the only correct
fp32 output is the float64 value and the only correct bf16 output its round-to-nearest-even.  Each case asserts the
precondition (`fp32_exact`: ref.float().double() == ref) on its own reference, pre-fills its outputs with NaN and compares
with `assert_exact`, which reports the count, the first index and the index range of the mismatches along every axis.

The float64 reference is the definition: cosine of the clamped-norm rows, 2 - 2 c or -c, the mean over positions, the rolls
composed as the reference tracker does (images2video, roll over time, video2images), autograd for the gradients.

Bounded quantities (everything else is equality):
  dense loss row, S not a power of two   the sum m of the S cosines is exact; the finish kernel forms inv = fl(1 / S),
        mu' = fl(m inv) (two roundings: mu' = mu (1 + e), |e| <= 2 u + u^2, u = 2^-24), l = fl(2 - 2 mu') (one rounding, 2 mu'
        is exact), s = fl(l1 / 2 + l2 / 2) (one), loss = fl(s w) (one).  First order:
        |loss - ref| <= w ((|mu1| + |mu2|) 2 u + (|l1| + |l2|) u / 2 + 2 u |s|); the test allows 1.001 times that for the
        second-order terms.  (The roundings after mu' cannot be left out: mu' is a full 24-bit number.)
  pairwise loss, Sa Sl not a power of two   the finish kernel divides the exact sum by the count in double, forms 2 - 2 m in
        double and rounds once to fp32: equal to the fp32 rounding of the float64 value up to a double rounding - one fp32 ulp.
  gradient of a zero p row   |p| is clamped to eps = float32(1e-12): gs = fl(g0 / eps) is one fp32 rounding of an exact g0,
        cos = 0, and gs (b / |b|) is a multiplication by a power of two.  The stored value is the bf16 rounding of a number
        within 2^-24 relative of the float64 value v: |got - v| <= 2^(e - 8) + 2^-23 |v|, e = floor(log2 |v|) (half a bf16
        ulp plus the fp32 rounding with room for a binade crossing); exactly 0 where v is 0.  One roll (K = 1), so no sum
        of rounded terms.

Streaming kernels: integer operands that depend on the index, lr = momentum = 1/2, wd = 1/4, coefficients of 1/2 - one step
is exact in fp32, an element updated twice or not at all shows.  The sizes are the issue's: one full pass of the capped grid
plus a second, partial trip and the scalar tail.  The emulator runs each of them in a fraction of a second, so none is
marked `gpu` only.

backend=emu: host build through the fiber emulator; backend=gpu: libvfs_hip.so on the MI355X."""
import numpy as np
import pytest
import torch

from oracle import vfs_oracle as O
from tests.test_bn_exact import fp32_exact, one_ulp, pm, rounded_share, seed
from tests.test_conv_exact import assert_bits, expect_bf16, ints, is_tie, nan_like

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
CPU = torch.device('cpu')
EPS = float(np.float32(1e-12))      # the kernels' clamp, as the double it is
SHAPE_ERR, ARG_ERR = -1, -3
U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------- helpers
def assert_exact(got, want, what, axes):
    """assert_bits, and on a mismatch the index range that holds mismatches along every (named) axis"""
    try:
        assert_bits(got, want, what, pixels=False)
    except AssertionError as e:
        if got.shape != want.shape or got.dtype != want.dtype:
            raise
        bad = (~(got.detach().cpu().double() == want.detach().cpu().double())).nonzero()
        where = [f'{name} {int(bad[:, d].min())}..{int(bad[:, d].max())} ({bad[:, d].unique().numel()} of {got.shape[d]})'
                 for d, name in enumerate(axes)]
        raise AssertionError(f'{e}; mismatches at ' + ', '.join(where)) from None


def unit_rows(g, lead, C, n2s=(64, 256, 1024)):
    """[*lead][C] fp32 rows of the recipe: per row a squared norm n2 drawn from the n2s that fit C (none fits: 64, with as many
    +-2 among the +-1 as it takes), live positions and signs drawn per row, channel C - 1 always live"""
    R = int(np.prod(lead))
    cands = [n for n in n2s if n <= C] or [64]
    n2 = torch.tensor(cands)[torch.randint(0, len(cands), (R,), generator=g)]
    twos = torch.clamp((n2 - C + 2) // 3, min=0)                  # 4 a + (L - a) = n2 with L = n2 - 3 a <= C live channels
    L = n2 - 3 * twos
    assert bool((L >= 1).all()) and bool((L <= C).all()) and bool((twos <= L - 1).all())
    rank = torch.rand(R, C - 1, generator=g).argsort(1).argsort(1)
    mag = (rank < (L - 1)[:, None]).float() + (rank < twos[:, None]).float()
    mag = torch.cat([mag, torch.ones(R, 1)], 1)
    rows = mag * pm(g, (R, C))
    sq = (rows.double() ** 2).sum(1)
    assert torch.equal(sq, n2.double()) and bool((rows[:, -1] != 0).all())
    return rows.reshape(*lead, C)


def dyadic_gloss(g, shape):
    """non-zero multiples of 1/4 in [-7/4, 7/4]"""
    return (pm(g, shape) * ints(g, shape, 1, 7) / 4).contiguous()


def cosines(a, b, eps=EPS):
    """[N][S][C] x [N][S][C] -> [N][S]: <a, b> / (max(|a|, eps) max(|b|, eps))"""
    na, nb = a.norm(dim=-1, keepdim=True).clamp_min(eps), b.norm(dim=-1, keepdim=True).clamp_min(eps)
    return ((a / na) * (b / nb)).sum(-1)


def rolled(x, T, k):
    """x [N][S][C] with every video of T frames rolled by k, as sim_siam_base_tracker.py composes it"""
    if k == 0:
        return x
    v = O.images2video(x.permute(0, 2, 1), T)
    return O.video2images(v.roll(k, dims=2)).permute(0, 2, 1)


def loss_rows(p1, z1, p2, z2, T, K, negative, w, eps=EPS):
    """float64 loss rows [K][N] of operands [N][S][C]: row k = w (L(p1, roll_k z2) / 2 + L(roll_k p2, z1) / 2), z detached"""
    def half(p, z):
        m = cosines(p, z.detach(), eps).mean(-1)
        return -m if negative else 2 - 2 * m
    return torch.stack([(half(p1, rolled(z2, T, k)) * 0.5 + half(rolled(p2, T, k), z1) * 0.5) * w for k in range(K)])


def reference(ops, gl, T, K, negative, w, eps=EPS):
    """(loss [K][N], dp1, dp2) in float64 from fp32 operands [N][S][C]"""
    p1, z1, p2, z2 = (t.double() for t in ops)
    p1.requires_grad_(True), p2.requires_grad_(True)
    loss = loss_rows(p1, z1, p2, z2, T, K, negative, w, eps)
    (loss * gl.double()).sum().backward()
    return loss.detach(), p1.grad, p2.grad


def frame_operands(g, N, C):
    return [unit_rows(g, (N,), C) for _ in range(4)]


def run_frame(be, ops, gl, N, C, T, K, negative, w):
    lib = be.hostlib
    args = [t.to(BF16).contiguous() for t in ops]
    loss = nan_like((K, N), CPU, F32)
    lib.cosine_loss_fwd(*args, loss, N, C, T, K, int(negative), w, None)
    dp1, dp2 = nan_like((N, C), CPU), nan_like((N, C), CPU)
    lib.cosine_loss_bwd(*args, gl, dp1, dp2, N, C, T, K, int(negative), w, None)
    return loss, dp1, dp2


def check_frame(be, ops, gl, N, C, T, K, negative, w, what):
    """the frame-level kernels on [N][C] operands against the reference; -> share of the gradients bf16 cannot hold"""
    rl, r1, r2 = reference([t[:, None, :] for t in ops], gl, T, K, negative, w)
    r1, r2 = r1[:, 0], r2[:, 0]
    fp32_exact(loss=rl, dp1=r1, dp2=r2)
    loss, dp1, dp2 = run_frame(be, ops, gl, N, C, T, K, negative, w)
    assert_exact(loss, rl.float(), what + ': loss', ('roll', 'row'))
    assert_exact(dp1, expect_bf16(r1), what + ': dp1', ('row', 'channel'))
    assert_exact(dp2, expect_bf16(r2), what + ': dp2', ('row', 'channel'))
    share = rounded_share(torch.cat([r1, r2]))
    print(f'{what}: {share:.3f} of the exact gradients are not bf16 values')
    return share


# ---------------------------------------------------------------------------------------------- 1. frame-level loss
#              N, C, T, K, negative, weight, asserts the rounded share
FRAME_CASES = [(8, 72, 4, 4, 0, 0.25, True),       # ragged 64-channel trip
               (6, 200, 3, 2, 1, 0.25, False),     # T = 3, 1 < K < T, negative
               (6, 200, 3, 3, 0, 0.5, False),      # T = 3, every roll
               (4, 2048, 2, 2, 0, 0.5, False),     # all MAXC = 32 accumulators
               (8, 128, 4, 1, 0, 1.0, False),      # no roll of T = 4
               (5, 64, 1, 1, 1, 1.0, False),       # no videos, negative
               (8, 130, 4, 3, 0, 0.25, True)]      # two channels past a 64-channel trip, 1 < K < T


@pytest.mark.parametrize('N,C,T,K,negative,w,rounds', FRAME_CASES)
def test_frame_loss(backend, N, C, T, K, negative, w, rounds):
    g = seed(21, N, C, T, K)
    ops = frame_operands(g, N, C)
    gl = dyadic_gloss(g, (K, N))
    share = check_frame(backend, ops, gl, N, C, T, K, negative, w, f'cosine_loss {N}x{C} T={T} K={K}')
    if rounds:
        assert share > 0.1, 'test bug: the rounding of the stored gradient is hardly exercised'


@pytest.mark.parametrize('negative', [0, 1])
def test_frame_loss_single_operand_use(backend, negative):
    """vfs_amd/sim_loss.py: L(p, z) through (p, z, p, z), T = K = 1, weight 1 forward and 2 backward; both gradient outputs
    hold dL/dp"""
    N, C = 6, 72
    g = seed(22, negative)
    p, z = unit_rows(g, (N,), C), unit_rows(g, (N,), C)
    gl = dyadic_gloss(g, (1, N))
    pd = p.double().requires_grad_(True)
    m = cosines(pd[:, None], z.double()[:, None]).mean(-1)
    ref = -m if negative else 2 - 2 * m
    (ref * gl[0].double()).sum().backward()
    fp32_exact(loss=ref.detach(), dp=pd.grad)
    lib = backend.hostlib
    pb, zb = p.to(BF16), z.to(BF16)
    loss = nan_like((1, N), CPU, F32)
    lib.cosine_loss_fwd(pb, zb, pb, zb, loss, N, C, 1, 1, negative, 1.0, None)
    assert_exact(loss[0], ref.detach().float(), 'single operand: loss', ('row',))
    dp, scratch = nan_like((N, C), CPU), nan_like((N, C), CPU)
    lib.cosine_loss_bwd(pb, zb, pb, zb, gl, dp, scratch, N, C, 1, 1, negative, 2.0, None)
    assert_exact(dp, expect_bf16(pd.grad), 'single operand: dp', ('row', 'channel'))
    assert_exact(scratch, expect_bf16(pd.grad), 'single operand: second output', ('row', 'channel'))


@pytest.mark.parametrize('N,C,T,K', [(8, 72, 4, 4), (5, 64, 1, 1)])
def test_frame_loss_zero_z_rows(backend, N, C, T, K):
    """a zero z row on either side: its norm takes the eps clamp, the cosine and the gradient against it are exactly 0"""
    g = seed(23, N, C)
    ops = frame_operands(g, N, C)
    ops[1][0] = 0           # z1[0]
    ops[3][N - 1] = 0       # z2[N - 1]
    gl = dyadic_gloss(g, (K, N))
    check_frame(backend, ops, gl, N, C, T, K, 0, 0.5, f'zero z rows {N}x{C} T={T}')
    if T == 1:      # no rolls: the rows that meet the zero z are known in full
        loss, dp1, dp2 = run_frame(backend, ops, gl, N, C, T, K, 0, 0.5)
        assert bool((dp1[N - 1].float() == 0).all()) and bool((dp2[0].float() == 0).all())
        c2 = cosines(ops[2].double()[:, None], ops[1].double()[:, None])[:, 0]
        c1 = cosines(ops[0].double()[:, None], ops[3].double()[:, None])[:, 0]
        assert float(c1[N - 1]) == 0.0 and float(c2[0]) == 0.0
        assert float(loss[0, N - 1]) == 0.5 * (0.5 * 2 + 0.5 * (2 - 2 * float(c2[N - 1])))
        assert float(loss[0, 0]) == 0.5 * (0.5 * (2 - 2 * float(c1[0])) + 0.5 * 2)


def test_frame_loss_zero_p_row(backend):
    """a zero p row on either side: |p| is clamped to eps = float32(1e-12), so cos = 0 (loss exact) and the gradient is
    gloss w / 2 * (-2) / eps * z / |z| - about 1e11, finite.  Against float64 of the same definition with that eps:
    |got - v| <= 2^(e - 8) + 2^-23 |v|, e = floor(log2 |v|): g0 = gloss w / 2 * (-2) is exact, fl(g0 / eps) is ONE fp32
    rounding (2^-24 |v|), the factor z / |z| is +-2^-3 ... (exact), cos * p / |p| is exactly 0, K = 1 so nothing is summed,
    and the bf16 store rounds to nearest: half a bf16 ulp, 2^(e - 8).  The second 2^-24 |v| covers a rounding that crosses a
    binade.  Where v is 0 the stored value is 0; every other row is compared for equality."""
    N, C, T, K, w = 4, 72, 2, 1, 0.5
    g = seed(24)
    ops = frame_operands(g, N, C)
    ops[0][1] = 0           # p1[1]
    ops[2][2] = 0           # p2[2]
    gl = dyadic_gloss(g, (K, N))
    rl, r1, r2 = reference([t[:, None, :] for t in ops], gl, T, K, 0, w)
    r1, r2 = r1[:, 0], r2[:, 0]
    fp32_exact(loss=rl)
    loss, dp1, dp2 = run_frame(backend, ops, gl, N, C, T, K, 0, w)
    assert_exact(loss, rl.float(), 'zero p row: loss', ('roll', 'row'))
    for name, got, ref, zero in (('dp1', dp1, r1, 1), ('dp2', dp2, r2, 2)):
        rest = [i for i in range(N) if i != zero]
        fp32_exact(rest=ref[rest])
        assert_exact(got[rest], expect_bf16(ref[rest]), f'zero p row: {name}, the other rows', ('row', 'channel'))
        v, x = ref[zero], got[zero].double()
        assert bool(torch.isfinite(x).all()) and float(v.abs().max()) > 1e9
        live = v != 0
        assert bool((x[~live] == 0).all())
        e = torch.floor(torch.log2(v[live].abs()))
        bound = 2.0 ** (e - 8) + 2.0 ** -23 * v[live].abs()
        err = (x[live] - v[live]).abs()
        print(f'zero p row: {name} worst error / bound {float((err / bound).max()):.3f}')
        assert bool((err <= bound).all()), f'zero p row: {name} is off by up to {float((err / bound).max())} of the bound'


def test_frame_loss_bwd_refuses_2056_channels(backend):
    """C = 2056 is past the 32 accumulators: the shape error, and nothing is written"""
    lib, dev = backend.lib, backend.dev
    N, C = 2, 2056
    z = torch.ones(N, C, dtype=BF16, device=dev)
    gl = torch.ones(1, N, device=dev)
    dp1, dp2 = nan_like((N, C), dev), nan_like((N, C), dev)
    args = (z, z, z, z, gl, dp1, dp2, N, C, 1, 1, 0, 1.0, None)
    assert len(args) == len(lib.protos['vfs_cosine_loss_bwd'][1])
    rc = lib.cfunc('cosine_loss_bwd')(*[a.data_ptr() if hasattr(a, 'data_ptr') else a for a in args])
    assert (rc, lib.last_error()) == (SHAPE_ERR, 'cosine_loss_bwd: C > 2048')
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    assert bool(torch.isnan(dp1.float()).all()) and bool(torch.isnan(dp2.float()).all())


# ---------------------------------------------------------------------------------------------- 2. per-position loss
def dense_plan(S, C):
    """the documented rule of vfs_dense_loss_split: lanes per position = the power of two >= C / 8 (at most 64), a unit = 4 waves
    of 64 / lpp positions -> (units, workgroups along z, 16-byte chunks per lane)"""
    nch = C // 8
    lpp = 1
    while lpp < nch and lpp < 64:
        lpp *= 2
    upw = 4 * (64 // lpp)
    nunits = (S + upw - 1) // upw
    return nunits, min(nunits, 32), (nch + lpp - 1) // lpp


def dense_workspace(lib, N, S, C, K):
    n = torch.zeros(1, dtype=torch.int64)
    lib.dense_cosine_loss_workspace_bytes(N, S, C, K, n)
    assert n.item() == K * N * dense_plan(S, C)[1] * 2 * 4
    return nan_like((n.item() // 4,), CPU, F32), n.item()


def run_dense(be, ops, gl, N, S, C, T, K, negative, w):
    lib = be.hostlib
    args = [t.to(BF16).contiguous() for t in ops]
    ws, nbytes = dense_workspace(be.lib, N, S, C, K)
    loss = nan_like((K, N), CPU, F32)
    lib.dense_cosine_loss_fwd(*args, loss, ws, nbytes, N, S, C, T, K, int(negative), w, None)
    dp1, dp2 = nan_like((N, S, C), CPU), nan_like((N, S, C), CPU)
    lib.dense_cosine_loss_bwd(*args, gl, dp1, dp2, N, S, C, T, K, int(negative), w, None)
    return loss, dp1, dp2


#              N, S, C, T, K, negative, weight, (units, chunks per lane) the case is there for, asserts the rounded share
DENSE_CASES = [(4, 16, 72, 2, 2, 0, 0.5, (1, 1), True),
               (4, 16, 72, 2, 2, 1, 0.5, (1, 1), True),             # negative
               (2, 8, 1024, 1, 1, 0, 1.0, (2, 2), False),           # the <2> instantiation
               (2, 4, 1536, 2, 2, 0, 0.5, (1, 3), True),            # three chunks in <DSL_MAX_CHUNKS>: its ch < nch guard is live
               (2, 256, 512, 2, 2, 0, 0.5, (64, 1), False),         # 64 units on 32 workgroups: every one makes two trips
               (2, 133, 2048, 2, 1, 0, 133 / 64, (34, 4), False),   # 34 units, the last with one position: two trips and one
               (3, 15, 72, 3, 3, 0, 15 / 4, (1, 1), True),          # ragged S, T = 3
               (4, 1, 64, 2, 2, 0, 0.5, (1, 1), False)]             # one position: the frame-level loss


@pytest.mark.parametrize('N,S,C,T,K,negative,w,plan,rounds', DENSE_CASES)
def test_dense_loss(backend, N, S, C, T, K, negative, w, plan, rounds):
    """gradients for equality at every S (the weight makes w / (2 S) exact); the loss for equality when S is a power of two
    and to the bound of the module docstring when it is not; the same bits on a second run; at S = 1 the frame-level kernel's
    bits"""
    nunits, Z, nchl = dense_plan(S, C)
    assert (nunits, nchl) == plan, 'test bug: the case no longer reaches the path it is there for'
    if S > 128:      # the multi-trip cases (dense_workspace ties Z to the library's own split)
        assert nunits > 32 and Z == 32, 'test bug: no workgroup makes a second trip of the unit loop'
    g = seed(25, N, S, C, T, K)
    ops = [unit_rows(g, (N, S), C) for _ in range(4)]
    gl = dyadic_gloss(g, (K, N))
    rl, r1, r2 = reference(ops, gl, T, K, negative, w)
    fp32_exact(dp1=r1, dp2=r2, weight=w, scale=w * 0.5 * 2 / S)
    loss, dp1, dp2 = run_dense(backend, ops, gl, N, S, C, T, K, negative, w)
    what = f'dense_cosine_loss {N}x{S}x{C} T={T} K={K}'
    if S & (S - 1) == 0:
        fp32_exact(loss=rl)
        assert_exact(loss, rl.float(), what + ': loss', ('roll', 'row'))
    else:
        p1, z1, p2, z2 = (t.double() for t in ops)
        bound = torch.empty(K, N, dtype=F64)
        for k in range(K):
            mu1, mu2 = cosines(p1, rolled(z2, T, k)).mean(-1).abs(), cosines(rolled(p2, T, k), z1).mean(-1).abs()
            l1, l2 = (mu1, mu2) if negative else (2 + 2 * mu1, 2 + 2 * mu2)      # upper bounds of |l|
            bound[k] = 1.001 * w * ((mu1 + mu2) * 2 * U + (l1 + l2) * U / 2 + 2 * U * (l1 + l2) / 2)
        err = (loss.double() - rl).abs()
        print(f'{what}: loss worst error / bound {float((err / bound).max()):.3f}')
        assert bool((err <= bound).all()), f'{what}: loss is off by up to {float((err / bound).max())} of the bound'
    assert_exact(dp1, expect_bf16(r1), what + ': dp1', ('image', 'position', 'channel'))
    assert_exact(dp2, expect_bf16(r2), what + ': dp2', ('image', 'position', 'channel'))
    share = rounded_share(torch.cat([r1, r2]))
    print(f'{what}: {share:.3f} of the exact gradients are not bf16 values')
    if rounds:
        assert share > 0.1, 'test bug: the rounding of the stored gradient is hardly exercised'
    again = run_dense(backend, ops, gl, N, S, C, T, K, negative, w)
    assert all(torch.equal(a.view(torch.int16) if a.dtype == BF16 else a, b.view(torch.int16) if b.dtype == BF16 else b)
               for a, b in zip((loss, dp1, dp2), again)), what + ': a second run gives other bits'
    if S == 1:
        floss, f1, f2 = run_frame(backend, [t[:, 0] for t in ops], gl, N, C, T, K, negative, w)
        assert_exact(loss, floss, what + ': loss against cosine_loss_fwd', ('roll', 'row'))
        assert_exact(dp1[:, 0], f1, what + ': dp1 against cosine_loss_bwd', ('row', 'channel'))
        assert_exact(dp2[:, 0], f2, what + ': dp2 against cosine_loss_bwd', ('row', 'channel'))


# ---------------------------------------------------------------------------------------------- 3. pairwise / spatial loss
def spatial_ref(a, l, mask, with_norm, pairwise, negative, w, gl):
    """sim_loss.py:42-63 in float64 on [B][C][S] operands -> loss [B], d loss / d (normalised operand), d loss / d operand, both
    sides"""
    a, l = a.double().requires_grad_(True), l.double().requires_grad_(True)
    ah = a / a.norm(dim=1, keepdim=True).clamp_min(EPS) if with_norm else a * 1
    lh = l / l.norm(dim=1, keepdim=True).clamp_min(EPS) if with_norm else l * 1
    ah.retain_grad(), lh.retain_grad()
    if pairwise:
        prod = torch.einsum('bci,bcj->bij', ah, lh)
        if mask is not None:
            prod = prod * mask.double()
        prod = prod.flatten(1)
    else:
        prod = (ah * lh).sum(1)
    m = prod.mean(-1)
    loss = (-m if negative else 2 - 2 * m) * w
    (loss * gl.double()).sum().backward()
    return loss.detach(), (ah.grad, a.grad), (lh.grad, l.grad)


def spatial_operands(g, B, C, S, with_norm):
    if not with_norm:
        return ints(g, (B, C, S), -3, 3).contiguous()
    return unit_rows(g, (B, S), C).permute(0, 2, 1).contiguous()


#                B, C, Sa, Sl, pairwise, with_norm, mask, negative, weight
SPATIAL_CASES = [(2, 64, 32, 32, 1, 1, True, 0, 1.0),
                 (2, 64, 32, 32, 1, 1, True, 1, 0.5),        # negative
                 (2, 70, 37, 50, 1, 1, True, 0, 1.0),        # rectangular, ragged against the 32-tiles, C % 8 != 0
                 (2, 33, 40, 40, 1, 0, False, 0, 1.0),       # no normalisation, no mask, integer operands
                 (3, 40, 36, 36, 0, 1, False, 0, 0.5)]       # the diagonal mode


@pytest.mark.parametrize('B,C,Sa,Sl,pairwise,with_norm,masked,negative,w', SPATIAL_CASES)
def test_spatial_loss(backend, B, C, Sa, Sl, pairwise, with_norm, masked, negative, w):
    """vfs_simloss_colnorm, _fwd, _bwd (both sides: mask_transposed 0 and 1) and _norm_bwd at the C ABI.  gloss = count x
    dyadic when the count is no power of two, so that coef = gloss w (-2) / count is exact and the gradients are compared for
    equality; the loss for equality when the count is a power of two, otherwise with the fp32 rounding of the float64 value to
    one ulp (module docstring)"""
    lib = backend.hostlib
    g = seed(26, B, C, Sa, Sl, negative)
    a, l = spatial_operands(g, B, C, Sa, with_norm), spatial_operands(g, B, C, Sl, with_norm)
    mask = (torch.rand(B, Sa, Sl, generator=g) < 0.6).float().contiguous() if masked else None
    count = Sa * Sl if pairwise else Sa
    gl = dyadic_gloss(g, (B,)) * (1 if count & (count - 1) == 0 else count)
    rl, (rda, rdxa), (rdl, rdxl) = spatial_ref(a, l, mask, with_norm, pairwise, negative, w, gl)
    fp32_exact(gloss=gl, da=rda, dxa=rdxa, dl=rdl, dxl=rdxl)
    what = f'simloss {B}x{C}x{Sa}x{Sl}'
    inva = invl = None
    if with_norm:
        inva, invl = nan_like((B, Sa), CPU, F32), nan_like((B, Sl), CPU, F32)
        lib.simloss_colnorm(a, inva, B, C, Sa, None)
        lib.simloss_colnorm(l, invl, B, C, Sl, None)
        assert_exact(inva, (1 / a.double().norm(dim=1)).float(), what + ': colnorm of a', ('sample', 'position'))
        assert_exact(invl, (1 / l.double().norm(dim=1)).float(), what + ': colnorm of l', ('sample', 'position'))
    tiles = ((Sa + 31) // 32) * (((Sl + 31) // 32) if pairwise else 1)
    partial, loss = nan_like((B * tiles,), CPU, F32), nan_like((B,), CPU, F32)
    lib.simloss_fwd(a, l, inva, invl, mask, partial, loss, B, C, Sa, Sl, pairwise, negative, w, None)
    if count & (count - 1) == 0:
        fp32_exact(loss=rl)
        assert_exact(loss, rl.float(), what + ': loss', ('sample',))
    else:
        err = (loss.double() - rl.float().double()).abs()
        print(f'{what}: loss differs from the rounded float64 value by up to {float((err / one_ulp(rl.float().double())).max())} ulp')
        assert bool((err <= one_ulp(rl.float().double())).all()), f'{what}: loss {loss.tolist()} against {rl.tolist()}'
    for side, x, invx, other, invo, Sx, So, transposed, rd, rdx in (('a', a, inva, l, invl, Sa, Sl, 0, rda, rdxa),
                                                                    ('l', l, invl, a, inva, Sl, Sa, 1, rdl, rdxl)):
        d = nan_like((B, C, Sx), CPU, F32)
        lib.simloss_bwd(other, invo, mask, transposed, gl, d, B, C, Sx, So, pairwise, negative, w, None)
        assert_exact(d, rd.float(), f'{what}: simloss_bwd, side {side}', ('sample', 'channel', 'position'))
        dx = nan_like((B, C, Sx), CPU, F32)
        lib.simloss_norm_bwd(x, invx, d, dx, B, C, Sx, None)
        assert_exact(dx, rdx.float(), f'{what}: simloss_norm_bwd, side {side}', ('sample', 'channel', 'position'))


# ---------------------------------------------------------------------------------------------- 4. loss_means
@pytest.mark.parametrize('K', [1, 4])
@pytest.mark.parametrize('N', [1, 6, 64, 200])
def test_loss_means(backend, K, N):
    """rows of N x quarters: every mean is a quarter-integer, means[K] their sum"""
    g = seed(27, K, N)
    loss = (ints(g, (K, N), -40, 40) * N / 4).contiguous()
    want = torch.cat([loss.double().mean(1), loss.double().mean(1).sum()[None]])
    fp32_exact(rows=loss.double(), means=want)
    assert torch.equal(want[:K] * 4 * N, (loss.double().sum(1) * 4)) and torch.equal(want * 4, (want * 4).round())
    means = nan_like((K + 1,), CPU, F32)
    backend.hostlib.loss_means(loss, means, K, N, None)
    assert_exact(means, want.float(), f'loss_means K={K} N={N}', ('entry',))


# ---------------------------------------------------------------------------------------------- 5. gradient buckets
BF16_MAX = float(torch.finfo(BF16).max)


def bucket_values(g, n):
    """+-0, the largest finite bf16, a block of exact bf16 ties of both parities (+-(257 + 2 j): between two bf16 values of
    spacing 2; RNE rounds j even down and j odd up), then 17-bit integers"""
    j = torch.arange(128).double()
    ties = torch.stack([257 + 2 * j, -(257 + 2 * j)], 1).reshape(-1)
    assert bool(is_tie(ties).all())
    up = expect_bf16(ties).double().abs() > ties.abs()
    assert int(up.sum()) == 128 and bool((up[0::4] == False).all()) and bool(up[2::4].all())      # noqa: E712
    head = torch.cat([torch.tensor([0.0, -0.0, BF16_MAX, -BF16_MAX], dtype=F64), ties]).float()
    if n <= head.numel():
        return head[:n].clone()
    return torch.cat([head, ints(g, (n - head.numel(),), -65535, 65535)])


@pytest.mark.parametrize('scale', [1.0, 0.5, 0.25])
@pytest.mark.parametrize('n', [1, 7, 8, 1027])
def test_gradient_buckets(backend, n, scale):
    """dst = bf16(src scale) bit for bit (the sign of a zero included), bf16_to_f32 returns the stored values, and converting
    those again changes nothing"""
    lib = backend.hostlib
    src = bucket_values(seed(28, n), n)
    ref = src.double() * scale
    fp32_exact(product=ref)
    want = expect_bf16(ref)
    if n > 1000:
        assert rounded_share(ref) > 0.1, 'test bug: the rounding is hardly exercised'
    dst = nan_like((n,), CPU)
    lib.f32_to_bf16(src, dst, n, scale, None)
    what = f'f32_to_bf16 n={n} scale={scale}'
    assert_exact(dst, want, what, ('element',))
    assert torch.equal(dst.view(torch.int16), want.view(torch.int16)), what + ': bit patterns (the sign of a zero)'
    back = nan_like((n,), CPU, F32)
    lib.bf16_to_f32(dst, back, n, None)
    assert_exact(back, want.float(), f'bf16_to_f32 n={n}', ('element',))
    assert torch.equal(back.view(torch.int32), want.float().view(torch.int32))
    again = nan_like((n,), CPU)
    lib.f32_to_bf16(back, again, n, 1.0, None)
    assert torch.equal(again.view(torch.int16), dst.view(torch.int16)), what + ': the round trip changes a value'


@pytest.mark.parametrize('name', ['f32_to_bf16', 'bf16_to_f32'])
@pytest.mark.parametrize('which', [0, 1])
def test_gradient_buckets_refuse_unaligned_buffers(backend, name, which):
    lib, dev = backend.lib, backend.dev
    P = nan_like((64,), dev, F32)
    bufs = [P, P]
    bufs[which] = P[1:]
    args = (bufs[0], bufs[1], 8) + ((1.0,) if name == 'f32_to_bf16' else ()) + (None,)
    assert len(args) == len(lib.protos['vfs_' + name][1])
    rc = lib.cfunc(name)(*[a.data_ptr() if hasattr(a, 'data_ptr') else a for a in args])
    assert (rc, lib.last_error()) == (ARG_ERR, name + ': 16-byte aligned buffers')
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    assert bool(torch.isnan(P).all())


# ---------------------------------------------------------------------------------------------- 6. second trip of the capped grids
CAP = 4096                                    # workgroups of the sgd / scale / bucket launches
N_QUAD = CAP * 256 * 4 + 4 * 256 + 3          # one pass of four-word lanes, one more workgroup's worth, the scalar tail
N_ONE = CAP * 256 + 259
N_OCT = CAP * 256 * 8 + 8 * 256 + 5


def by_index(n, mul, mod):
    """integers in [-mod / 2, mod / 2] that depend on the index"""
    return ((torch.arange(n, dtype=torch.int64) * mul) % mod - mod // 2).float()


def where_1d(bad):
    idx = bad.nonzero()[:, 0]
    return f'{idx.numel()} of {bad.numel()} elements differ, first at {int(idx[0])}, last at {int(idx[-1])}'


def assert_stream(got, want64, what):
    fp32_exact(**{'reference': want64})
    bad = ~(got.double() == want64)
    assert not bool(bad.any()), f'{what}: {where_1d(bad)} (one pass of the grid ends at word {CAP * 256} x the words per lane)'


@pytest.mark.parametrize('clip', [False, True])
def test_sgd_second_trip(backend, clip):
    """g (c) + wd p, buf / 2 + that, p - buf / 2 on integers: eighths, exact"""
    n = N_QUAD
    p, gr, buf = by_index(n, 7, 251), by_index(n, 13, 127), by_index(n, 29, 61)
    c = 0.5 if clip else 1.0
    b64 = 0.5 * buf.double() + (gr.double() * c + 0.25 * p.double())
    p64 = p.double() - 0.5 * b64
    g0 = gr.clone()
    if clip:
        backend.hostlib.sgd_step_clip(p, gr, buf, n, 0.5, 0.5, 0.25, torch.tensor([0.5]), None, None)
    else:
        backend.hostlib.sgd_step(p, gr, buf, n, 0.5, 0.5, 0.25, None, None)
    assert_stream(buf, b64, f'sgd_step{"_clip" if clip else ""}: momentum')
    assert_stream(p, p64, f'sgd_step{"_clip" if clip else ""}: parameters')
    assert torch.equal(gr, g0)


def test_scale_by_second_trip(backend):
    n = N_QUAD
    x = by_index(n, 7, 2047)
    want = x.double() * 0.5
    backend.hostlib.scale_by(x, n, torch.tensor([0.5]), None)
    assert_stream(x, want, 'scale_by')


def test_scale_second_trip(backend):
    n = N_ONE
    x = by_index(n, 7, 2047)
    want = x.double() * 0.5
    backend.hostlib.scale(x, n, 0.5, None)
    assert_stream(x, want, 'scale')


def test_f32_to_bf16_second_trip(backend):
    n = N_OCT
    src = by_index(n, 7919, 131071)
    ref = src.double() * 0.5
    fp32_exact(product=ref)
    assert rounded_share(ref[:100000]) > 0.1
    dst = nan_like((n,), CPU)
    backend.hostlib.f32_to_bf16(src, dst, n, 0.5, None)
    bad = ~(dst.double() == expect_bf16(ref).double())
    assert not bool(bad.any()), f'f32_to_bf16: {where_1d(bad)} (one pass of the grid ends at element {CAP * 256 * 8})'


def test_imgs_to_nhwc4_second_trip(backend):
    """8 frames of 512 x 514 padded positions = 8192 x 256 + 8192: the last 8192 positions belong to a second trip.  W = 513 < Wp:
    the padding column and the fourth channel are zeros; 11-bit integers, so the stored value is the RNE rounding"""
    B, V, T, H, W, Wp = 2, 2, 2, 512, 513, 514
    assert 8192 * 256 < V * B * T * H * Wp < 8192 * 256 + 8192 * 2
    imgs = by_index(B * V * 3 * T * H * W, 7919, 2047).reshape(B, V, 3, T, H, W)
    want = torch.zeros(V, B, T, H, Wp, 4, dtype=F64)
    want[..., :W, :3] = imgs.double().permute(1, 0, 3, 4, 5, 2)
    assert rounded_share(want[0, 0, 0, :, :W, :3]) > 0.1
    out = nan_like((V * B * T, H, Wp, 4), CPU)
    backend.hostlib.imgs_to_nhwc4(imgs, out, B, V, T, H, W, Wp, None)
    assert_exact(out, expect_bf16(want).reshape(V * B * T, H, Wp, 4), 'imgs_to_nhwc4', ('frame', 'row', 'column', 'channel'))
