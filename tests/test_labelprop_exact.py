"""Exact-operand parity of the bf16 label-propagation kernels (vfs_amd/csrc/labelprop.hip: labelprop_kernel, labelprop_merge_kernel,
l2norm_rows_kernel, seg_minmax_kernel, seg_argmax_kernel, onehot_kernel) at the C ABI against numpy float64 references written
here.  Only the spatial mask comes from oracle/vfs_oracle.py.  u = 2^-24 is the fp32 unit roundoff throughout.

1. Affinity + top-k.  The feature bank is passed as it is (the kernel does not normalise).  Features are integers times a power of
   two `fs`, the temperature is a power of two and fs^2 / temperature = 2^-10, so every score is an integer number of 2^-10 and is
   exact in fp32 in any MFMA order: each case asserts sum_c |q_c| |k_c| / fs^2 < 2^24 and C max|q| max|k| / temperature < 2^24.
     * Four "tag" channels, one in every quarter of the channel range (so every 64-channel K-step of C = 256 holds one).  A key
       pixel of bank frame t holds there the four base-8 digits of a code that is unique over (t, pixel) - a random permutation of
       0..4095.  The query pixel holds +-8^pi(i) there, with the permutation pi and the signs chosen by the pixel index.  The score
       is then a signed mixed-radix reading of the code: injective for every query, different from query to query, within a span
       of 4095 * 2^-10 < 4, so that the 10th kept weight is at least e^-4 / 10 > 2^-10 of the sum (asserted for every query).
     * All other channels hold non-zero integers in pairs (c, c + C/2): the query the same x in both, the key y and -y.  They
       cancel exactly, but only if both halves of the channel range are read, from the right pixel.
     * Frames that are neither query nor key hold keys with codes of their own: a wrong slot gives a plausible, different list.
   The float64 score matrix is masked with oracle.spatial_neighbor_circle; no two in-mask candidates of a query are equal
   (asserted).  The workspace is filled with int32 -1 (a NaN as float) before the call; the partial lists are read back and
   checked entry by entry: value == exact score of the id, id inside the mask, strictly descending then (-inf, -1), the rows
   of a query cover disjoint increasing key ranges, the ten best of their union are the reference's ten best with their ids, rows
   are written for the same leading splits for every query and nothing else is touched.  The launcher's split rule is not
   mirrored: written rows are those without the sentinel.

   `out` against softmax(top-k) @ seg in float64, bound c u sum_k w_k |v_k| with c = 32.  Chain of labelprop_merge_kernel:
   bv[k] - m is exact (multiples of 2^-10 below 8); expf within 2 ulp, 4 u (the device's is documented at 1 ulp); z, nine
   additions of positive terms, 9 u on top of the 4 u of its terms, so 1 / z carries 13 u and its own rounding u; wgt * iz u; the
   product with the value u; the ten-term sum 9 u on the partial sums, which sum_k w_k |v_k| bounds.  4 + 14 + 1 + 1 + 9 = 29 u
   per term, second-order terms and a contraction into fma (which only removes roundings) leave c = 32 <= 64.  With weights
   between e^-4 / 10 and 1 a lost, doubled or swapped entry moves `out` by about 2^-10 |v| at the least, 2^9 times the bound.

   Ties.  Two candidates of equal score with different ids: the kernel keeps the one it met first, which is lane order inside a
   key block (a lane owns keys tm * 16 + 4 * (lane / 16) + reg), then block, frame and split order - not id order - and
   torch.topk leaves the choice unspecified as well.  Nothing is asserted about ties between distinct candidates; no case but
   the tie case has any.  The tie case is the DAVIS duplicated first frame, slots [0, 0, 1, 2]: key 0 and key 1 are the same
   bank frame, every candidate ties with its twin.  The value sequence must be the reference's, the ids either twin (compared
   after mapping the key index to its slot) and no id twice; `out` to the same bound, since both twins read one seg row.

2. l2norm_rows.  Exact regime: rows of n in {1, 4, 16, 64, 256} entries +-2^a: sum of squares n 4^a in any order, sqrtf and
   1 / . exact, every output +-2^-log2(sqrt n) by equality; a zero row gives zeros.  General regime: random bf16 rows of norms
   2^-20 .. 2^20 against x / max(||x||, 1e-12) in float64, element by element: every output is one of the two bf16 neighbours
   of the reference, and the round-to-nearest-even one wherever the reference is farther from the midpoint of the two than the
   kernel's fp32 error E |ref|, E = (C + 8) u: the sum of C squares carries u per square and u per addition on any path, at most
   C u relative as all terms are positive; sqrtf halves it and adds u, the reciprocal u, the product u: (C / 2 + 3) u <= E.  The
   share of elements excused is asserted below 10 % on the reference (the band is 2 E wide against a midpoint spacing of at least
   2^-8: (C + 8) 2^-15, 6.3 % at C = 2048).

3. seg_postprocess.  Exact regime: power-of-two upscales of integer maps: the source coordinate, the weights (multiples of 1/16)
   and the bilerp are exact in fp32 (asserted: the float64 bilerp is an fp32 value).  Channels have max - min a power of two >= 1
   (then fl(max - min + 1e-12f) = max - min and the quotient is exact), or max <= 0 (left as they are), or are constant (0 / 1e-12f
   = 0).  The reference applies the fp32 value of the denominator, fl32(max - min + 1e-12f), which is a single correctly rounded
   operation, and is asserted to equal max - min or 1e-12f.  Labels by equality with numpy argmax (first maximum), `partial`
   reduced over its rows by equality with the reference's min / max.
   General regime: random fp32 maps, non-dyadic ratios.  fp32 error of a sample of channel c: the coordinate fl(fl(s (o + .5)) - .5)
   is off by at most 3 u max(H, W) (s, the product, the difference), each of the two lerps moves by that times a neighbour
   difference <= R_c = max - min of the channel, and the three lerps round 2 u each on values <= M_c = max |.|:
   e_c = u (6 max(H, W) R_c + 6 M_c).  Normalised (v - mn) / D: v, mn and mx each carry e_c, the subtraction, the sum and the
   quotient u each: n_c = 4 e_c / D + 3 u.  A pixel whose label differs from the float64 argmax b must have ref[b] - ref[a] <=
   n_a + n_b for the label a it got; the near-ties of the reference are the pixels where any other channel is that close to the
   best, so the mismatches are a subset of them.  Both shares are printed.

backend=emu: host build through the fiber emulator; backend=gpu: libvfs_hip.so on the MI355X."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

from oracle import vfs_oracle as O
from tests.test_siamfc_exact import call_raw

BF16 = torch.bfloat16
U = 2.0 ** -24
SHAPE_ERR, ARG_ERR = -1, -3
LP_ROWS, LP_K = 96, 10           # vfs_labelprop_workspace_bytes: [96][H*W][10] values, then as many ids
C_SOFTMAX = 32
WORST = {}                       # backend -> largest used fraction of the softmax bound (printed by every case)


# ---------------------------------------------------------------------------------------------- bf16 in numpy
def bf16_grid(x64):
    """-> (down, up, rne, mid) as float64: the bf16 neighbours of |x| (down <= |x| <= up, equal when x is a bf16 value), its
    round-to-nearest-even and the midpoint of the neighbours, all carrying the sign of x.  Normal range only."""
    x64 = np.asarray(x64, dtype=np.float64)
    a = np.abs(x64)
    _, e = np.frexp(np.where(a > 0, a, 1.0))
    ulp = np.ldexp(1.0, e - 8)                       # |x| = m 2^e, m in [0.5, 1): eight significant bits
    q = a / ulp
    lo, rne = np.floor(q), np.rint(q)
    hi = np.where(lo == q, lo, lo + 1)
    s = np.sign(x64)
    return s * lo * ulp, s * hi * ulp, s * rne * ulp, s * (lo + 0.5) * ulp


def as_bf16(x64):
    """float64 array of bf16 values -> torch bf16, checked to lose nothing"""
    t = torch.from_numpy(np.ascontiguousarray(x64, dtype=np.float32))
    b = t.to(BF16)
    assert torch.equal(b.float(), t), 'test bug: an operand is not a bf16 value'
    return b


def rng(*key):
    return np.random.default_rng([20240611, *key])


# ---------------------------------------------------------------------------------------------- 1. affinity + top-k
TAG_PERMS = list(itertools.permutations(range(4)))


def lp_operands(T, H, W, C, CO, qframe, fs, salt):
    """-> bank [T][HW][C] float64 (bf16 values), seg [T][HW][CO] float32"""
    g = rng(1, salt)
    HW, half = H * W, C // 2
    assert (T - 1) * HW <= 4096, 'test bug: more key pixels than codes'
    tags = [1, C // 4 + 2, C // 2 + 3, 3 * C // 4 + 4]
    noise = np.array([c for c in range(half) if c not in [t % half for t in tags]])
    bank = np.zeros((T, HW, C))
    code = g.permutation(4096)[:(T - 1) * HW].reshape(T - 1, HW)
    mag = lambda shape: g.integers(1, 16, shape) * g.choice([-1, 1], shape)      # noqa: E731
    for t in range(T):
        if t == qframe:
            x = mag((HW, len(noise)))
            bank[t][:, noise], bank[t][:, noise + half] = x, x
            for p in range(HW):
                v = (p * 7 + 3) % 384
                for i in range(4):
                    bank[t, p, tags[i]] = (1 - 2 * ((v >> i) & 1)) * 8 ** TAG_PERMS[v // 16][i]
        else:
            y = mag((HW, len(noise)))
            bank[t][:, noise], bank[t][:, noise + half] = y, -y
            cd = code[t - (t > qframe)]
            for i in range(4):
                bank[t][:, tags[i]] = (cd >> (3 * i)) & 7
    seg = (g.standard_normal((T, HW, CO)) * 2).astype(np.float32)
    return bank * fs, seg


def lp_mask(H, W, nkeys, radius, non_mask_len):
    """[HW queries][nkeys * HW candidates] bool"""
    HW = H * W
    full = np.ones((HW, HW), dtype=bool)
    circle = O.spatial_neighbor_circle(H, W, 2 * radius).numpy() if radius > 0 else full
    return np.concatenate([full if f < non_mask_len else circle for f in range(nkeys)], axis=1)


#  tag: (H, W, C, radius, slots, qframe, T, topk, non_mask_len, (fs, temperature))
S7, T4 = (2.0 ** -7, 2.0 ** -4), (2.0 ** -5, 1.0)
LP_CASES = {
    'one_tile_8x8': (8, 8, 64, 2, [0, 1], 2, 3, 10, 0, S7),
    'ragged_9x13_unsorted_slots_qframe_inside': (9, 13, 64, 4, [6, 1, 4, 0, 3], 2, 8, 10, 0, S7),
    'blocks_20x28_r6': (20, 28, 64, 6, [0, 1, 2], 3, 4, 10, 0, S7),
    'c128': (9, 13, 128, 2, [2, 0], 1, 3, 10, 0, T4),
    'c256': (9, 13, 256, 3, [0, 1, 3], 2, 4, 10, 0, (1.0, 1024.0)),
    'radius0_no_mask': (9, 13, 64, 0, [1, 0], 2, 3, 10, 0, S7),
    'radius1_own_pixel': (9, 13, 64, 1, [0, 1, 2, 3, 4], 5, 6, 10, 0, S7),
    'radius_larger_than_map': (9, 13, 64, 40, [0, 1], 2, 3, 10, 0, T4),
    'radius1_single_candidate': (9, 13, 64, 1, [1], 0, 2, 10, 0, S7),
    'radius1_three_candidates_topk10': (9, 13, 64, 1, [0, 2, 1], 3, 4, 10, 0, S7),
    'nkeys1': (8, 8, 64, 2, [0], 1, 2, 10, 0, S7),
    'nkeys5': (8, 8, 64, 2, [0, 1, 2, 3, 4], 5, 6, 10, 0, S7),
    'nkeys24': (8, 8, 64, 2, list(range(24)), 24, 25, 10, 0, S7),
    'nkeys25_two_frames_per_workgroup': (8, 8, 64, 2, list(range(25)), 25, 26, 10, 0, S7),
    'nkeys64_three_frames_per_workgroup': (8, 8, 64, 2, list(range(64)), 64, 65, 10, 0, S7),
    'nkeys25_c128_radius0': (8, 8, 128, 0, list(range(24, -1, -1)), 25, 26, 10, 0, T4),
    'topk1': (9, 13, 64, 2, [0, 1], 2, 3, 1, 0, S7),
    'topk5': (9, 13, 64, 2, [0, 1], 2, 3, 5, 0, S7),
    'topk5_radius1_three_candidates': (9, 13, 64, 1, [0, 1, 2], 3, 4, 5, 0, S7),
    'non_mask_len1': (9, 13, 64, 2, [2, 0, 1], 3, 4, 10, 1, S7),
    'non_mask_len1_topk5': (9, 13, 64, 1, [0, 1, 2], 3, 4, 5, 1, S7),
    'radius0_non_mask_len_nkeys': (8, 8, 64, 0, [0, 1, 2], 3, 4, 10, 3, S7),
    'twin_first_frame': (9, 13, 64, 3, [0, 0, 1, 2], 3, 4, 10, 0, S7),
    'twin_first_frame_unmasked': (8, 8, 128, 2, [0, 0, 1, 2], 3, 4, 10, 1, T4),
}


@functools.lru_cache(maxsize=None)
def lp_reference(tag):
    """everything a case needs, computed once per process and never written to"""
    H, W, C, radius, slots, qframe, T, topk, nml, (fs, temp) = LP_CASES[tag]
    salt = list(LP_CASES).index(tag)
    HW, nkeys, CO = H * W, len(slots), 3
    bank, seg = lp_operands(T, H, W, C, CO, qframe, fs, salt)
    assert fs * fs / temp == 2.0 ** -10 and 1.0 / np.float32(temp) == 1.0 / temp
    q, k = bank[qframe], bank[slots].reshape(nkeys * HW, C)
    assert C * np.abs(q).max() * np.abs(k).max() / temp < 2 ** 24
    assert (np.abs(q) @ np.abs(k).T).max() / (fs * fs) < 2 ** 24, 'test bug: a partial sum may not be an fp32 value'
    S = (q @ k.T) / temp
    assert np.array_equal(S, S.astype(np.float32)) and np.array_equal(S * 1024, np.rint(S * 1024))
    M = lp_mask(H, W, nkeys, radius, nml)
    Sm = np.where(M, S, -np.inf)
    order = np.argsort(-Sm, axis=1, kind='stable')[:, :LP_K + 1]                  # ties: lower id first
    top = np.take_along_axis(Sm, order, axis=1)
    ncand = M.sum(axis=1)
    twins = len(set(slots)) < nkeys
    canon = np.array(slots)[np.arange(nkeys * HW) // HW] * HW + np.arange(nkeys * HW) % HW
    for r in range(HW):                                                          # no two in-mask candidates of a query are equal
        ids = np.nonzero(M[r])[0]
        key = np.unique(canon[ids]) if twins else ids
        vals = S[r, key] if not twins else np.array([S[r, ids[canon[ids] == c][0]] for c in key])
        assert len(np.unique(vals)) == len(key), f'test bug: query {r} has tied candidates'
    K = np.minimum(topk, ncand)
    w = np.where(np.arange(LP_K)[None] < K[:, None], np.exp(top[:, :LP_K] - top[:, :1]), 0.0)
    w /= w.sum(axis=1, keepdims=True)
    kept = w[np.arange(HW), K - 1]
    assert (kept >= 2.0 ** -10).mean() >= 0.9, 'test bug: the last kept weight is too small to be seen'
    vals = seg[np.array(slots)].reshape(nkeys * HW, CO).astype(np.float64)
    ids10 = np.where(top[:, :LP_K] > -np.inf, order[:, :LP_K], 0)
    v = vals[ids10]                                                              # [HW][10][CO]
    out = (w[:, :, None] * v).sum(axis=1)
    bound = C_SOFTMAX * U * (w[:, :, None] * np.abs(v)).sum(axis=1)
    return dict(bank=bank, seg=seg, S=S, M=M, order=order, top=top, ncand=ncand, canon=canon, out=out, bound=bound, twins=twins)


def lp_edge(tag):
    """the property a case is there for, on its own numbers"""
    H, W, C, radius, slots, qframe, T, topk, nml, _ = LP_CASES[tag]
    nkeys, tiles = len(slots), ((H + 7) // 8) * ((W + 7) // 8)
    win = min(H, 8 + 2 * (radius - 1)) * min(W, 8 + 2 * (radius - 1)) if radius > 0 else H * W
    return {'one_tile_8x8': tiles == 1, 'ragged_9x13_unsorted_slots_qframe_inside': H % 8 and W % 8 and qframe < T - 1 and slots != sorted(slots),
            'blocks_20x28_r6': win > 256 and win % 128 != 0, 'c128': C == 128, 'c256': C == 256, 'radius0_no_mask': radius == 0,
            'radius1_own_pixel': radius == 1, 'radius_larger_than_map': radius > max(H, W), 'radius1_single_candidate': nkeys == 1 and radius == 1,
            'radius1_three_candidates_topk10': nkeys == 3 and radius == 1 and topk == 10, 'nkeys1': nkeys == 1, 'nkeys5': nkeys == 5,
            'nkeys24': nkeys == 24, 'nkeys25_two_frames_per_workgroup': nkeys == 25, 'nkeys64_three_frames_per_workgroup': nkeys == 64,
            'nkeys25_c128_radius0': nkeys == 25 and C == 128, 'topk1': topk == 1, 'topk5': topk == 5,
            'topk5_radius1_three_candidates': topk == 5 and radius == 1, 'non_mask_len1': nml == 1 and radius > 0,
            'non_mask_len1_topk5': nml == 1 and topk == 5, 'radius0_non_mask_len_nkeys': radius == 0 and nml == nkeys,
            'twin_first_frame': slots[:2] == [0, 0], 'twin_first_frame_unmasked': slots[:2] == [0, 0] and nml == 1}[tag]


def check_partial_lists(tag, ref, pval, pidx, HW, nkeys):
    """pval / pidx: [96][HW][10] as read back"""
    S, M, canon = ref['S'], ref['M'], ref['canon']
    written = ~np.isnan(pval)
    rows = written.all(axis=2)
    assert np.array_equal(rows, written.any(axis=2)), f'{tag}: a partial list is written in part'
    nrows = rows.sum(axis=0)
    assert (nrows == nrows[0]).all() and nrows[0] >= 1, f'{tag}: queries have different numbers of partial lists: {np.unique(nrows)}'
    n = int(nrows[0])
    assert rows[:n].all() and not rows[n:].any(), f'{tag}: the written rows are not the leading {n} splits'
    assert (pidx[n:] == -1).all(), f'{tag}: ids past the written rows were touched'
    assert n <= nkeys
    valid = pval[:n] > -np.inf
    # strictly descending, then (-inf, -1)
    assert (valid[:, :, :-1] >= valid[:, :, 1:]).all(), f'{tag}: a list has an entry after its end'
    both = valid[:, :, :-1] & valid[:, :, 1:]
    assert (pval[:n][:, :, :-1][both] > pval[:n][:, :, 1:][both]).all(), f'{tag}: a list is not strictly descending'
    empty_ok = (pval[:n][~valid] == -np.inf).all() and (pidx[:n][~valid] == -1).all()
    assert empty_ok, (f'{tag}: the entries past a list\'s end are not (-inf, -1): ids '
                      f'{np.unique(pidx[:n][~valid])[:8]}, {int((pidx[:n][~valid] != -1).sum())} of {int((~valid).sum())}')
    assert valid[:, :, 0].all(), f'{tag}: a split without any candidate (every key frame holds at least the own pixel)'
    ids = np.where(valid, pidx[:n], 0)
    assert (pidx[:n][valid] >= 0).all() and (pidx[:n][valid] < nkeys * HW).all(), f'{tag}: an id outside [0, nkeys * HW)'
    qi = np.broadcast_to(np.arange(HW)[None, :, None], ids.shape)
    assert M[qi, ids][valid].all(), f'{tag}: a listed candidate lies outside the mask'
    exact = S[qi, ids].astype(np.float32)
    bad = valid & (pval[:n] != exact)
    assert not bad.any(), (f'{tag}: {int(bad.sum())} listed values are not the score of their id; first (split, query, place) '
                           f'{tuple(np.argwhere(bad)[0])}: {pval[:n][bad][0]!r} against {exact[bad][0]!r}')
    # disjoint, increasing key ranges from split to split
    key = ids // HW
    kmin, kmax = np.where(valid, key, nkeys).min(axis=2), np.where(valid, key, -1).max(axis=2)
    assert (kmax[:-1] < kmin[1:]).all(), f'{tag}: the key ranges of two splits overlap or are out of order'
    # the ten best of the union == the reference's
    for r in range(HW):
        v, i = pval[:n, r][valid[:, r]], pidx[:n, r][valid[:, r]]
        assert len(np.unique(i)) == len(i), f'{tag}: query {r} lists an id twice'
        o = np.lexsort((i, -v))[:LP_K]
        m = min(LP_K, int(ref['ncand'][r]))
        assert len(o) >= m, f'{tag}: query {r}: {len(o)} candidates listed, {m} exist'
        want_i, want_v = ref['order'][r, :m], ref['top'][r, :m]
        assert np.array_equal(v[o][:m], want_v.astype(np.float32)), f'{tag}: query {r}: values {v[o][:m]} against {want_v}'
        got_i = canon[i[o][:m]] if ref['twins'] else i[o][:m]
        want_i = canon[want_i] if ref['twins'] else want_i
        assert np.array_equal(got_i, want_i), f'{tag}: query {r}: ids {got_i} against {want_i}'
    return n


@pytest.mark.parametrize('tag', list(LP_CASES))
def test_labelprop_exact(backend, tag):
    """partial lists and `out` of vfs_labelprop on exact operands (module docstring, 1.)"""
    H, W, C, radius, slots, qframe, T, topk, nml, (fs, temp) = LP_CASES[tag]
    assert lp_edge(tag), 'test bug: the case no longer reaches the edge it is there for'
    ref = lp_reference(tag)
    HW, nkeys, CO = H * W, len(slots), 3
    fb = as_bf16(ref['bank'])
    seg = torch.from_numpy(ref['seg'].copy())
    out = torch.full((HW, CO), float('nan'))
    ws = torch.full((LP_ROWS * HW * LP_K * 2,), -1, dtype=torch.int32).view(torch.float32)
    ks = (ctypes.c_int * nkeys)(*slots)
    backend.hostlib.labelprop(fb, seg, out, ws, ws.numel() * 4, qframe, ks, nkeys, H, W, C, CO, radius, nml, topk, temp, None)
    raw = ws.view(torch.int32).numpy()
    pval = raw[:LP_ROWS * HW * LP_K].view(np.float32).reshape(LP_ROWS, HW, LP_K)
    pidx = raw[LP_ROWS * HW * LP_K:].reshape(LP_ROWS, HW, LP_K)
    n = check_partial_lists(tag, ref, pval, pidx, HW, nkeys)
    got = out.numpy().astype(np.float64)
    assert not np.isnan(got).any(), f'{tag}: {int(np.isnan(got).sum())} elements of out were not written'
    frac = np.abs(got - ref['out']) / ref['bound']
    WORST[backend.name] = max(WORST.get(backend.name, 0.0), float(frac.max()))
    print(f'labelprop {tag}: {n} partial lists per query, candidates per query {int(ref["ncand"].min())}..{int(ref["ncand"].max())}, '
          f'|out - ref| / bound <= {frac.max():.3f} (largest so far on {backend.name}: {WORST[backend.name]:.3f})')
    r, c = np.unravel_index(np.argmax(frac), frac.shape)
    assert frac.max() <= 1.0, f'{tag}: out[{r}][{c}] = {got[r, c]!r} against {ref["out"][r, c]!r}: {frac.max():.1f} times the bound'


LP_OK = dict(qframe=2, nkeys=2, H=8, W=8, C=64, CO=2, radius=2, non_mask_len=0, topk=10, temperature=1.0)


@pytest.mark.parametrize('bad,code', [(dict(H=0), SHAPE_ERR), (dict(W=-1), SHAPE_ERR), (dict(C=0), SHAPE_ERR), (dict(CO=0), SHAPE_ERR),
                                      (dict(topk=0), SHAPE_ERR), (dict(topk=11), SHAPE_ERR), (dict(nkeys=0), SHAPE_ERR),
                                      (dict(nkeys=65), SHAPE_ERR), (dict(qframe=-1), ARG_ERR), (dict(kslot=[0, -1]), ARG_ERR),
                                      (dict(temperature=0.0), ARG_ERR), (dict(non_mask_len=2), ARG_ERR), (dict(C=72), SHAPE_ERR)])
def test_labelprop_refuses(backend, bad, code):
    """bad scalars are refused before anything is launched: the error code, and neither `out` nor the workspace is written.  Every
    buffer has the size of the good call."""
    dev = backend.dev
    a = dict(LP_OK, kslot=[0, 1])
    fb = torch.ones(3, 64, 64, dtype=BF16, device=dev)
    seg = torch.ones(3, 64, 2, device=dev)
    out = torch.full((64, 2), float('nan'), device=dev)
    ws = torch.full((LP_ROWS * 64 * LP_K * 2,), float('nan'), device=dev)
    a.update(bad)
    if 'topk' in bad:          # topk is refused before the workspace is looked at
        args_ws = (None, 0)
    else:
        args_ws = (ws, ws.numel() * 4)
    ks = (ctypes.c_int * 64)(*a['kslot'], *([0] * 62))
    rc, text = call_raw(backend, 'labelprop', (fb, seg, out, *args_ws, a['qframe'], ks, a['nkeys'], a['H'], a['W'], a['C'], a['CO'],
                                               a['radius'], a['non_mask_len'], a['topk'], a['temperature'], None))
    assert rc == code and text.startswith('labelprop: '), (rc, text)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all())


# ---------------------------------------------------------------------------------------------- 2. l2norm_rows
SENT16 = 0x7FC1        # a bf16 NaN with a payload: the pre-fill of y


def run_l2norm(be, x, P, C, spare=3):
    """x: bf16 [P][C] -> y bf16 [P][C]; `spare` rows behind y must keep the pre-fill"""
    y = torch.full((P + spare, C), SENT16, dtype=torch.int16).view(BF16)
    be.hostlib.l2norm_rows(x, y, P, C, None)
    tail = y[P:].view(torch.int16)
    assert bool((tail == SENT16).all()), f'l2norm P={P} C={C}: {int((tail != SENT16).sum())} elements of the rows past P were written'
    return y[:P]


def l2norm_rule(x, y, what):
    """the per-element rule of the module docstring (2., general regime) for bf16 tensors x, y [P][C] -> share of elements excused
    from round-to-nearest-even"""
    x64, y64 = x.float().numpy().astype(np.float64), y.float().numpy().astype(np.float64)
    C = x64.shape[1]
    assert np.isfinite(y64).all(), f'{what}: {int((~np.isfinite(y64)).sum())} outputs are not finite (or were never written)'
    norm = np.sqrt((x64 * x64).sum(axis=1, keepdims=True))
    ref = x64 / np.maximum(norm, float(np.float32(1e-12)))
    down, up, rne, mid = bf16_grid(ref)
    faithful = (y64 == down) | (y64 == up)
    if not faithful.all():
        r, c = np.argwhere(~faithful)[0]
        raise AssertionError(f'{what}: {int((~faithful).sum())} outputs are neither bf16 neighbour of the reference; first at row {r} channel '
                             f'{c}: {y64[r, c]!r} against {ref[r, c]!r}')
    excused = np.abs(ref - mid) <= (C + 8) * U * np.abs(ref)
    wrong = ~excused & (y64 != rne)
    if wrong.any():
        r, c = np.argwhere(wrong)[0]
        raise AssertionError(f'{what}: {int(wrong.sum())} outputs are not the nearest bf16 value; first at row {r} channel {c}: {y64[r, c]!r}, '
                             f'reference {ref[r, c]!r}, nearest {rne[r, c]!r}')
    return float(excused.mean())


L2_SHAPES = [(1, 8), (3, 64), (4, 504), (5, 512), (9, 520), (5, 1024), (3, 2048), (9, 64), (1, 2048)]


@pytest.mark.parametrize('P,C', L2_SHAPES)
def test_l2norm_exact_rows(backend, P, C):
    """rows of n entries +-2^a (n a power of 4), one zero row where P allows: every output by equality"""
    g = rng(2, P, C)
    ns = [n for n in (1, 4, 16, 64, 256) if n <= C]
    x = np.zeros((P, C))
    want = np.zeros((P, C))
    for r in range(P):
        if P >= 3 and r == 1:
            continue                                          # the zero row
        n = ns[::-1][r % len(ns)]
        a = int(g.integers(-20, 21))
        pos = np.arange(n) * C // n + (3 * r + np.arange(n)) % (C // n)
        sign = g.choice([-1.0, 1.0], n)
        x[r, pos] = sign * 2.0 ** a
        want[r, pos] = sign / np.sqrt(n)
    assert np.array_equal(want, bf16_grid(want)[2]), 'test bug: an expected output is not a bf16 value'
    lanes = {(c // 8 % 64, c // 512) for c in np.nonzero(np.abs(x).sum(axis=0))[0]}
    assert len(lanes) == C // 8, 'test bug: a lane or a pass of the channel loop holds no non-zero'
    y = run_l2norm(backend, as_bf16(x), P, C)
    got = y.float().numpy().astype(np.float64)
    bad = ~(got == want)
    assert not bad.any(), f'l2norm exact P={P} C={C}: {int(bad.sum())} differ; first (row, channel) {tuple(np.argwhere(bad)[0])}: {got[bad][0]!r} against {want[bad][0]!r}'
    if P >= 3:
        assert not np.signbit(got[1]).any() and (got[1] == 0).all()


@pytest.mark.parametrize('P,C', L2_SHAPES)
def test_l2norm_general_rows(backend, P, C):
    """random bf16 rows of norms 2^-20 .. 2^20 in one tensor: faithful everywhere, nearest outside the excused band"""
    g = rng(3, P, C)
    scale = 2.0 ** g.integers(-20, 21, (P, 1))
    scale[0], scale[-1] = 2.0 ** 20, 2.0 ** -20
    x = as_bf16(bf16_grid(g.standard_normal((P, C)) * scale)[2])
    y = run_l2norm(backend, x, P, C)
    x64 = x.float().numpy().astype(np.float64)
    ref = x64 / np.sqrt((x64 * x64).sum(axis=1, keepdims=True))
    share = float((np.abs(ref - bf16_grid(ref)[3]) <= (C + 8) * U * np.abs(ref)).mean())
    assert share < 0.10, f'test bug: {share} of the elements are excused'
    assert l2norm_rule(x, y, f'l2norm P={P} C={C}') == share
    print(f'l2norm P={P} C={C}: share excused from round-to-nearest {share:.4f}')


@pytest.mark.parametrize('P,C,code', [(0, 64, SHAPE_ERR), (-4, 64, SHAPE_ERR), (4, 0, SHAPE_ERR), (4, 12, SHAPE_ERR)])
def test_l2norm_refuses(backend, P, C, code):
    dev = backend.dev
    x = torch.ones(4, 64, dtype=BF16, device=dev)
    y = torch.full((4, 64), float('nan'), dtype=BF16, device=dev)
    rc, text = call_raw(backend, 'l2norm_rows', (x, y, P, C, None))
    assert rc == code and text.startswith('l2norm'), (rc, text)
    assert bool(torch.isnan(y.float()).all())


# ---------------------------------------------------------------------------------------------- 3. seg_postprocess
POST_BLOCKS = 64
EPS32 = np.float32(1e-12)


def bilerp64(seg, H, W, Ho, Wo):
    """seg [H*W][CO] -> [Ho][Wo][CO] float64: bilinear, align_corners=False (source coordinate clamped at 0, neighbour at the edge)"""
    s = np.asarray(seg, dtype=np.float64).reshape(H, W, -1)
    fy = np.maximum((np.arange(Ho) + 0.5) * (H / Ho) - 0.5, 0.0)
    fx = np.maximum((np.arange(Wo) + 0.5) * (W / Wo) - 0.5, 0.0)
    y0, x0 = np.floor(fy).astype(int), np.floor(fx).astype(int)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    ly, lx = (fy - y0)[:, None, None], (fx - x0)[None, :, None]
    top = (1 - lx) * s[y0][:, x0] + lx * s[y0][:, x1]
    bot = (1 - lx) * s[y1][:, x0] + lx * s[y1][:, x1]
    return (1 - ly) * top + ly * bot


def post_reference(seg, H, W, Ho, Wo):
    """-> (normalised [Ho][Wo][CO] float64, mn [CO], mx [CO], up).  The denominator is the fp32 value of mx - mn + 1e-12f."""
    up = bilerp64(seg, H, W, Ho, Wo)
    mn, mx = up.min(axis=(0, 1)), up.max(axis=(0, 1))
    den = (mx.astype(np.float32) - mn.astype(np.float32) + EPS32).astype(np.float64)
    return np.where(mx > 0, (up - mn) / den, up), mn, mx, up


def run_post(be, seg, H, W, CO, Ho, Wo):
    partial = torch.full((POST_BLOCKS * CO * 2,), float('nan'))
    lab = torch.full((Ho * Wo + 64,), 255, dtype=torch.uint8)
    be.hostlib.seg_postprocess(torch.from_numpy(np.ascontiguousarray(seg, dtype=np.float32)), partial, lab, H, W, CO, Ho, Wo, None)
    assert bool((lab[Ho * Wo:] == 255).all()), 'labels past Ho * Wo were written'
    return lab[:Ho * Wo].numpy().reshape(Ho, Wo), partial.numpy().reshape(POST_BLOCKS, CO, 2)


def exact_maps(kind, H, W, g):
    """integer-valued [H*W][CO] whose channels meet the preconditions of the exact regime"""
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]      # the only source pixels that an upscaled map reproduces as they are

    def spread(span, lo=0, inner_lo=None):
        """integers in [lo, lo + span], both ends present at two corners (so the upscaled map has the same range)"""
        m = g.integers(lo if inner_lo is None else inner_lo, lo + span + 1, (H, W)).astype(np.float64)
        a, b = g.permutation(4)[:2]
        m[corners[a]], m[corners[b]] = lo, lo + span
        return m
    if kind == 'ties':
        a, b = spread(16, 3), spread(8, -2)
        # channels 6 and 7 are equal on the first and last source row and column (3 and 19 in turn there) and 7 is one lower inside:
        # after the upscale they tie exactly where all four taps lie on the source border, and 7 is lower everywhere else
        e = spread(16, 3, inner_lo=4)
        ring = np.ones((H, W), dtype=bool)
        ring[1:-1, 1:-1] = False
        e[ring] = (3 + 16 * ((np.arange(H)[:, None] + np.arange(W)[None]) % 2 == 0))[ring]
        e[0, 0], e[0, W - 1] = 19, 3
        bord = np.where(ring, e, e - 1)
        chans = [b, a, a.copy(), -spread(4, 0), -spread(4, 1), np.full((H, W), 5.0), e, bord, a.copy()]
    elif kind == 'one':
        chans = [spread(32, -7)]
    elif kind == 'limit256':
        # channels 3 and 17 take two values only, so they reach 1 after normalisation (and win) at many pixels; their copies are channels 100 and 255
        base = [spread(1 if i in (3, 17) else 2 ** int(g.integers(1, 5)), int(g.integers(-3, 4))) for i in range(254)]
        chans = base[:100] + [base[17].copy()] + base[100:] + [base[3].copy()]
    else:
        raise KeyError(kind)
    return np.stack([c.reshape(-1) for c in chans], axis=1)


#               tag: (kind, H, W, Ho, Wo)
POST_EXACT = {'ties_x2': ('ties', 5, 7, 10, 14), 'ties_x4_x8': ('ties', 6, 5, 24, 40), 'ties_x8_x2': ('ties', 3, 9, 24, 18),
              'ties_small_output': ('ties', 3, 4, 6, 8), 'one_class': ('one', 4, 6, 16, 12), 'classes_256': ('limit256', 3, 5, 6, 20),
              'ties_x4_ragged_256': ('ties', 7, 11, 28, 44)}


@pytest.mark.parametrize('tag', list(POST_EXACT))
def test_seg_postprocess_exact(backend, tag):
    kind, H, W, Ho, Wo = POST_EXACT[tag]
    assert Ho // H in (2, 4, 8) and Wo // W in (2, 4, 8) and Ho % H == 0 and Wo % W == 0
    assert {'ties_small_output': Ho * Wo < 256, 'ties_x4_ragged_256': Ho * Wo % 256 != 0 and Ho * Wo > 256,
            'ties_x4_x8': Ho // H != Wo // W, 'ties_x8_x2': Ho // H != Wo // W}.get(tag, True)
    seg = exact_maps(kind, H, W, rng(4, list(POST_EXACT).index(tag)))
    CO = seg.shape[1]
    ref, mn, mx, up = post_reference(seg, H, W, Ho, Wo)
    # preconditions, on the reference alone
    assert np.array_equal(up, up.astype(np.float32)) and np.array_equal(ref, ref.astype(np.float32)), 'test bug: not exact in fp32'
    span = mx - mn
    norm = mx > 0
    pow2 = (span >= 1) & (np.frexp(np.where(span > 0, span, 1.0))[0] == 0.5)
    assert (pow2 | (span == 0) | ~norm).all(), 'test bug: max - min of a normalised channel is no power of two >= 1'
    den = (mx.astype(np.float32) - mn.astype(np.float32) + EPS32).astype(np.float64)
    assert (np.where(span > 0, den == span, den == float(EPS32)) | ~norm).all()
    want = ref.argmax(axis=2)
    if kind == 'ties':
        assert (mx[3] == 0) and (mx[4] < 0) and span[5] == 0 and mx[5] > 0
        assert not (want == 2).any() and not (want == 8).any() and (want == 1).any(), 'test bug: the identical channels never win'
        tie67 = ref[:, :, 6] == ref[:, :, 7]
        edge = np.zeros((Ho, Wo), dtype=bool)
        edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
        assert tie67[edge].all() and not tie67[Ho // H:-(Ho // H), Wo // W:-(Wo // W)].any(), 'test bug: channels 6 and 7 do not tie on the border only'
        assert (tie67 & (want == 6))[edge].sum() >= 4 and not (want == 7).any(), 'test bug: the border tie never decides a label'
    if kind == 'limit256':
        assert CO == 256 and (want == 3).any() and (want == 17).any() and not (want == 255).any() and not (want == 100).any()
    lab, partial = run_post(backend, seg, H, W, CO, Ho, Wo)
    assert not np.isnan(partial).any(), 'a min / max partial was not written'
    assert np.array_equal(partial[:, :, 0].min(axis=0), mn.astype(np.float32)), f'{tag}: per-channel minimum'
    assert np.array_equal(partial[:, :, 1].max(axis=0), mx.astype(np.float32)), f'{tag}: per-channel maximum'
    bad = lab != want
    on_edge = ''
    if bad.any():
        ys, xs = np.nonzero(bad)
        on_edge = 'all on the border' if ((ys == 0) | (ys == Ho - 1) | (xs == 0) | (xs == Wo - 1)).all() else 'not only on the border'
    assert not bad.any(), (f'{tag}: {int(bad.sum())} of {bad.size} labels differ ({on_edge}); first at {tuple(np.argwhere(bad)[0])}: '
                           f'{lab[bad][0]} against {want[bad][0]}')


def post_explained(seg, H, W, Ho, Wo, lab, what):
    """the rule of the module docstring (3., general regime): every label that is not the float64 argmax is explained by a near-tie
    -> (share of mismatches, share of near-ties in the reference)"""
    seg = np.asarray(seg, dtype=np.float64)
    ref, mn, mx, _ = post_reference(seg, H, W, Ho, Wo)
    R, Mx = seg.max(axis=0) - seg.min(axis=0), np.abs(seg).max(axis=0)
    e = U * (6 * max(H, W) * R + 6 * Mx)
    tol = np.where(mx > 0, 4 * e / np.maximum(mx - mn, 1e-300) + 3 * U, e)                  # per channel
    lab = np.asarray(lab).astype(int).reshape(Ho, Wo)
    best = ref.argmax(axis=2)
    bv = ref.max(axis=2)
    close = (bv[:, :, None] - ref) <= (np.take(tol, best)[:, :, None] + tol[None, None, :])
    close[np.arange(Ho)[:, None], np.arange(Wo)[None], best] = False
    near = close.any(axis=2)
    assert lab.max() < ref.shape[2], f'{what}: a label past the class count'
    got_close = np.take_along_axis(close, lab[:, :, None], axis=2)[:, :, 0]
    mism = lab != best
    unexplained = mism & ~got_close
    if unexplained.any():
        y, x = np.argwhere(unexplained)[0]
        raise AssertionError(f'{what}: {int(unexplained.sum())} of {int(mism.sum())} mismatching labels are no near-tie; first at ({y}, {x}): label '
                             f'{lab[y, x]} ({ref[y, x, lab[y, x]]!r}) against {best[y, x]} ({bv[y, x]!r}), allowed gap '
                             f'{tol[lab[y, x]] + tol[best[y, x]]!r}')
    assert mism.mean() <= near.mean()
    return float(mism.mean()), float(near.mean())


POST_GENERAL = {'up_7x9_23x31': (7, 9, 4, 23, 31), 'down_12x16_5x7': (12, 16, 5, 5, 7), 'davis_60x107_480x854': (60, 107, 4, 480, 854),
                'up_12x16_96x128': (12, 16, 4, 96, 128)}


@pytest.mark.parametrize('tag', list(POST_GENERAL))
def test_seg_postprocess_general(backend, tag):
    H, W, CO, Ho, Wo = POST_GENERAL[tag]
    g = rng(5, list(POST_GENERAL).index(tag))
    seg = g.random((H * W, CO)).astype(np.float32)
    seg[:, CO - 1] = -seg[:, CO - 1]                   # max <= 0: stays as it is
    seg[:, 0] = seg[:, 0] * 3 - 1
    lab, partial = run_post(backend, seg, H, W, CO, Ho, Wo)
    mism, near = post_explained(seg, H, W, Ho, Wo, lab, tag)
    print(f'seg_postprocess {tag}: labels off the float64 argmax {mism:.2e}, near-ties in the reference {near:.2e}')


@pytest.mark.parametrize('bad', [dict(H=0), dict(W=0), dict(Ho=0), dict(Wo=-2), dict(CO=0), dict(CO=257), dict(Ho=65536, Wo=32768)])
def test_seg_postprocess_refuses(backend, bad):
    dev = backend.dev
    a = dict(H=4, W=4, CO=2, Ho=8, Wo=8)
    a.update(bad)
    seg = torch.ones(16, 2, device=dev)
    partial = torch.full((POST_BLOCKS * 2 * 2,), float('nan'), device=dev)
    lab = torch.full((64,), 255, dtype=torch.uint8, device=dev)
    rc, text = call_raw(backend, 'seg_postprocess', (seg, partial, lab, a['H'], a['W'], a['CO'], a['Ho'], a['Wo'], None))
    assert rc == SHAPE_ERR and text.startswith('seg_postprocess: '), (rc, text)
    assert bool(torch.isnan(partial).all()) and bool((lab == 255).all())


# ---------------------------------------------------------------------------------------------- 4. onehot
@pytest.mark.parametrize('P,CO', [(1, 1), (255, 1), (85, 3), (256, 1), (257, 1), (1, 256), (3, 256), (86, 3), (1000, 3)])
def test_onehot(backend, P, CO):
    assert P * CO in (1, 255, 256, 257, 768, 258, 3000)
    g = rng(6, P, CO)
    lab = g.integers(0, CO, P).astype(np.uint8)
    lab[g.random(P) < 0.3] = 255                                     # the ignore value: a zero row unless CO = 256
    if P >= 3:
        lab[0], lab[P - 1], lab[1] = CO - 1, 0, min(CO, 255)
    want = (lab[:, None].astype(int) == np.arange(CO)[None]).astype(np.float32)
    assert CO == 256 or (want[lab >= CO] == 0).all()
    out = torch.full((P * CO + 300,), float('nan'))
    backend.hostlib.onehot(torch.from_numpy(lab), out, P, CO, None)
    assert bool(torch.isnan(out[P * CO:]).all()), 'elements past P * CO were written'
    assert np.array_equal(out[:P * CO].numpy().reshape(P, CO), want)


@pytest.mark.parametrize('P,CO', [(0, 3), (-1, 3), (8, 0), (8, 257), (2 ** 23, 256), (2 ** 31 - 1, 1)])
def test_onehot_refuses(backend, P, CO):
    dev = backend.dev
    lab = torch.zeros(8, dtype=torch.uint8, device=dev)
    out = torch.full((8 * 256,), float('nan'), device=dev)
    rc, text = call_raw(backend, 'onehot', (lab, out, P, CO, None))
    assert rc == SHAPE_ERR and text.startswith('onehot: '), (rc, text)
    assert bool(torch.isnan(out).all())
