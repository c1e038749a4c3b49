"""Exact-operand parity of the table-driven optimizer step (vfs_opt_step_table: opt_table_kernel / opt_update / the launcher of
vfs_amd/csrc/misc.hip, the segment map of vfs_amd/csrc/opt_table.h) at the C ABI against a float64 reference: SGD, Nesterov SGD,
Adam and AdamW over all param groups of the flat arena.  One step from the recipes below is compared for equality on every
stored word of p, state1 and state2; only the Adam steps after the first are bounded (listed at the end).

The reference evaluates the documented formulas of include/vfs_hip.h (the vfs_opt_step_table comment) per word in float64, from
the (begin, end, group) triples and the group rows:
    SGD:   g' = clip g + wd p;  buf = momentum buf + g';  p -= lr (nesterov ? g' + momentum buf : buf)
    Adam:  g' = clip g + wd p;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;
           p -= lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    AdamW: p *= 1 - lr wd first, g' = clip g
It calls no kernel of the project and never vfs_opt_segment_map: the map under test is the library's, and its contents are
compared with the definition of opt_table.h in a test of their own.

Operand recipes.  Each case asserts with `fp32_exact` that every intermediate of its reference round-trips through fp32; the only
correct stored value is then the float64 one, whatever the contraction (the argument of the streaming-kernel section of
tests/test_loss_exact.py).

  SGD and Nesterov SGD.  p, g and buf are small integers that depend on the word index: an element updated twice, not at all or
        from a neighbouring word shows.  Each group's lr, momentum and wd come from {1/2, 1/4, 1/8, 0}, every group another triple
        (Nesterov: momentum > 0, as the entry point demands; the triples with lr = 0 come last).  The clip coefficient is 1/2, a
        device float written by the test.  |p|, |g|, |buf| <= 15: g' is a multiple of 1/8, buf of 1/8, the Nesterov term
        g' + momentum buf' of 1/64, the update of 1/512, and everything stays below 2^5: 14 bits.

  Adam and AdamW, step = 1 (the recipe of tests/test_siamfc_exact.py:test_adam_first_step_exact, extended so that the state is
        read).  b1 = 1/2, b2 = 3/4; each group its own lr in {2^-2, 2^-3, 2^-4}, eps = 2^k with k in {-3, 0, 5} and wd in
        {0, 1/4} (18 rows; group G takes row G mod 18, neighbours differ in all three).  Per word (a, b) is drawn by the index from
        {(+-3, 0), (+-3/2, 9), (0, 12)}: the effective gradient is g' = a 2^k, v0 = b 4^(k-1), so v = 3/4 v0 + 1/4 g'^2 =
        9 4^(k-1) for every entry, sqrt(v) = 3 2^(k-1), bc2s = 1/2, the denominator 4 2^k - a power of two.  m0 is an
        index-dependent multiple of 2^(k-2), bc1 = 1/2 and lr / bc1 a power of two: p, m and v are single correct fp32 values, a
        kernel that ignores m0 or v0 or takes another group's eps, lr or wd fails.  p is a multiple of 1/8, |p| <= 8.  Adam: the
        stored g is (g' - wd p) / clip; AdamW: g' / clip and p (1 - lr wd) is exact.  This needs powf(b, 1.0f) == b in the launcher.

  Group-row transport (224, 225, 448 groups, every row distinct) needs more rows than those menus hold: the same recipes with
        further powers of two - SGD: the 448 triples (lr, momentum, wd) = (2^-a, 2^-b, 2^-c or 0), a, b, c <= 8, with the fewest
        fraction bits a + b + max(b, c) in the update (18 at the most, on values below 2^5); Adam / AdamW: lr = 2^-1 .. 2^-8,
        k = -3 .. 5, wd in {0, 2^-1 .. 2^-6}.  The same `fp32_exact` assertions hold them to the argument above.

Arena.  Every word of p, state1 and state2 outside every segment - frozen parameters, the padding up to 4 words, the 256 guard
words behind n - holds NaN and must keep its bit pattern; so does the whole of g, whose words outside the segments are NaN as
well (a gradient read from there poisons the result).  The device table is pre-filled with NaN and the unused slots of the host
rows with 77: a row that is never written, or a slot that is not ignored, shows.

Layouts (segments in words; C = VFS_OPT_CHUNK_WORDS read from opt_table.h) and the branch of opt_table_kernel each reaches:
  small_segments_one_chunk      1, 2, 3, 4, 5 words in five groups: the per-lane walk, several steps per lane, tails 1, 2, 3, 0, 1
  mid_chunk_over_whole_chunks   begins mid-chunk, three whole chunks, ends mid-chunk with a 1-word tail, frozen words and a small
                                segment of another group on either side: the walk in both edge chunks, the uniform path between
  chunk_edge_to_chunk_edge      [C, 2C) and a neighbour of another group from 2C: the uniform path at `begin4 == base` and
                                `base + 256 == end4`; chunk 0 is frozen in front of segment 0 (`begin4 > i`)
  ends_in_last_vector           a segment whose 1-word tail lies in the last vector of its chunk, and one that ends on the vector
                                before the edge with a neighbour in that last vector: `base + 256 <= end4` is false by one, the walk
  two_frozen_chunks_between     two trainable segments, two wholly frozen chunks between them: first[] of a frozen chunk
  frozen_to_the_end             frozen from mid-chunk over two more chunks to the end: the early `s0 == nseg` exit
  frozen_to_the_end_partial     the same with n % 4 = 3: the last vector of the arena is partial and frozen
  forty_groups_two_chunks       forty 5-word parameters, a group each, across a chunk edge: the lane's group is its own segment's
  second_grid_pass              starts mid-chunk, ends five words past one pass of the grid (4096 workgroups x 256 lanes x 4
                                words): the stride loop's second trip, on a chunk with an edge; once per kind, no clip

Bounded quantities (everything else is equality): Adam and AdamW at step 2 and 7, m, v and the update p_after - p_before,
against the float64 formula from the state the kernel stored before the step, to exactly the bounds derived in the docstring of
tests/test_siamfc_exact.py ("Adam, steps 2 to 4": u (|b1 m0| + |(1 - b1) g'| + |m64|), u (|b2 v0| + 2 (1 - b2) g'^2 + |v64|),
u (2 c1 + c2 + 9.5) |U64| + u |p0 - U64|, c = b^t / (1 - b^t), all times 1.001).  The table kernel uses adam_kernel's expressions
and the launcher forms the bias corrections as vfs_adam_launch does, so the derivation carries over for any b1, b2 in [1/2, 1].
It has no weight-decay term, so the operands keep that step exact: group 0 has wd = 0 and runs on from its own p; group 1
(lr = 2^-3, wd = 1/4) gets p in eighths up to 1 and g in multiples of 2^-10 before every step, so that g' = clip g + wd p and
p (1 - lr wd) are fp32 values (asserted) and stand for g and p0 in the bounds.

Every case takes well under a second on the emulator but second_grid_pass (4 M words, as tests/test_optim_table.py's 'pass+5').
backend=emu: host build through the fiber emulator; backend=gpu: libvfs_hip.so on the MI355X."""
import os
import re

import numpy as np
import pytest
import torch

from tests.test_bn_exact import fp32_exact
from tests.test_conv_exact import assert_bits, nan_like
from tests.test_loss_exact import assert_exact
from tests.test_siamfc_exact import all_nan, guarded

F32 = torch.float32
F64 = torch.float64
I32 = torch.int32
CPU = torch.device('cpu')
U = 2.0 ** -24
SGD, ADAM, ADAMW = 0, 1, 2
#        tag: (kind, nesterov)
KINDS = {'sgd': (SGD, 0), 'nesterov': (SGD, 1), 'adam': (ADAM, 0), 'adamw': (ADAMW, 0)}
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    with open(os.path.join(REPO, 'vfs_amd', 'csrc', 'opt_table.h')) as f:
        return int(re.search(r'^#define\s+' + name + r'\s+(\d+)', f.read(), re.M).group(1))


C = header_constant('VFS_OPT_CHUNK_WORDS')
HYPER = header_constant('VFS_OPT_HYPER')
BY_VALUE = header_constant('VFS_OPT_WRITE_GROUPS')
GRID_PASS = 4096 * 256 * 4      # words one pass of the update launch's capped grid covers


# ---------------------------------------------------------------------------------------------- layouts
def layouts():
    """tag -> (n, [(begin, end, group), ...]); the branch each one reaches is in the module docstring"""
    assert C % 64 == 0 and C >= 512
    return {
        # one chunk, walk only: 1, 2, 3, 4, 5 words, tails 1, 2, 3, 0, 1; vector 0 frozen; (16, 20) and (20, 25) touch
        'small_segments_one_chunk': (C, [(4, 5, 0), (8, 10, 1), (12, 15, 2), (16, 20, 3), (20, 25, 4)]),
        # walk in chunks 0 and 4 (frozen words and a small segment of another group on either side), uniform path in 1, 2, 3
        'mid_chunk_over_whole_chunks': (5 * C, [(8, 14, 1), (C // 2 + 8, 4 * C + 149, 0), (4 * C + 160, 4 * C + 163, 2)]),
        # uniform path with begin4 == base and base + 256 == end4; chunk 0: begin4 > i; chunk 2: walk from a neighbour on the edge
        'chunk_edge_to_chunk_edge': (3 * C, [(C, 2 * C, 0), (2 * C, 2 * C + 9, 1)]),
        # chunk 1: 255 whole vectors and a 1-word tail in the last one; chunk 2: 255 whole vectors, the last vector another group's
        'ends_in_last_vector': (3 * C, [(C, 2 * C - 3, 0), (2 * C, 3 * C - 4, 1), (3 * C - 4, 3 * C - 1, 2)]),
        # chunks 1 and 2 hold nothing: their first[] entry is segment 1, whose begin4 lies behind every lane
        'two_frozen_chunks_between': (4 * C, [(4, C // 2 + 3, 0), (3 * C + 8, 3 * C + 21, 1)]),
        # chunk 0 walks off the end of the map (s == nseg), chunks 1 and 2 leave at s0 == nseg
        'frozen_to_the_end': (3 * C, [(0, 6, 0), (8, C // 2 + 2, 1)]),
        'frozen_to_the_end_partial': (2 * C + 39, [(0, 6, 0), (8, C // 2 + 2, 1)]),
        # twenty parameters on either side of the edge C: up to twenty walk steps, the row is that of the lane's own segment
        'forty_groups_two_chunks': (2 * C, [(C - 160 + 8 * k, C - 160 + 8 * k + 5, k) for k in range(40)]),
    }


def second_grid_pass():
    # 4097 chunks on 4096 workgroups: workgroup 0 comes back for the last chunk, which holds the segment's end and its 1-word tail
    return GRID_PASS + 5, [(8, 11, 1), (C // 2 + 4, GRID_PASS + 5, 0)]


def group_of(segs, n):
    """[n] the group of every word, -1 outside every segment"""
    grp = torch.full((n,), -1, dtype=torch.int64)
    for b, e, k in segs:
        assert bool((grp[b:e] == -1).all())
        grp[b:e] = k
    return grp


# ---------------------------------------------------------------------------------------------- group rows
HALVES = (0.5, 0.25, 0.125, 0.0)


def sgd_rows(ngroups, nesterov):
    """(lr, wd, momentum) from {1/2, 1/4, 1/8, 0}, every group another triple, lr changing fastest, lr = 0 last"""
    moms = HALVES[:3] if nesterov else HALVES
    rows = [(lr, wd, mom) for mom in moms for wd in HALVES for lr in HALVES[:3]] + [(0.0, wd, mom) for mom in moms for wd in HALVES]
    assert ngroups <= len(rows) == len(set(rows))
    return rows[:ngroups]


def adam_rows(ngroups):
    """(lr, wd, b1, b2, eps): group G takes row G mod 18 of {2^-2, 2^-3, 2^-4} x {1/4, 0} x 2^{-3, 0, 5}; G mod 6 fixes (lr, wd), and
    (G // 6 + G) mod 3 the exponent of eps - a bijection on 0 .. 17 in which neighbouring groups differ in all three"""
    rows = [(2.0 ** -(2 + G % 3), (0.25, 0.0)[G % 2], 0.5, 0.75, 2.0 ** (-3, 0, 5)[(G // 6 + G) % 3]) for G in range(ngroups)]
    assert len(set(rows[:18])) == min(ngroups, 18)
    return rows


def sgd_rows_wide(ngroups):
    """the transport test's distinct triples: (2^-a, 2^-c or 0, 2^-b) with the fewest fraction bits in the update"""
    cand = sorted((a + b + max(b, c, 1), a, b, c) for a in range(1, 9) for b in range(1, 9) for c in range(0, 9))
    rows = [(2.0 ** -a, 2.0 ** -c if c else 0.0, 2.0 ** -b) for _, a, b, c in cand[:ngroups]]
    assert len(set(rows)) == ngroups
    return rows


def adam_rows_wide(ngroups):
    rows = [(2.0 ** -a, wd, 0.5, 0.75, 2.0 ** k) for wd in [0.0] + [2.0 ** -c for c in range(1, 7)] for k in range(-3, 6) for a in range(1, 9)]
    assert ngroups <= len(rows) == len(set(rows))
    return rows[:ngroups]


def rows_for(tag, ngroups, wide=False):
    if KINDS[tag][0] == SGD:
        return sgd_rows_wide(ngroups) if wide else sgd_rows(ngroups, KINDS[tag][1])
    return adam_rows_wide(ngroups) if wide else adam_rows(ngroups)


# ---------------------------------------------------------------------------------------------- operands
def arena(values64, grp):
    """float64 [n] -> the fp32 arena: the values inside the segments, NaN outside and in the guard"""
    live = grp >= 0
    fp32_exact(operand=values64[live])
    return guarded(torch.where(live, values64, torch.full_like(values64, float('nan'))))


def by_index(n, mul, mod):
    """integers in [-mod / 2, mod / 2] that depend on the index"""
    return ((torch.arange(n, dtype=torch.int64) * mul) % mod - mod // 2).double()


ADAM_MENU = torch.tensor([(3.0, 0.0), (-3.0, 0.0), (1.5, 9.0), (-1.5, 9.0), (0.0, 12.0)], dtype=F64)      # (a, b)


def operands(tag, grp, rows, c):
    """p, g, state1, state2 of the recipe as guarded fp32 arenas (state2: None for SGD); c: the clip coefficient (1: no clip)"""
    kind, _ = KINDS[tag]
    n = grp.numel()
    if kind == SGD:
        return arena(by_index(n, 7, 31), grp), arena(by_index(n, 13, 29), grp), arena(by_index(n, 29, 27), grp), None      # |.| <= 15, 14, 13
    i = torch.arange(n, dtype=torch.int64)
    R = torch.tensor(rows, dtype=F64)[grp.clamp_min(0)]
    wd, k = R[:, 1], torch.log2(R[:, 4])
    assert torch.equal(k, k.round())
    ab = ADAM_MENU[(i * 3 + i // 5) % 5]
    geff = ab[:, 0] * 2.0 ** k
    v0 = ab[:, 1] * 4.0 ** (k - 1)
    m0 = by_index(n, 11, 17) * 2.0 ** (k - 2)
    p0 = by_index(n, 7, 129) / 8
    g0 = ((geff - wd * p0) if kind == ADAM else geff) / c
    return arena(p0, grp), arena(g0, grp), arena(m0, grp), arena(v0, grp)


# ---------------------------------------------------------------------------------------------- the float64 reference
def reference(tag, grp, rows, p, g, s1, s2, c, step):
    """the documented formulas per word -> (p, state1, state2) [n] float64 (the input outside the segments), and every
    intermediate on the words inside them"""
    kind, nesterov = KINDS[tag]
    n, live = grp.numel(), grp >= 0
    R = torch.tensor(rows, dtype=F64)[grp.clamp_min(0)]
    lr, wd = R[:, 0], R[:, 1]
    p0, g0, a0 = p[:n].double(), g[:n].double(), s1[:n].double()
    gc = g0 * c
    if kind == SGD:
        mom = R[:, 2]
        wdp = wd * p0
        ge = gc + wdp
        ma = mom * a0
        a1 = ma + ge
        mb = mom * a1
        d = ge + mb if nesterov else a1
        upd = lr * d
        p1, b1 = p0 - upd, None
        inter = dict(clipped=gc, wd_p=wdp, g_eff=ge, mom_buf=ma, buf=a1, mom_buf_new=mb, direction=d, update=upd, p=p1)
    else:
        be1, be2, eps = R[:, 2], R[:, 3], R[:, 4]
        b0 = s2[:n].double()
        bc1, bc2s = 1 - be1 ** step, (1 - be2 ** step).sqrt()
        keep = 1 - lr * wd if kind == ADAMW else torch.ones_like(lr)
        pd = p0 * keep
        wdp = wd * p0 if kind == ADAM else torch.zeros_like(p0)
        ge = gc + wdp
        m_old, m_new = be1 * a0, (1 - be1) * ge
        a1 = m_old + m_new
        g2s = (1 - be2) * ge
        v_old, v_new = be2 * b0, g2s * ge
        b1 = v_old + v_new
        root = b1.sqrt()
        over = root / bc2s
        den = over + eps
        quot = a1 / den
        rate = lr / bc1
        upd = rate * quot
        p1 = pd - upd
        inter = dict(clipped=gc, wd_p=wdp, g_eff=ge, keep=keep, p_decayed=pd, b1_m=m_old, g_share=m_new, m=a1, g_scaled=g2s, b2_v=v_old,
                     g2_share=v_new, v=b1, root=root, over_bc2s=over, den=den, quot=quot, bc1=bc1, bc2s=bc2s, rate=rate, update=upd, p=p1)
    inter = {name: v[live] for name, v in inter.items()}
    out = [torch.where(live, new, old) for new, old in ((p1, p0), (a1, a0))]
    return out[0], out[1], (torch.where(live, b1, s2[:n].double()) if kind != SGD else None), inter


# ---------------------------------------------------------------------------------------------- launch and compare
def segment_map(lib, segs, n, ngroups):
    """host: the library's map of the segments of an arena of n words"""
    words = torch.zeros(1, dtype=torch.int64)
    lib.opt_segment_map_words(n, len(segs), words)
    m = torch.zeros(max(int(words), 4), dtype=I32)
    lib.opt_segment_map(torch.tensor(segs, dtype=torch.int64).reshape(-1, 3), len(segs), n, ngroups, m, m.numel())
    return m, int(words)


def table_step(backend, tag, p, g, s1, s2, n, segs, rows, step=1, clip=None, skip=None):
    """one vfs_opt_step_table launch on host tensors of n live words (the guard behind them is not part of the arena)"""
    kind, nesterov = KINDS[tag]
    m, _ = segment_map(backend.lib, segs, n, len(rows))
    hyper = torch.full((len(rows), HYPER), 77.0)      # hyper stays host memory on both backends: its address goes in as an integer
    hyper[:, :len(rows[0])] = torch.tensor(rows, dtype=F32)
    assert torch.equal(hyper[:, :len(rows[0])].double(), torch.tensor(rows, dtype=F64)), 'test bug: a group value is not an fp32 value'
    table = nan_like((len(rows) * HYPER,), CPU, F32)
    backend.hostlib.opt_step_table(kind, p, g, s1, s2, n, m, len(segs), hyper.data_ptr(), len(rows), table, nesterov, step, clip, skip, None)


def bits(t):
    return t.contiguous().view(I32)


def assert_untouched(got, before, live, what):
    """every word outside the segments, the guard included, keeps its bit pattern (they are all NaN)"""
    dead = ~torch.cat([live, torch.zeros(got.numel() - live.numel(), dtype=torch.bool)])
    assert all_nan(before[dead]), 'test bug: a word outside the segments is not NaN'
    assert_bits(bits(got)[dead], bits(before)[dead], what + ': the bit patterns of the words outside every segment (index among those words)', pixels=False)


def assert_words(got, before, want64, live, what):
    """inside the segments the float64 value, outside the bit pattern from before"""
    n = live.numel()
    fp32_exact(**{what: want64[live]})
    zero = torch.zeros(n)
    assert_exact(torch.where(live, got[:n], zero), torch.where(live, want64.float(), zero), what, ('word',))
    assert_untouched(got, before, live, what)


def run_exact(backend, tag, n, segs, rows, clip):
    grp = group_of(segs, n)
    live = grp >= 0
    c = 0.5 if clip else 1.0
    p, g, s1, s2 = operands(tag, grp, rows, c)
    p64, a64, b64, inter = reference(tag, grp, rows, p, g, s1, s2, c, 1)
    fp32_exact(**inter)
    before = [t.clone() if t is not None else None for t in (p, g, s1, s2)]
    table_step(backend, tag, p, g, s1, s2, n, segs, rows, clip=torch.tensor([c]) if clip else None)
    what = f'{tag}{" clip" if clip else ""}, {len(segs)} segments, {len(rows)} groups: '
    assert_words(s1, before[2], a64, live, what + 'state1')
    if s2 is not None:
        assert_words(s2, before[3], b64, live, what + 'state2')
    assert_words(p, before[0], p64, live, what + 'p')
    assert torch.equal(bits(g), bits(before[1])), what + 'g (an input) changed'
    moved = (p[:n][live] != before[0][:n][live]).double().mean()
    assert float(moved) > 0.5, 'test bug: the step leaves most parameters where they were'


# ---------------------------------------------------------------------------------------------- 1. the segment map
@pytest.mark.parametrize('layout', list(layouts()) + ['second_grid_pass'])
def test_segment_map_is_the_documented_one(backend, layout):
    """opt_table.h: per segment {begin / 4, end / 4, group, end % 4}, then per chunk the first segment that ends behind the chunk's
    first word (nseg where none does) - for a wholly frozen chunk the NEXT segment, so that a lane never walks over segments of
    earlier chunks"""
    n, segs = second_grid_pass() if layout == 'second_grid_pass' else layouts()[layout]
    ngroups = max(k for _, _, k in segs) + 1
    m, words = segment_map(backend.lib, segs, n, ngroups)
    nchunks = (n + C - 1) // C
    assert words == 4 * len(segs) + nchunks
    want = [v for b, e, k in segs for v in (b // 4, e // 4, k, e % 4)]
    want += [next((s for s, (_, e, _) in enumerate(segs) if e > chunk * C), len(segs)) for chunk in range(nchunks)]
    assert_bits(m[:words], torch.tensor(want, dtype=I32), f'segment map of {layout}', pixels=False)


# ---------------------------------------------------------------------------------------------- 2. one exact step on every layout
@pytest.mark.parametrize('clip', [False, True])
@pytest.mark.parametrize('layout', list(layouts()))
@pytest.mark.parametrize('tag', list(KINDS))
def test_one_step_exact(backend, tag, layout, clip):
    n, segs = layouts()[layout]
    ngroups = max(k for _, _, k in segs) + 1
    run_exact(backend, tag, n, segs, rows_for(tag, ngroups), clip)


@pytest.mark.parametrize('tag', list(KINDS))
def test_second_grid_pass_exact(backend, tag):
    n, segs = second_grid_pass()
    run_exact(backend, tag, n, segs, rows_for(tag, 2), False)


# ---------------------------------------------------------------------------------------------- 3. group-row transport
@pytest.mark.parametrize('ngroups', [BY_VALUE, BY_VALUE + 1, 2 * BY_VALUE])
@pytest.mark.parametrize('tag', ['nesterov', 'adam', 'adamw'])
def test_group_rows_by_value_and_through_the_table(backend, tag, ngroups):
    """up to VFS_OPT_WRITE_GROUPS groups the rows are kernel arguments, more go through the device table in launches of that many:
    one 5-word parameter per group, every row distinct, EVERY parameter against the float64 reference - the bias corrections
    (slots 5 and 6) included, which the launcher adds to each row"""
    segs = [(8 * k, 8 * k + 5, k) for k in range(ngroups)]
    run_exact(backend, tag, 8 * ngroups, segs, rows_for(tag, ngroups, wide=True), True)


# ---------------------------------------------------------------------------------------------- 4. skip word, repeatability
@pytest.mark.parametrize('tag', list(KINDS))
def test_skip_word_keeps_every_bit(backend, tag):
    n, segs = layouts()['mid_chunk_over_whole_chunks']
    grp = group_of(segs, n)
    rows = rows_for(tag, 3)
    arenas = operands(tag, grp, rows, 0.5)
    before = [t.clone() if t is not None else None for t in arenas]
    table_step(backend, tag, *arenas, n, segs, rows, clip=torch.tensor([0.5]), skip=torch.tensor([1 << 40], dtype=torch.int64))
    for name, t, t0 in zip(('p', 'g', 'state1', 'state2'), arenas, before):
        assert t is None or torch.equal(bits(t), bits(t0)), f'{tag}: a step with the skip word set changed {name}'


@pytest.mark.parametrize('tag', list(KINDS))
def test_a_second_run_gives_the_same_bits(backend, tag):
    n, segs = layouts()['mid_chunk_over_whole_chunks']
    grp = group_of(segs, n)
    rows = rows_for(tag, 3)
    runs = []
    for _ in range(2):
        arenas = operands(tag, grp, rows, 0.5)
        start = arenas[0].clone()
        table_step(backend, tag, *arenas, n, segs, rows, clip=torch.tensor([0.5]), skip=torch.zeros(1, dtype=torch.int64))
        assert not torch.equal(bits(arenas[0]), bits(start)), 'a zero skip word must let the step through'
        runs.append(arenas)
    for name, t, t2 in zip(('p', 'g', 'state1', 'state2'), *runs):
        assert t is None or torch.equal(bits(t), bits(t2)), f'{tag}: two runs from the same inputs differ in {name}'


# ---------------------------------------------------------------------------------------------- 5. later Adam steps: the bounds
LATER_N = 3 * C
LATER_SEGS = [(4, 261, 0), (C - 8, 2 * C + 10, 1)]      # group 0: walk, 1-word tail; group 1: walk, a uniform chunk, walk, 2-word tail


@pytest.mark.parametrize('clip', [False, True])
@pytest.mark.parametrize('tag', ['adam', 'adamw'])
def test_later_steps_bound(backend, tag, clip):
    """steps 1 to 7 with fresh gradients; at steps 2 and 7 m, v and the update against the float64 formula from the state stored
    before the step, to the bounds of tests/test_siamfc_exact.py's docstring (module docstring: what stands for g and p0)"""
    kind, _ = KINDS[tag]
    f = lambda a: float(np.float32(a))      # noqa: E731  the rows are floats
    rows = [(f(1e-3), 0.0, f(0.9), f(0.999), f(1e-8)), (2.0 ** -3, 0.25, f(0.8), f(0.99), f(1e-6))]
    n, segs = LATER_N, LATER_SEGS
    grp = group_of(segs, n)
    live, second = grp >= 0, grp == 1
    nan = torch.full((n,), float('nan'), dtype=F64)
    R = torch.tensor(rows, dtype=F64)[grp.clamp_min(0)]
    lr, wd, b1, b2, eps = R.unbind(1)
    c = 0.5 if clip else 1.0
    gen = torch.Generator().manual_seed(41)
    p = guarded(torch.where(live, torch.randn(n, generator=gen).double() * 0.01, nan))
    m, v = arena(torch.zeros(n, dtype=F64), grp), arena(torch.zeros(n, dtype=F64), grp)
    eighths = by_index(n, 7, 17) / 8
    worst = dict(m=0.0, v=0.0, update=0.0)
    for t in range(1, 8):
        p[:n][second] = eighths[second].float()
        g64 = torch.where(second, torch.randint(-1024, 1025, (n,), generator=gen).double() / 1024, torch.randn(n, generator=gen).double())
        gr = arena(g64.float().double(), grp)
        before = [x.clone() for x in (p, gr, m, v)]
        p0, m0, v0, g = p[:n].double(), m[:n].double(), v[:n].double(), gr[:n].double() * c
        table_step(backend, tag, p, gr, m, v, n, segs, rows, step=t, clip=torch.tensor([c]) if clip else None)
        for name, x, x0 in zip(('p', 'g', 'm', 'v'), (p, gr, m, v), before):
            assert_untouched(x, x0, live, f'{tag} step {t}: {name}')
        assert torch.equal(bits(gr), bits(before[1]))
        if t not in (2, 7):
            continue
        ge = g + wd * p0 if kind == ADAM else g
        pd = p0 * (1 - lr * wd) if kind == ADAMW else p0
        fp32_exact(g_eff=ge[live], p_decayed=pd[live])
        m64 = b1 * m0 + (1 - b1) * ge
        v64 = b2 * v0 + (1 - b2) * ge * ge
        bound_m = 1.001 * U * ((b1 * m0).abs() + ((1 - b1) * ge).abs() + m64.abs())
        bound_v = 1.001 * U * (b2 * v0 + 2 * (1 - b2) * ge * ge + v64)
        ms, vs = m[:n].double(), v[:n].double()                      # the stored state: what the update is formed from
        u64 = lr / (1 - b1 ** t) * ms / (vs.sqrt() / (1 - b2 ** t).sqrt() + eps)
        c1, c2 = b1 ** t / (1 - b1 ** t), b2 ** t / (1 - b2 ** t)
        bound_u = 1.001 * (U * (2 * c1 + c2 + 9.5) * u64.abs() + U * (pd - u64).abs())
        for name, err, bound in (('m', (ms - m64).abs(), bound_m), ('v', (vs - v64).abs(), bound_v),
                                 ('update', ((p[:n].double() - pd) + u64).abs(), bound_u)):
            for G in (0, 1):
                sel = grp == G
                frac = float((err[sel] / bound[sel].clamp_min(1e-300)).max())
                worst[name] = max(worst[name], frac)
                assert bool((err[sel] <= bound[sel]).all()), f'{tag} step {t}, group {G}: {name} is off by up to {frac} of the bound'
        assert float((u64[live].abs() > 0).double().mean()) > 0.9, 'test bug: hardly any update to compare'
    print(f'{tag}{" clip" if clip else ""}, steps 2 and 7: worst error / bound m {worst["m"]:.3f}, v {worst["v"]:.3f}, update {worst["update"]:.3f}')
