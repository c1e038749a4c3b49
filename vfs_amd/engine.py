"""Host-side executor: sequences the libvfs_hip.so kernels for ResNet / SimSiam-head forward
and backward over NHWC bf16 buffers.  PyTorch supplies device memory (torch.empty), streams and
torch.distributed; every number on the path is produced by the HIP kernels.

Layout of one "unit" (mmcv ConvModule = conv -> BN -> act in the reference):
    raw = conv(a_prev)                 bf16, BatchNorm partial statistics from the GEMM epilogue
    bnp = finalize(statistics)         float[G][4][C]   (G independent BN batches = views)
    act = relu(raw*scale+shift [+res]) bf16
Backward of a unit: bn_bwd_reduce -> (all-reduce) -> bn_bwd_apply -> wgrad (+dgrad).
"""
import math
from typing import NamedTuple, Optional

import torch
import torch.distributed as dist

from . import knobs
from ._lib import Tape, TapeLib, get_lib
from .packing import bn_fold_eligible, build_pack_table, build_reduce_table, conv_plan, stem_stats_rows, wgrad_halo_eligible, wgrad_splits

BF16 = torch.bfloat16


def side_stream_on(dev):
    """do the weight gradients (data parallel: and the gradient buckets behind them) get a stream of their own on `dev`?"""
    return dev.type == 'cuda' and knobs.flag('VFS_SIDE_STREAM')


class ConvUnit:
    """Host state of one conv / linear layer (+ its BatchNorm)."""

    def __init__(self, name, weight, bias, bn, k, stride, pad, kind='conv', dil=1):
        self.name, self.weight, self.bias, self.bn = name, weight, bias, bn
        self.k, self.stride, self.pad, self.kind, self.dil = k, stride, pad, kind, dil
        self.cout, self.cin = weight.shape[0], weight.shape[1]
        self.wf = self.wd = None
        self.bnp = self.sums = self.bsums = None
        self.need_wd = True
        self.relu = False        # head units: the fused Linear + BatchNorm1d + ReLU launch applies the activation itself
        self.true_w = None       # stem: image width without the NHWC4 row padding
        self.mask_bits = None    # bit-packed ReLU mask of the last bn_act(want_mask=True), None when it wrote none
        self.nbt_pending = 0     # BatchNorm.num_batches_tracked increments not yet materialised (Engine.flush_counters)

    def out_hw(self, H, W):
        span = self.dil * (self.k - 1) + 1
        return (H + 2 * self.pad - span) // self.stride + 1, (W + 2 * self.pad - span) // self.stride + 1


class FinRows(NamedTuple):
    """conv_fwd -> bn_act: BatchNorm statistics that the apply launch finishes in its prologue"""
    rows: Optional[torch.Tensor]      # float[G][nrows][2][C] partial sums; None: u.sums already holds the sums over the ranks
    nrows: int                        # rows per group
    count: float                      # elements per channel behind one group's statistics (all ranks)
    xchg: object = None               # SyncBN: the P2PExchange whose window exchange runs inside the same launch


class FusedAct(NamedTuple):
    """conv_fwd -> bn_act: the activation, already produced by the fused Linear + BatchNorm1d + ReLU launch"""
    act: torch.Tensor


class BwdRows(NamedTuple):
    """conv_bwd -> bn_bwd: the BatchNorm-backward statistics rows of `unit` that the dgrad epilogue emitted"""
    unit: ConvUnit
    rows: torch.Tensor
    nrows: int                        # rows of all groups together


class NCHWGrad(NamedTuple):
    """a gradient as the caller's autograd holds it - fp32 [N, C, h, w] (or [N, C]) - where backward_nhwc takes bf16 NHWC: it is
    converted (vfs_nchw_f32_to_nhwc_bf16) or joined (vfs_nchw_f32_add_nhwc_bf16) by Engine.grad_join"""
    t: torch.Tensor


class Engine:
    def __init__(self, lib=None):
        self.lib = lib if lib is not None else get_lib()
        self._real_lib = None     # the library itself while self.lib records onto a tape
        self.bufs = {}
        self.units = []
        self._pack = None
        self._pack_key = None
        self.process_group = None
        self._side = {}
        self._side_dirty = False
        self.prof = None     # list collecting (kind, flops, start_event, end_event) when profiling
        self.prof_pool = None     # optional pre-created timing events for it
        self.tape = None
        self.grad_norm_rows = None     # vfs_grad_norm_rows of the library, asked once (optim._grad_norm)
        # weight-gradient split-K partials: reduced per layer right after the kernel (default), or - inside the trackers'
        # backward chain (defer_wgrad) - kept in per-layer buffers and reduced by ONE table-driven launch per flush
        self.defer_wgrad = False
        self._wpending = []
        self._wtables = {}
        self._p2p, self._p2p_tried = None, False      # SyncBN statistic exchange over xGMI (vfs_amd/p2p.py), set up lazily
        self._xseq = 0      # number of the next folded SyncBN exchange of the running launch chain
        self.generation = 0  # bumped whenever a persistent buffer is (re)allocated: recorded launch chains hold raw pointers
        for kv in knobs.items('VFS_OPTS'):
            name, value = kv.split('=')
            self.lib.set_option(name.strip().encode(), int(value))

    # ------------------------------------------------------------------ command tape (see _lib.Tape)
    def begin_tape(self):
        assert self.tape is None
        self.tape = Tape(self.lib)
        self._real_lib, self.lib = self.lib, TapeLib(self.lib, self.tape)
        return self.tape

    def end_tape(self):
        self.lib, self.tape = self._real_lib, None

    @property
    def host_lib(self):
        """the library itself, also while a tape is recording: for host-only entry points (size queries) that are no part of a chain"""
        return self._real_lib if self.tape is not None else self.lib

    def record(self, fn, *args):
        """run a Python-side action of the chain (stream wait, collective) and put it on the tape if one is recording"""
        if self.tape is not None:
            self.tape.ops.append((None, fn, args))
        return fn(*args)

    # ------------------------------------------------------------------ plumbing
    @property
    def world(self):
        if dist.is_available() and dist.is_initialized():
            return dist.get_world_size(self.process_group)
        return 1

    @staticmethod
    def stream(dev):
        if dev.type == 'cuda':
            return torch.cuda.current_stream(dev).cuda_stream
        return None

    def buf(self, key, shape, dtype, dev):
        t = self.bufs.get(key)
        shape = tuple(int(s) for s in shape)
        if t is None or t.shape != shape or t.dtype != dtype or t.device != dev:
            if t is not None and dev.type == 'cuda':
                torch.cuda.synchronize(dev)     # a recorded chain may still be reading the old block
            t = torch.empty(shape, dtype=dtype, device=dev)
            self.bufs[key] = t
            self.generation += 1
        return t

    def ws(self, key, numel, dtype, dev, alloc=torch.empty):
        """grow-only flat workspace"""
        t = self.bufs.get(key)
        if t is None or t.numel() < numel or t.dtype != dtype or t.device != dev:
            if t is not None and dev.type == 'cuda':
                torch.cuda.synchronize(dev)     # the old block may still be in use on the side stream
            t = alloc(int(numel), dtype=dtype, device=dev)
            self.bufs[key] = t
            self.generation += 1
        return t

    def zeros(self, key, numel, dtype, dev):
        """grow-only flat buffer that starts zero-filled and that every user leaves zero (ticket counters, constant zero operands)"""
        return self.ws(key, numel, dtype, dev, alloc=torch.zeros)

    def conv_plan(self, u, N, G, H, W, dgrad=False):
        """the library's plan (packing.ConvPlan) for unit u's forward / dgrad launch over N images of H x W INPUT pixels"""
        Ho, Wo = u.out_hw(H, W)
        return conv_plan(N, G, H, W, u.cin, u.cout, u.k, u.stride, u.pad, Ho, Wo, dil=u.dil, dgrad=dgrad, lib=self.host_lib)

    def conv_kind(self, u, N, H, W, dgrad=False):
        """kernel family a forward / dgrad launch of unit u (input H x W) lands in, as the library dispatches it (bench.py's
        per-kernel roofline classes): stem_fwd | conv3x3_halo | conv_igemm"""
        if u.kind == 'stem':
            return 'stem_fwd'
        return 'conv3x3_halo' if self.conv_plan(u, N, 1, H, W, dgrad).halo else 'conv_igemm'

    def timed(self, kind, work, dev, fn, *args):
        """launch through `fn`; with profiling on, bracket it with events on the launch stream.
        work = algorithmic FLOP of the launch, or (FLOP, algorithmic HBM bytes: every operand once)"""
        flops, nbytes = work if isinstance(work, tuple) else (work, 0.0)
        if kind in knobs.items('VFS_DEBUG_SKIP'):      # what-if measurement: the step WITHOUT this family's launches
            return 0
        if self.prof is None or dev.type != 'cuda':
            if self.tape is not None:      # recording: the launch carries its family and algorithmic work onto the tape (_lib.Tape.meta)
                self.tape.next_meta = (kind, flops, nbytes)
                try:
                    return fn(*args)
                finally:
                    self.tape.next_meta = None
            return fn(*args)
        pool = self.prof_pool
        if pool:                       # pre-created events: creation is the expensive part
            e0, e1 = pool.pop(), pool.pop()
        else:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*args)
        e1.record()
        self.prof.append((kind, flops, e0, e1, nbytes))
        return rc

    @property
    def collectives_on(self):
        """collectives run when world > 1; VFS_FORCE_COLLECTIVES=1 also runs them in a 1-rank group
        (exercises the RCCL calls, dtypes and stream ordering on a single-GPU box)"""
        if not (dist.is_available() and dist.is_initialized()):
            return False
        return self.world > 1 or knobs.flag('VFS_FORCE_COLLECTIVES')

    def allreduce(self, t):
        """sum a SyncBN statistic buffer over the ranks: the P2P window exchange (vfs_amd/p2p.py; one small kernel, on the launch
        stream and on a recording tape like any other C-ABI call) when it is up, a collective-library all-reduce otherwise"""
        if not self.collectives_on:
            return
        x = self.p2p_exchange(t.device)
        if x is not None and x.fits(t):
            x.allreduce(self.lib, t, self.stream(t.device))
        else:
            self.record(self._all_reduce, t)

    def p2p_exchange(self, dev):
        """the SyncBN exchange of this process, set up on first use (VFS_SYNCBN_P2P=0: never; GPUs only; world > 1 - a 1-rank
        group with VFS_FORCE_COLLECTIVES=1 keeps exercising the collective-library calls).  Set-up or self-test failure on any
        rank -> None for good (collective library)."""
        if self._p2p is not None or self._p2p_tried:
            return self._p2p
        self._p2p_tried = True
        want = knobs.text('VFS_SYNCBN_P2P')
        if want not in ('1', 'force') or dev.type != 'cuda' or (self.world < 2 and want != 'force'):
            return None
        from .p2p import P2PExchange
        x, ok = None, 1
        try:
            x = P2PExchange(self._real_lib if self.tape is not None else self.lib, dev, self.process_group)
        except Exception as e:      # noqa: BLE001
            print(f'[vfs_amd] SyncBN P2P exchange unavailable ({type(e).__name__}: {e}); using the collective library', flush=True)
            ok = 0
        # every rank must take the same path: agree before (and inside) the self-test
        flag = torch.tensor([ok], dtype=torch.int32, device=dev if dist.get_backend(self.process_group) == 'nccl' else 'cpu')
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.process_group)
        if int(flag.item()) and x.self_test(self.stream(dev)):
            self._p2p = x
            self.generation += 1
        elif x is not None:
            if ok:
                print('[vfs_amd] SyncBN P2P exchange failed its self-test; using the collective library', flush=True)
            x.close()
        return self._p2p

    def p2p_chain_start(self, dev):
        """head of a launch chain (forward / backward of a train step): the folded SyncBN exchanges of the chain are numbered from 0
        and the chain counter in device memory moves on (vfs_p2p_chain_start; recorded on the tape like any other call)"""
        self._xseq = 0
        if not (self.collectives_on and knobs.flag('VFS_FIN_XCHG') and knobs.flag('VFS_FIN_FUSE')):
            return
        x = self.p2p_exchange(dev)
        if x is not None:
            self.lib.p2p_chain_start(x.state, self.stream(dev))

    def next_xseq(self):
        n = self._xseq
        self._xseq = n + 1
        return n

    def _all_reduce(self, t):
        dist.all_reduce(t, group=self.process_group)

    # ------------------------------------------------------------------ weights
    def register(self, unit):
        self.units.append(unit)
        self._pack = None
        self.generation += 1      # the pack table (and its bf16 weight copies) will be rebuilt
        return unit

    def pack_weights(self):
        """fp32 OIHW master weights -> bf16 MFMA layouts, all layers in ONE launch."""
        if not self.units:
            return
        dev = self.units[0].weight.device
        key = tuple((u.weight.data_ptr(), u.weight.device) for u in self.units)
        if self._pack is None or self._pack_key != key:
            entries = []
            for u in self.units:
                if u.kind == 'stem':
                    u.wf = torch.zeros(u.cout, 8, 8, 4, dtype=BF16, device=dev)
                    u.wd = None
                else:
                    u.wf = torch.empty(u.cout, u.k, u.k, u.cin, dtype=BF16, device=dev)
                    u.wd = torch.empty(u.cin, u.k, u.k, u.cout, dtype=BF16, device=dev) if u.need_wd else None
                entries.append((u.weight.data, u.wf, u.wd, 1 if u.kind == 'stem' else 0))
            if dev.type == 'cuda':
                torch.cuda.synchronize(dev)     # the previous packed copies may still be in use
            self._pack = build_pack_table(entries, dev)
            self._pack_key = key
            self.generation += 1
        tab, n, total = self._pack
        nel = sum(u.weight.numel() for u in self.units)
        self.timed('pack_weights', (0.0, 4.0 * nel + 2.0 * sum(u.weight.numel() * (2 if u.wd is not None else 1) for u in self.units)), dev,
                   self.lib.pack_weights, tab, n, total, self.stream(dev))

    # ------------------------------------------------------------------ forward primitives
    def conv_fwd(self, u, x, N, H, W, G, train, tag='', in_bn=None, defer_fin=False):
        """raw = conv(x); BN statistics/params when the unit has a BN.  Returns (raw, Ho, Wo, fin).  defer_fin: the caller's next
        launch is bn_act on raw, which gets `fin` - what is left for it to do (FinRows), the finished activation (FusedAct) or None"""
        dev = x.device
        s = self.stream(dev)
        lib = self.lib
        if u.kind == 'stem':
            Ho, Wo = (H + 6 - 7) // 2 + 1, (u.true_w + 6 - 7) // 2 + 1
        else:
            Ho, Wo = u.out_hw(H, W)
        M = N * Ho * Wo
        y = self.buf(f'{u.name}{tag}.raw', (N, Ho, Wo, u.cout), BF16, dev)
        want_stats = u.bn is not None and train
        Ng = N // G
        mpg = Ng * Ho * Wo
        # statistics rows per group when ONE launch covers all groups (spatial tiles of the halo kernels, ragged
        # edges included, or linear 128-pixel blocks), else one launch per group
        def rows_of(n, g):
            return stem_stats_rows(n, g, H, W, Ho, Wo, lib=self.host_lib) if u.kind == 'stem' else self.conv_plan(u, n, g, H, W).rows
        rows = rows_of(N, G)
        fused = rows is not None
        nblk_g = rows if fused else rows_of(Ng, 1)
        # small groups that are not multiples of the 128-pixel statistics rows (the head's Linear layers on the ResNet-50
        # config: 32 rows per view): ONE launch without statistics rows, the sums come from the stored output
        raw_stats = (want_stats and not fused and not self.collectives_on and mpg <= 2048
                     and knobs.flag('VFS_RAW_STATS'))
        # round 6: Linear + BatchNorm1d + ReLU of the head in ONE launch (vfs_linear_bn_act: the workgroup that owns 16 output channels
        # owns all <= 64 rows, so the batch statistics are local to it) instead of conv + statistics + apply
        lin_fused = (raw_stats and u.kind == 'linear' and defer_fin and M <= 256 and G <= 4 and u.cin % 128 == 0 and u.cout % 16 == 0
                     and knobs.flag('VFS_HEAD_FUSE'))
        if raw_stats:
            fused, want_rows = True, False
        else:
            want_rows = want_stats
        partial = self.ws('ws.stats', G * nblk_g * 2 * u.cout, torch.float32, dev) if want_rows else None
        bias = u.bias.data if u.bias is not None else None

        def work(n):      # algorithmic FLOP and HBM bytes (every operand once) of a launch over n images
            return (2.0 * n * Ho * Wo * u.cout * u.k * u.k * u.cin, 2.0 * (n * H * W * u.cin + n * Ho * Wo * u.cout + u.cout * u.k * u.k * u.cin))
        if lin_fused:
            bn = u.bn
            u.sums = self.buf(f'{u.name}.sums', (G, 2, u.cout), torch.float64, dev)
            u.bnp = self.buf(f'{u.name}{tag}.bnp', (G, 4, u.cout), torch.float32, dev)
            act = self.buf(f'{u.name}{tag}.act', (N, u.cout), BF16, dev)      # (the shape bn_act gives the head: raw.view(N, cout))
            flops, nbytes = work(N)
            self.timed('conv_igemm', (flops, nbytes + 2.0 * M * u.cout), dev, lib.linear_bn_act,      # (raw AND the activation go out)
                       x, u.wf, bias, bn.weight.data, bn.bias.data, y, act, u.bnp, u.sums, bn.running_mean, bn.running_var, M, u.cin, u.cout, mpg,
                       1 if u.relu else 0, float(mpg), float(bn.eps), float(bn.momentum), s)
            u.nbt_pending += G
            return y, Ho, Wo, FusedAct(act)
        groups = [(0, N, partial)] if fused else [
            (g * Ng, Ng, partial[g * nblk_g * 2 * u.cout:] if want_rows else None) for g in range(G)]
        for n0, nn_, part in groups:
            if u.kind == 'stem':
                self.timed('stem_fwd', (2.0 * nn_ * Ho * Wo * 64 * 147, 2.0 * nn_ * (H * W * 4 + Ho * Wo * 64)), dev, lib.stem_fwd,
                           x[n0:n0 + nn_], u.wf, y[n0:n0 + nn_], part, nn_, H, W, Ho, Wo, s)
            elif in_bn is not None:     # x is the producer's RAW output: BatchNorm + ReLU folded into the operand load
                assert (n0, nn_) == (0, N), 'folded input BatchNorm needs the single-launch (fused statistics) path'
                self.timed('conv3x3_halo' if u.k == 3 else 'conv_igemm', work(nn_), dev, lib.conv_fwd_bnin,
                           x, in_bn[0], in_bn[1], u.wf, y, bias, part, nn_, H, W, u.cin, Ho, Wo, u.cout,
                           u.k, u.k, u.stride, u.pad, s)
            elif u.dil != 1:            # dilated taps: implicit-GEMM forward only (frozen backbones)
                self.timed('conv_igemm', work(nn_), dev,
                           lib.conv_fwd_dilated, x[n0:n0 + nn_], u.wf, y[n0:n0 + nn_], bias, part, nn_, H, W, u.cin, Ho, Wo, u.cout,
                           u.k, u.k, u.stride, u.pad, u.dil, s)
            else:
                self.timed(self.conv_kind(u, nn_, H, W), work(nn_), dev, lib.conv_fwd, x[n0:n0 + nn_], u.wf, y[n0:n0 + nn_], bias, part,
                           nn_, H, W, u.cin, Ho, Wo, u.cout, u.k, u.k, u.stride, u.pad, s)
        fin = None if u.bn is None else self._finish_stats(u, y, partial, G, nblk_g, mpg, train, raw_stats, fused, defer_fin and u.kind != 'stem', tag)
        return y, Ho, Wo, fin

    @staticmethod
    def prologue_can_finish(nrows, G, C, xchg=False):
        """may an apply kernel (bn_act / bn_bwd_apply) sum `nrows` statistics rows per group in its prologue - and, with xchg, run the
        SyncBN window exchange of the sums there as well?"""
        return (knobs.flag('VFS_FIN_FUSE') and nrows <= knobs.integer('VFS_FIN_MAX_ROWS')
                and (not xchg or (knobs.flag('VFS_FIN_XCHG') and G * 2 * min(C, 64) <= 256 and C <= 4096)))

    def _finish_stats(self, u, y, partial, G, nblk_g, mpg, train, raw_stats, fused, defer, tag=''):
        """where the BatchNorm statistics of u's fresh output y get finished: eval parameters, from the stored output (raw_stats),
        in the prologue of the bn_act that follows (defer: there is one; fused: ONE conv launch wrote the rows in `partial`), or by
        the launches issued here (SyncBN: with the sums over the ranks in between).  Returns the FinRows for that bn_act, or None.
        tag: the batch's scale / shift / mean / invstd (u.bnp) belong to the pass - its backward reads them (vfs_amd/autograd.py)"""
        dev = y.device
        s = self.stream(dev)
        lib = self.lib
        bn = u.bn
        C = u.cout
        if not train:
            u.bnp = self.buf(f'{u.name}{tag}.bnp_eval', (1, 4, C), torch.float32, dev)      # (per pass: another module under the same name may be alive)
            lib.bn_eval_params(bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, u.bnp, C, float(bn.eps), s)
            return None
        u.sums = self.buf(f'{u.name}.sums', (G, 2, C), torch.float64, dev)
        u.bnp = self.buf(f'{u.name}{tag}.bnp', (G, 4, C), torch.float32, dev)
        u.nbt_pending += G   # num_batches_tracked, flushed lazily
        params = (bn.weight.data, bn.bias.data, u.bnp, bn.running_mean, bn.running_var)
        if raw_stats:
            self.timed('bn_stats', (0.0, 2.0 * y.numel()), dev, lib.bn_stats_raw_finalize, y, u.sums, *params,
                       G, mpg, C, float(mpg), float(bn.eps), float(bn.momentum), s)
            return None
        if not self.collectives_on:
            if defer and fused and self.prologue_can_finish(nblk_g, G, C):
                return FinRows(partial, nblk_g, float(mpg))
            self.timed('bn_stats', (0.0, 8.0 * G * nblk_g * C), dev, lib.bn_stats_finalize, partial, u.sums, self.bn_scratch(G, C, dev), *params,
                       G, nblk_g, C, float(mpg), float(bn.eps), float(bn.momentum), s)
            return None
        # SyncBN: statistics are summed over the ranks between the two stages
        count = float(mpg * self.world)
        x = self.p2p_exchange(dev)
        if x is not None and not x.fits(u.sums):
            x = None
        if x is not None and defer and fused and self.prologue_can_finish(nblk_g, G, C, xchg=True):
            return FinRows(partial, nblk_g, count, x)      # few rows: bn_act sums them AND runs the window exchange
        if x is not None:      # rows -> sums -> window exchange, one launch
            self.timed('bn_stats', (0.0, 8.0 * G * nblk_g * C), dev, lib.bn_reduce_partials_xchg, partial, u.sums,
                       self.bn_scratch(G, C, dev), G, nblk_g, C, *x.tail_args(), s)
        else:
            self.timed('bn_stats', (0.0, 8.0 * G * nblk_g * C), dev, lib.bn_reduce_partials, partial, u.sums,
                       self.bn_scratch(G, C, dev), G, nblk_g, C, s)
            self.allreduce(u.sums)
        if defer and knobs.flag('VFS_FIN_FUSE'):
            return FinRows(None, 0, count)      # bn_act turns the all-reduced sums into scale / shift itself (any size)
        lib.bn_finalize(u.sums, *params, G, C, count, float(bn.eps), float(bn.momentum), s)
        return None

    def can_fold_input_bn(self, u, N, G, H, W, train):
        """may conv unit u read the raw output of its producer (BatchNorm + ReLU folded into the load)?"""
        if not knobs.flag('VFS_BNACT_FUSE') or u.kind == 'stem' or u.dil != 1:
            return False
        # whole-image tiles (maps of at most 8x8): the fold is a loss
        if u.k == 3 and self.conv_plan(u, N, G, H, W).pairs and not knobs.flag('VFS_BNACT_FUSE_SMALL'):
            return False
        # pays only where the saved activation pass is large: the fold costs VALU work in the staging of the consumer's kernels
        mb = knobs.number('VFS_BNACT_FUSE_1X1_MB' if u.k == 1 else 'VFS_BNACT_FUSE_MB')
        if N * H * W * u.cin * 2 < mb * (1 << 20):
            return False
        Ng = N // G
        mpg = Ng * H * W
        if not (G == 1 or mpg % 128 == 0):      # the consumer must take the single-launch statistics path
            return False
        return bn_fold_eligible(N, G if train else 1, H, W, u.cin, u.cout, u.k, u.stride, u.pad, lib=self.host_lib)

    def bn_scratch(self, G, C, dev):
        """scratch of the chunked BatchNorm reductions: 64 ticket counters (must start at zero; every
        launch leaves them at zero) followed by double[G][128][2][C] chunk sums"""
        return self.zeros('ws.bnred', 32 + G * 128 * 2 * C, torch.float64, dev)

    def bn_act(self, u, raw, M, G, train, relu, fin=None, res=None, rres=None, rbnp=None, tag='', want_mask=False):
        """y = [relu](bn(raw) [+ res] [+ bn(rres)]).  fin: what the conv_fwd that produced raw returned for this call.
        want_mask (the join of a residual block, training): also write the bit-packed mask y > 0 (uint8 [M][C/8], left in u.mask_bits) - the unit's BatchNorm backward reads it instead of y"""
        dev = raw.device
        if isinstance(fin, FusedAct):      # Linear + BatchNorm1d + ReLU ran as one launch (conv_fwd, lin_fused)
            assert res is None and rres is None and not want_mask and bool(relu) == bool(u.relu)
            u.mask_bits = None
            return fin.act
        y = self.buf(f'{u.name}{tag}.act', raw.shape, BF16, dev)
        u.mask_bits = self.buf(f'{u.name}{tag}.mbits', (M * u.cout // 8,), torch.uint8, dev) if (want_mask and knobs.flag('VFS_MASK_BITS') and u.cout % 8 == 0 and (u.cout < 64 or u.cout % 64 == 0)) else None      # slab-major layout (mask8_index): whole 64-channel slabs
        mpg = M // G if train else M
        nbytes = 2.0 * M * u.cout * (2 + (res is not None) + (rres is not None)) + (M * u.cout / 8.0 if u.mask_bits is not None else 0.0)      # raw in, activation out, identity in (+ mask bits out)
        if fin is None:
            self.timed('bn_act', (0.0, nbytes), dev, self.lib.bn_act_mask, raw, u.bnp, res, rres, rbnp, y, u.mask_bits, M, u.cout, mpg, 1 if relu else 0,
                       self.stream(dev))
            return y
        bn = u.bn
        # the statistics rows are summed in the prologue; SyncBN (fin.xchg): AND exchanged with the peers inside this launch
        fn, tail = (self.lib.bn_act_fin_mask, ()) if fin.xchg is None else (self.lib.bn_act_fin_xchg, (*fin.xchg.tail_args(), self.next_xseq()))
        self.timed('bn_act', (0.0, nbytes), dev, fn, raw, fin.rows, fin.nrows, bn.weight.data, bn.bias.data, u.bnp, u.sums, bn.running_mean, bn.running_var,
                   res, rres, rbnp, y, u.mask_bits, M, u.cout, mpg, 1 if relu else 0, fin.count, float(bn.eps), float(bn.momentum), *tail, self.stream(dev))
        return y

    # ------------------------------------------------------------------ backward primitives
    def grad_join(self, g, new, key, N, HW, C):
        """the gradient wrt a [N, HW, C] activation: `new` - bf16 NHWC or NCHWGrad - alone (g is None) or joined with the bf16 NHWC
        gradient g already in flight: bf16_rne(float(g) + new), one launch, one rounding.  A bf16 `new` alone is returned as it is;
        everything else lands in the engine buffer `key`."""
        if g is None and not isinstance(new, NCHWGrad):
            return new
        dev = new.t.device if isinstance(new, NCHWGrad) else new.device
        s = self.stream(dev)
        dst = self.buf(key, (N, HW, C), BF16, dev)
        if isinstance(new, NCHWGrad):
            t = new.t.contiguous().float()
            if t.numel() != N * HW * C:
                raise ValueError(f'{key}: a gradient of {tuple(t.shape)} for an activation of [{N}, {C}, {HW}]')
            if g is None:
                self.timed('layout', (0.0, 6.0 * t.numel()), dev, self.lib.nchw_f32_to_nhwc_bf16, t, dst, N, HW, C, s)
            else:
                self.timed('layout', (0.0, 8.0 * t.numel()), dev, self.lib.nchw_f32_add_nhwc_bf16, t, g, dst, N, HW, C, s)
        else:
            if new.dtype != BF16 or new.numel() != N * HW * C:
                raise ValueError(f'{key}: a {new.dtype} gradient of {tuple(new.shape)} for a bf16 activation of [{N}, {HW}, {C}]')
            self.timed('layout', (0.0, 6.0 * new.numel()), dev, self.lib.bf16_add, g, new.contiguous(), dst, N * HW * C, s)
        return dst

    @staticmethod
    def bwd_row_pixels(mpg, cap):
        """pixels per BatchNorm-backward statistics row: a divisor of the group size mpg (rows never straddle groups), at most cap;
        a whole group per row where that divisor would be under 16"""
        ppb = math.gcd(mpg, cap)
        return ppb if ppb >= 16 else mpg

    def bn_bwd(self, u, g, ymask, raw, M, G, want_gm=False, relu=False, rows=None, tag=''):
        """gradient wrt the raw conv output (and optionally the ReLU-masked incoming gradient).
        ymask: the unit's output (residual units); relu=True without ymask: conv->BN->ReLU unit,
        the mask is recomputed from raw inside the kernels.
        rows: the BwdRows the conv_bwd that produced g returned (the reduce pass is skipped), or None.
        tag: buffer namespace of the pass (a second context of another size alive at the same time keeps its own buffers)."""
        assert rows is None or rows.unit is u, 'backward statistics rows of another unit'
        if knobs.flag('VFS_DEBUG_NOMASK'):
            ymask = None       # what-if only (WRONG gradients): the step without the mask operand reads
        if not u.bn.training:
            return self._bn_bwd_eval(u, g, ymask, raw, M, want_gm, relu, rows, tag)
        dev = raw.device
        s = self.stream(dev)
        lib = self.lib
        C = u.cout
        mpg = M // G
        ppb = self.bwd_row_pixels(mpg, 512)
        nblk = M // ppb
        partial = self.ws('ws.bnbwd', nblk * 2 * C, torch.float32, dev)
        u.bsums = self.buf(f'{u.name}.bsums', (G, 2, C), torch.float64, dev)
        bits = ymask is not None and ymask.dtype == torch.uint8      # bit-packed mask from bn_act(want_mask=True)
        rl = 2 if bits else (1 if relu else 0)
        mask_bytes = 0.0 if ymask is None else (M * C / 8.0 if bits else 2.0 * M * C)
        raw_row = False
        if rows is not None:     # the producing dgrad already emitted the statistics rows
            partial, nblk = rows.rows, rows.nrows
        elif knobs.flag('VFS_FIN_FUSE') and not self.collectives_on and nblk == G and mpg <= 512 and knobs.flag('VFS_HEAD_FUSE'):
            raw_row = True      # round 6: one statistics row per group (the head's BatchNorm1d layers): the apply pass computes it itself
        else:
            self.timed('bn_bwd_reduce', (0.0, 2.0 * M * C * 2 + mask_bytes), dev, lib.bn_bwd_reduce, g, ymask, raw, u.bnp,
                       partial, M, C, mpg, ppb, rl, s)
        dx = self.buf(f'{u.name}{tag}.dx', raw.shape, BF16, dev)
        # with the bit-packed mask the masked gradient is not materialised: its consumers take (g, mask) instead (conv_bwd add_mask,
        # the downsample unit's bn_bwd)
        want_gm = want_gm and not (bits and knobs.flag('VFS_MASK_ADD') and C % 64 == 0)      # (the mask-gated add reads whole 64-channel mask words)
        gm = self.buf(f'{u.name}{tag}.gm', raw.shape, BF16, dev) if want_gm else None
        abytes = 2.0 * M * C * (3 + want_gm) + mask_bytes      # g, raw in; dx out; activation (or its bit mask) in; masked gradient out
        if raw_row:
            self.timed('bn_bwd_apply', (0.0, abytes + 2.0 * M * C * 2 + mask_bytes), dev, lib.bn_bwd_apply_raw, g, ymask, raw, u.bnp, u.bsums, u.bn.weight.grad, u.bn.bias.grad,
                       dx, gm, M, C, mpg, float(mpg), rl, s)
            return dx, gm
        if self.collectives_on and self.prologue_can_finish(nblk // G, G, C, xchg=True):
            x = self.p2p_exchange(dev)
            if x is not None and x.fits(u.bsums):
                # SyncBN, few statistics rows: the apply pass sums them in its prologue, exchanges the sums with the peers there and
                # writes bsums (over the ranks), dgamma, dbeta (local)
                self.timed('bn_bwd_apply', (0.0, abytes), dev, lib.bn_bwd_apply_fin_xchg, g, ymask, raw, u.bnp, partial, nblk // G, u.bsums, u.bn.weight.grad, u.bn.bias.grad,
                           dx, gm, M, C, mpg, float(mpg * self.world), rl, *x.tail_args(), self.next_xseq(), s)
                return dx, gm
        if not self.collectives_on and self.prologue_can_finish(nblk // G, G, C):
            # few statistics rows: the apply pass sums them in its prologue (and writes bsums, dgamma, dbeta)
            self.timed('bn_bwd_apply', (0.0, abytes), dev, lib.bn_bwd_apply_fin, g, ymask, raw, u.bnp, partial, nblk // G, u.bsums, u.bn.weight.grad, u.bn.bias.grad, dx, gm, M, C,
                                 mpg, float(mpg), rl, s)
            return dx, gm
        self._bwd_sums(u, partial, G, nblk // G, C, dev)
        self.timed('bn_bwd_apply', (0.0, abytes), dev, lib.bn_bwd_apply, g, ymask, raw, u.bnp, u.bsums, dx, gm, M, C, mpg,
                   float(mpg * self.world), rl, s)
        return dx, gm

    def zero_sums(self, C, dev):
        """double[1][2][C] of zeros (never written): BatchNorm backward without the batch-statistic terms"""
        return self.zeros(f'ws.zero_sums.{C}', 2 * C, torch.float64, dev)

    def _bn_bwd_eval(self, u, g, ymask, raw, M, want_gm, relu, rows, tag=''):
        """BatchNorm in eval mode inside a training step (resnet.py:577-654: frozen_stages, norm_eval, partial_bn): the output is
        an affine map of the input with FIXED coefficients, so dx = g * mask * scale - the apply kernel with zero statistic
        sums - and, when gamma / beta are still trained (norm_eval), dgamma = sum g*mask*xhat, dbeta = sum g*mask with xhat
        from the running statistics.  One group, no SyncBN exchange (the parameter gradients are local sums like any other)."""
        dev = raw.device
        s = self.stream(dev)
        lib = self.lib
        C = u.cout
        bits = ymask is not None and ymask.dtype == torch.uint8
        rl = 2 if bits else (1 if relu else 0)
        if u.bn.weight.requires_grad or u.bn.bias.requires_grad:
            if rows is not None:
                partial, nblk = rows.rows, rows.nrows
            else:
                ppb = self.bwd_row_pixels(M, 512)
                nblk = M // ppb
                partial = self.ws('ws.bnbwd', nblk * 2 * C, torch.float32, dev)
                self.timed('bn_bwd_reduce', (0.0, 4.0 * M * C), dev, lib.bn_bwd_reduce, g, ymask, raw, u.bnp, partial, M, C, M, ppb, rl, s)
            scratch = self.buf(f'{u.name}.bsums', (1, 2, C), torch.float64, dev)
            self.timed('bn_stats', (0.0, 8.0 * nblk * C), dev, lib.bn_bwd_sums_paramgrad, partial, scratch, self.bn_scratch(1, C, dev),
                       u.bn.weight.grad, u.bn.bias.grad, 1, nblk, C, s)
        dx = self.buf(f'{u.name}{tag}.dx', raw.shape, BF16, dev)
        want_gm = want_gm and not (bits and knobs.flag('VFS_MASK_ADD') and C % 64 == 0)      # (the mask-gated add reads whole 64-channel mask words)
        gm = self.buf(f'{u.name}{tag}.gm', raw.shape, BF16, dev) if want_gm else None
        self.timed('bn_bwd_apply', (0.0, 2.0 * M * C * (3 + want_gm)), dev, lib.bn_bwd_apply, g, ymask, raw, u.bnp, self.zero_sums(C, dev), dx, gm,
                   M, C, M, 1.0, rl, s)
        return dx, gm

    def _bwd_sums(self, u, partial, G, bpg, C, dev):
        """partial (S1, S2) rows -> u.bsums (all-reduced for SyncBN) and dgamma / dbeta (local sums)"""
        # SyncBN with the window exchange up: the reduction's last workgroup runs it in the same launch; else the sums go over the ranks after it
        x = self.p2p_exchange(dev) if self.collectives_on else None
        xchg = x is not None and x.fits(u.bsums)
        self.timed('bn_stats', (0.0, 8.0 * G * bpg * C), dev, self.lib.bn_bwd_sums_paramgrad_xchg if xchg else self.lib.bn_bwd_sums_paramgrad,
                   partial, u.bsums, self.bn_scratch(G, C, dev), u.bn.weight.grad, u.bn.bias.grad, G, bpg, C, *(x.tail_args() if xchg else ()), self.stream(dev))
        if not xchg:
            self.allreduce(u.bsums)

    def flush_counters(self):
        """materialise the lazily counted BatchNorm.num_batches_tracked buffers"""
        for u in self.units:
            if u.nbt_pending and u.bn is not None:
                u.bn.num_batches_tracked += u.nbt_pending
                u.nbt_pending = 0

    def stem_pool_bn_bwd(self, u, gp, yp, idx, raw, N, H, W, Hp, Wp, G, xpool=None):
        """BN backward of the stem through max-pool + ReLU (no full-resolution gradient tensor)."""
        dev = raw.device
        s = self.stream(dev)
        lib = self.lib
        C = u.cout
        if not u.bn.training:      # eval-mode BatchNorm (norm_eval): one group, no statistic terms in dx (zero sums)
            G = 1
        npg = N // G
        mpg_p = npg * Hp * Wp
        ppb = self.bwd_row_pixels(mpg_p, 256)
        nblk = (N * Hp * Wp) // ppb
        partial = self.ws('ws.bnbwd', nblk * 2 * C, torch.float32, dev)
        u.bsums = self.buf(f'{u.name}.bsums', (G, 2, C), torch.float64, dev)
        self.timed('bn_bwd_reduce', (0.0, (2.0 * 2 + 1.0) * N * Hp * Wp * C), dev, lib.stem_pool_bn_bwd_reduce, gp, yp, idx, raw, xpool,
                   u.bnp, partial, N, H, W, C, Hp, Wp, npg, ppb, s)
        if u.bn.training:
            self._bwd_sums(u, partial, G, nblk // G, C, dev)
            return float(npg * H * W * self.world)
        if u.bn.weight.requires_grad or u.bn.bias.requires_grad:
            scratch = self.buf(f'{u.name}.bsums_eval', (1, 2, C), torch.float64, dev)
            self.timed('bn_stats', (0.0, 8.0 * nblk * C), dev, lib.bn_bwd_sums_paramgrad, partial, scratch, self.bn_scratch(1, C, dev),
                       u.bn.weight.grad, u.bn.bias.grad, 1, nblk, C, s)
        u.bsums = self.zero_sums(C, dev)
        return 1.0

    # ------------------------------------------------------------------ side stream for weight gradients
    def on_side_stream(self, dev):
        """context: subsequent launches go to the side stream, ordered after everything already
        enqueued on the current stream (no-op on the CPU / when VFS_SIDE_STREAM=0)"""
        import contextlib
        if not side_stream_on(dev):
            return contextlib.nullcontext()
        side = self._side.get(dev)
        if side is None:
            side = self._side[dev] = torch.cuda.Stream(dev)
        self.record(side.wait_stream, torch.cuda.current_stream(dev))
        self._side_dirty = True
        return torch.cuda.stream(side)

    def wgrad_join(self, dev):
        """the current stream waits for every weight-gradient kernel issued so far"""
        if dev.type == 'cuda' and self._side_dirty:
            side = self._side.get(dev)
            if side is not None:
                self.record(torch.cuda.current_stream(dev).wait_stream, side)
            self._side_dirty = False

    def stem_wgrad_fused(self, u, x4, Hin, Win, gp, yp, idx, raw, N, H, W, Hp, Wp, G, count):
        """stem weight gradient; the BN-backward apply pass is folded into its operand load"""
        dev = raw.device
        ntiles = N * ((H + 7) // 8) * ((W + 15) // 16)
        nb = knobs.integer('VFS_STEM_WGRAD_BLOCKS')
        tpb = (ntiles + nb - 1) // nb        # ~6 workgroups per CU: the operand gather is latency-bound
        nblocks = (ntiles + tpb - 1) // tpb
        partial = self.wgrad_partial(u, nblocks, 64, 224, dev)
        with self.on_side_stream(dev):      # ws.wgrad belongs to the side stream
            self.timed('stem_wgrad', (2.0 * N * H * W * 64 * 147, 2.0 * N * (Hin * Win * 4 + H * W * 64) + 5.0 * N * Hp * Wp * 64),
                       dev, self.lib.stem_wgrad_fused,
                       x4, raw, gp, yp, idx, u.bnp, u.bsums, partial, self.wgrad_target(u, partial, nblocks, 64, 224, 3, 7, 1),
                       N, Hin, Win, H, W, Hp, Wp, (N // G) if u.bn.training else N, count, nblocks, self.stream(dev))

    def wgrad_partial(self, u, nsplit, cout, ktot, dev):
        """split-K workspace of unit u's weight gradient: the shared scratch (reduced right after the kernel) or, when the
        reduction is deferred, a per-unit buffer that lives until flush_wgrad"""
        if self.defer_wgrad:
            return self.buf(f'{u.name}.wpart', (nsplit * cout * ktot,), torch.float32, dev)
        return self.ws('ws.wgrad', nsplit * cout * ktot, torch.float32, dev)

    def wgrad_target(self, u, partial, nsplit, cout, ktot, cin, k, stem):
        """the `grad` argument of the weight-gradient entry points: the gradient itself, or None (= reduce later)"""
        if not self.defer_wgrad:
            return u.weight.grad
        self._wpending.append((partial, u.weight.grad, nsplit, cout, ktot, cin, k, k, stem))
        return None

    def flush_wgrad(self, dev):
        """ONE table-driven launch reduces the split-K partials of every weight gradient issued since the last flush
        (side stream, after the kernels that wrote them)"""
        if not self._wpending:
            return
        pend, self._wpending = self._wpending, []
        key = tuple((p.data_ptr(), g.data_ptr(), ns) for p, g, ns, *_ in pend)
        tab = self._wtables.get(key)
        if tab is None:
            if len(self._wtables) > 64:
                self._wtables.clear()
            tab = self._wtables[key] = build_reduce_table(pend, dev)
            self.generation += 1
        with self.on_side_stream(dev):
            self.lib.wgrad_reduce_table(tab[0], tab[1], tab[2], self.stream(dev))

    def conv_bwd(self, u, dx, x_in, N, H, W, Ho, Wo, need_dgrad, add=None, g_out=None, bn_next=None, x_in_bn=None, add_mask=None, tag=''):
        """weight (and bias) gradients accumulate into .grad; returns (input gradient or None, BwdRows or None).
        bn_next = (unit, raw, ymask, relu, G): the BatchNorm unit whose backward consumes the input
        gradient; for stride-1 convs the dgrad epilogue also emits that unit's backward statistics
        (vfs_conv_dgrad_bn): handed to its bn_bwd, the returned BwdRows let it skip the reduce pass."""
        dev = dx.device
        s = self.stream(dev)
        lib = self.lib
        M = N * Ho * Wo
        if u.dil != 1:
            raise NotImplementedError(f'{u.name}: conv_bwd takes undilated units; the backward of a dilated convolution is '
                                      'Engine.conv_bwd_dilated (ResNet._block_bwd routes there)')
        if u.kind == 'stem':
            nsplit, pps = wgrad_splits(M, 64, 256)
            partial = self.wgrad_partial(u, nsplit, 64, 256, dev)
            with self.on_side_stream(dev):
                self.timed('stem_wgrad', (2.0 * M * 64 * 147, 2.0 * (M * 64 + N * H * W * 4)), dev, lib.stem_wgrad,
                           dx, x_in, partial, self.wgrad_target(u, partial, nsplit, 64, 256, 3, 7, 1), N, H, W, Ho, Wo, nsplit, pps,
                           self.stream(dev))
            return None, None
        ktot = u.k * u.k * u.cin
        halo = (N, H, W, u.cin) if wgrad_halo_eligible(N, H, W, u.cin, u.cout, u.k, u.stride, u.pad, lib=self.host_lib) else None
        nsplit, pps = wgrad_splits(M, u.cout, ktot, halo_geom=halo, lib=self.host_lib)
        partial = self.wgrad_partial(u, nsplit, u.cout, ktot, dev) if u.weight.requires_grad else None
        flops = 2.0 * M * u.cout * ktot
        # ALGORITHMIC bytes: dY + x once, the fp32 gradient read-modify-write.  (The fp32 split-K partials - written by the
        # kernel, re-read by the reduction: 8 * nsplit * Cout * Ktot bytes - are implementation traffic; they show up in the
        # PMC 'traffic' figure, not here.)
        wbytes = 2.0 * (M * u.cout + N * H * W * u.cin) + 8.0 * u.cout * ktot
        # dgrad: dY + weights in, dx out (+ residual gradient / fused BatchNorm operands when present)
        dbytes = 2.0 * (M * u.cout + N * H * W * u.cin + u.cout * ktot)
        # the weight gradient only feeds the optimizer: it runs on the side stream, concurrently
        # with the dgrad / BatchNorm-backward kernels of the critical path (joined by wgrad_join).  Frozen weights
        # (requires_grad = False: frozen_stages) get none.
        if u.weight.requires_grad:
            wtarget = self.wgrad_target(u, partial, nsplit, u.cout, ktot, u.cin, u.k, 0)
            with self.on_side_stream(dev):
                ss = self.stream(dev)
                family = 'conv3x3_wgrad_halo' if halo is not None else 'conv_wgrad'
                if x_in_bn is not None:     # x_in is the producer's RAW output (see conv_fwd)
                    self.timed(family, (flops, wbytes), dev, lib.conv_wgrad_bnin, dx, x_in, x_in_bn[0], x_in_bn[1], partial,
                               wtarget, N, H, W, u.cin, Ho, Wo, u.cout, u.k, u.k, u.stride, u.pad, nsplit, pps, ss)
                else:
                    self.timed(family, (flops, wbytes), dev, lib.conv_wgrad, dx, x_in, partial, wtarget, N, H, W, u.cin, Ho,
                               Wo, u.cout, u.k, u.k, u.stride, u.pad, nsplit, pps, ss)
                if u.bias is not None and u.bias.requires_grad:
                    lib.bias_grad(dx, u.bias.grad, M, u.cout, ss)
        elif u.bias is not None and u.bias.requires_grad:      # a trainable bias under a frozen weight (the SiamFC head allows it)
            with self.on_side_stream(dev):
                lib.bias_grad(dx, u.bias.grad, M, u.cout, self.stream(dev))
        if not need_dgrad:
            return None, None
        gin = g_out if g_out is not None else self.buf(f'{u.name}{tag}.gin', (N, H, W, u.cin), BF16, dev)
        if bn_next is not None and u.stride == 1 and knobs.flag('VFS_BN_FUSE'):
            pu, praw, pymask, prelu, G = bn_next
            if knobs.flag('VFS_DEBUG_NOMASK'):
                pymask = None
            Min = N * H * W
            mpg = Min // G
            # the dgrad as a conv [N,Ho,Wo,cout] -> [N,H,W,cin]: its statistics rows (tiles or linear blocks)
            rows = self.conv_plan(u, N, G, H, W, dgrad=True).rows
            if rows is not None:
                nblk = rows * G
                partial = self.ws('ws.bnbwd_fused', nblk * 2 * u.cin, torch.float32, dev)
                pbits = pymask is not None and pymask.dtype == torch.uint8
                mask_units = 0.0 if pymask is None else (1.0 / 16 if pbits else 1.0)
                self.timed(self.conv_kind(u, N, H, W, dgrad=True), (flops, dbytes + 2.0 * N * H * W * u.cin * ((1 if add is not None else 0) + 1 + mask_units)),
                           dev, lib.conv_dgrad_bn_maskadd, dx, u.wd, gin, add, add_mask, praw, pymask, pu.bnp, partial,
                           mpg, 2 if pbits else (1 if (prelu and pymask is None) else 0), N, H, W, u.cin, Ho, Wo, u.cout, u.k, u.k,
                           u.stride, u.pad, s)
                return gin, BwdRows(pu, partial, nblk)
        work = (flops, dbytes + (2.0 * N * H * W * u.cin if add is not None else 0.0))
        self.timed(self.conv_kind(u, N, H, W, dgrad=True), work, dev, lib.conv_dgrad_maskadd, dx, u.wd, gin, add, add_mask, N, H, W, u.cin, Ho, Wo, u.cout,
                   u.k, u.k, u.stride, u.pad, s)
        return gin, None

    def conv_bwd_dilated(self, u, dx, x_in, N, H, W, Ho, Wo, need_dgrad, add=None, add_mask=None, g_out=None, tag=''):
        """conv_bwd for a unit with u.dil != 1 (vfs_conv_wgrad_dilated / vfs_conv_dgrad_dilated): the weight gradient accumulates
        into .grad on the side stream (none for a frozen weight; deferred reduction as in conv_bwd), the input gradient takes the
        residual `add`, gated by the bit-packed `add_mask`.  The dilated dgrad emits no BatchNorm-backward statistics rows: returns
        (input gradient or None, None) and the consumer's bn_bwd runs its own reduce pass."""
        dev = dx.device
        lib = self.lib
        if u.kind != 'conv' or u.dil == 1:
            raise ValueError(f'{u.name}: conv_bwd_dilated takes dilated conv units (dil={u.dil}, kind={u.kind})')
        M = N * Ho * Wo
        ktot = u.k * u.k * u.cin
        flops = 2.0 * M * u.cout * ktot
        if u.weight.requires_grad:
            nsplit, pps = wgrad_splits(M, u.cout, ktot, lib=self.host_lib)
            partial = self.wgrad_partial(u, nsplit, u.cout, ktot, dev)
            wtarget = self.wgrad_target(u, partial, nsplit, u.cout, ktot, u.cin, u.k, 0)
            with self.on_side_stream(dev):
                ss = self.stream(dev)
                self.timed('conv_wgrad_dilated', (flops, 2.0 * (M * u.cout + N * H * W * u.cin) + 8.0 * u.cout * ktot), dev, lib.conv_wgrad_dilated,
                           dx, x_in, partial, wtarget, N, H, W, u.cin, Ho, Wo, u.cout, u.k, u.k, u.stride, u.pad, u.dil, nsplit, pps, ss)
                if u.bias is not None and u.bias.requires_grad:
                    lib.bias_grad(dx, u.bias.grad, M, u.cout, ss)
        if not need_dgrad:
            return None, None
        gin = g_out if g_out is not None else self.buf(f'{u.name}{tag}.gin', (N, H, W, u.cin), BF16, dev)
        dbytes = 2.0 * (M * u.cout + N * H * W * u.cin * (2 if add is not None else 1) + u.cout * ktot)
        self.timed('conv_dgrad_dilated', (flops, dbytes), dev, lib.conv_dgrad_dilated, dx, u.wd, gin, add, add_mask, N, H, W, u.cin, Ho, Wo,
                   u.cout, u.k, u.k, u.stride, u.pad, u.dil, self.stream(dev))
        return gin, None


_ENGINES = {}

# Bumped by everything that writes parameters or BatchNorm running statistics THROUGH RAW POINTERS (vfs_sgd_step /
# vfs_adam_step on the arenas, the BatchNorm kernels of a training forward): such writes never touch tensor._version, so
# caches of derived data (the fp32 evaluation executor's folded BatchNorm / repacked weights, the SiamFC head's packed
# weights) key on this counter as well.
_PARAMS_EPOCH = [0]


def params_epoch():
    return _PARAMS_EPOCH[0]


def bump_params_epoch():
    _PARAMS_EPOCH[0] += 1


def shared_engine(device=None):
    """One Engine (buffer pool + packed weights) per process; one process drives one GPU."""
    eng = _ENGINES.get('default')
    if eng is None:
        eng = _ENGINES['default'] = Engine()
    return eng


def flush_counters_hook(module, prefix, keep_vars):
    """state_dict pre-hook of the VFS modules: num_batches_tracked is counted on the host"""
    eng = _ENGINES.get('default')
    if eng is not None:
        eng.flush_counters()


def set_shared_engine(eng):
    _ENGINES['default'] = eng
