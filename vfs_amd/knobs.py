"""The VFS_* environment variables of the Python side: one table, read through the accessors below and nowhere else in vfs_amd/.

Every accessor reads os.environ at the moment of the call, so a knob can be switched inside a process - it takes effect for
chains that run eagerly or are recorded afterwards (a recorded chain replays what was decided while it was recorded).  A name
that is not in the table is a KeyError.  Classes: `product` - an operator may set it; `ab` - a measurement switch, the default
is the measured-best setting; `debug` - diagnostics and what-if timing, results may be wrong.
`python -m vfs_amd.knobs` prints the table as Markdown."""
import os

# name: (default as the environment would spell it - None: unset, kind, class, what it does and what was measured)
TABLE = {
    # launch path
    'VFS_TAPE': ('1', 'flag', 'product', 'launch chains recorded once as a host-side command tape and replayed (~4 us of CPU per launch '
                 'instead of ~25); 0: plain eager'),
    'VFS_GRAPHS': ('0', 'flag', 'product', 'single process on a GPU: each chain captured into a hipGraph and replayed; the tape beats it on '
                   'MI355X (R50 10.7 -> 10.1 ms, R18 8.04 -> 7.81: the weight-gradient stream overlaps better with direct launches)'),
    'VFS_GC_FREEZE': ('0', 'flag', 'product', 'gc.freeze() once the launch chains are recorded (a full collection over the live objects of a '
                      'torch process showed up as +3.5 ms per step inside 20 R18 steps); process-wide, therefore opt-in: bench.py sets it, a '
                      'training script that owns its process can too'),
    'VFS_SIDE_STREAM': ('1', 'flag', 'ab', 'weight gradients on a second stream, beside the dgrad / BatchNorm-backward chain'),
    'VFS_MAIN_PRIO': (None, 'choice: 0, 1', 'ab', 'forbids / forces the high-priority stream for the launch chains; unset: only with '
                      'collectives (1-rank RCCL group: R50 13.47 -> 12.55 ms, R18 9.40 -> 9.13; without collectives it changes nothing)'),
    'VFS_FAST_TRAIN_STEP': ('1', 'flag', 'ab', 'train_step reduces the loss on the device inside the forward chain and reads the log vars '
                            'once; 0: the reference\'s _parse_losses (~30 tiny launches, 0.33 ms of GPU idle time per 8.5 ms R18 step)'),
    'VFS_LAZY_LOG': ('1', 'flag', 'ab', 'log_vars of the fused train_step are read from the device on first access, not inside train_step '
                     '(0.2 ms of GPU idle time per R50 step otherwise)'),
    'VFS_LOG_ASYNC': ('1', 'flag', 'ab', 'with VFS_LAZY_LOG: through an asynchronous pinned copy queued behind the forward chain; 0: a '
                      'blocking read of the device tensor (~0.1 ms of GPU idle time at each step boundary)'),
    # BatchNorm statistics
    'VFS_FIN_FUSE': ('1', 'flag', 'ab', 'BatchNorm statistics finished in the apply kernels\' prologue'),
    'VFS_FIN_MAX_ROWS': ('128', 'int', 'ab', '... for at most this many statistics rows per group'),
    'VFS_FIN_XCHG': ('0', 'flag', 'ab', 'SyncBN: ... and the window exchange folded into the same launch (vfs_bn_act_fin_xchg / '
                     'vfs_bn_bwd_apply_fin_xchg); measured LEVEL with the reduction + exchange launch on one GPU (8.92 vs 8.88 ms), and its '
                     'waiting workgroups hold their CUs, so the default stays 0'),
    'VFS_RAW_STATS': ('1', 'flag', 'ab', 'statistics from the stored output for small groups that are not multiples of the 128-pixel '
                      'statistics rows (the head\'s Linear layers: 32 rows per view)'),
    'VFS_HEAD_FUSE': ('1', 'flag', 'ab', 'the head\'s Linear + BatchNorm1d + ReLU units in one launch (vfs_linear_bn_act) and BatchNorm '
                      'backward of single-row groups without the reduction launch (vfs_bn_bwd_apply_raw); 0: three / two launches - same bits'),
    'VFS_BN_FUSE': ('1', 'flag', 'ab', 'BatchNorm-backward statistics from the producing stride-1 dgrad\'s epilogue (vfs_conv_dgrad_bn)'),
    'VFS_MASK_BITS': ('1', 'flag', 'ab', 'residual joins also write a bit-packed ReLU mask; their BatchNorm backward reads it instead of the '
                      'block output (R50 -0.3 ms) - same bits'),
    'VFS_MASK_ADD': ('1', 'flag', 'ab', 'with VFS_MASK_BITS: the identity-branch gradient g * (y > 0) is applied on the fly '
                     '(vfs_conv_dgrad_maskadd), never written'),
    # BatchNorm + ReLU folded into the consumer's operand load
    'VFS_BNACT_FUSE': ('1', 'flag', 'ab', 'a conv reads the RAW output of its producer: BatchNorm-apply + ReLU folded into the staging of its '
                       'forward and weight-gradient kernels'),
    'VFS_BNACT_FUSE_MB': ('16', 'float', 'ab', '... for 3x3 consumers whose input has at least this many MB: the fold costs VALU work, it pays '
                          'where the saved activation pass is large (threshold 48 / 32 / 16: R50 9.36 / 9.30 / 9.24 ms, R18 unchanged - its '
                          'folded tensors are all >= 48 MB)'),
    'VFS_BNACT_FUSE_1X1': ('1', 'flag', 'ab', '... and for the 1x1 / stride-1 consumer (conv2 -> conv3 of a bottleneck block) on the '
                           'register-staged implicit-GEMM forward and weight-gradient kernels'),
    'VFS_BNACT_FUSE_1X1_MB': ('16', 'float', 'ab', '... whose input has at least this many MB'),
    'VFS_BNACT_FUSE_SMALL': ('0', 'flag', 'ab', '1: also fold for 3x3 consumers on whole-image tiles (maps of at most 8x8), where it is a loss '
                             '(R18 layer4 at 256^2, 17 MB: step 6.90 with, 6.82 without - profiles/r06_fold3x3_threshold_step_ab.txt); tests switch it on to run those kernels through '
                             'the engine'),
    # weight gradients
    'VFS_WGRAD_TB': ('192', 'int', 'ab', 'workgroup target of the halo weight gradient\'s split-K plan; whole-step A/B beside the dgrad chain: '
                     '256 > 128 > 512, then with the leaner main chain 192 > 256 > 384 (R18 6.84 -> 6.79 ms)'),
    'VFS_WGRAD_TBG': (None, 'optional int', 'ab', 'workgroup target of the generic weight gradient\'s split-K plan instead of the caller\'s '
                      '(192: R50 7.95 -> 7.88 ms; 160 level, 128 / 256 / 384 slower)'),
    'VFS_WGRAD_TBG_SMALL': (None, 'optional int', 'ab', '... a target of their own for layers with <= 4 tiles (large maps: the operands dwarf '
                            'the partials); measured level'),
    'VFS_WGRAD_TBG_DEEP': (None, 'optional int', 'ab', '... and for layers with >= 16 tiles (small maps: the partials rival the operands); '
                           'measured level'),
    'VFS_WGRAD_BATCH': ('0', 'flag', 'ab', 'split-K partials of all layers reduced by one table-driven launch per stage (measured slower)'),
    'VFS_STEM_FUSED': ('1', 'flag', 'ab', 'stem weight gradient with the BatchNorm-backward apply folded into its operand load; 0: materialise '
                       'dx, then the generic stem weight gradient'),
    'VFS_STEM_WGRAD_BLOCKS': ('1536', 'int', 'ab', 'workgroups of the fused stem weight gradient (~6 per CU: the operand gather is '
                              'latency-bound)'),
    'VFS_FAST_PACK': ('1', 'flag', 'ab', '16-byte tile variants of the weight packing for the aligned 1x1 / 3x3 shapes; 0: the generic 32x32 '
                      'tile for every tensor'),
    # data parallel
    'VFS_FORCE_COLLECTIVES': (None, 'flag', 'ab', 'run the collective code path in a 1-rank group (the RCCL calls, dtypes and stream ordering '
                              'of N > 1 on one GPU)'),
    'VFS_SYNCBN_P2P': ('1', 'choice: 0, 1, force', 'product', 'SyncBN statistics through the IPC-window exchange over xGMI; 0: '
                       'collective-library all-reduces; force: also in a 1-rank group (the exchange kernels\' cost on one GPU)'),
    'VFS_P2P_SPIN': (str(1 << 31), 'int', 'product', 'polls (~0.3 us each) before a kernel waiting for a peer\'s SyncBN statistics gives up and '
                     'sets the error word: ~10 minutes'),
    'VFS_P2P_CHECK_EVERY': ('50', 'int', 'product', 'optimizer steps between two looks at the sticky error word of the SyncBN exchange'),
    'VFS_GRAD_BF16': ('0', 'flag', 'product', 'bf16 gradient buckets for the data-parallel all-reduce: half the xGMI traffic (the reference '
                      'reduces fp32)'),
    'VFS_DDP_AVG': ('1', 'flag', 'ab', 'gradient buckets averaged by the collective itself (ReduceOp.AVG, RCCL backend only: one pass less '
                    'over the 153 MB gradient arena); 0: scale launch + SUM - same bits'),
    'VFS_DDP_SIDE': ('1', 'flag', 'ab', 'gradient buckets issued behind the weight-gradient stream; 0: the side stream is joined into the main '
                     'chain at every stage boundary (the dgrad chain then waits five times per step)'),
    # evaluation
    'VFS_EVAL_PRECISION': ('fp32', 'choice: fp32, bf16', 'product', 'evaluation path where test_cfg.precision / ResNet.eval_precision name '
                           'none: bit-defined fp32 kernels, or the bf16 kernels of the training path (about 3x faster)'),
    'VFS_LP_TWO_PASS': ('1', 'flag', 'ab', 'fp32 label propagation through the two-pass kernels (csrc/labelprop2.hip); 0: the dense kernel - '
                        'same bits'),
    'VFS_LP2_ENTRIES': ('0', 'int', 'product', 'candidate-list entries per query in the workspace of the two-pass label propagation where '
                        'test_cfg.lp2_entries names none (0: full capacity, 237 MB at 60 x 107)'),
    # the library
    'VFS_HIP_LIB': (None, 'str', 'ab', 'path of another build of the same ABI to load (A/B of two libraries); unset or empty: the built one'),
    'VFS_OPTS': ('', 'list', 'ab', '"name=value,...": the library\'s own A/B options, handed to vfs_set_option (include/vfs_hip_tuning.h)'),
    'VFS_TRACE_CALLS': (None, 'flag', 'debug', 'print the name of every entry point before it runs (with AMD_SERIALIZE_KERNEL=3 the last '
                        'line names a faulting launch)'),
    'VFS_DEBUG_SKIP': ('', 'list', 'debug', 'kernel families (Engine.timed labels) whose launches are dropped: the step time shows what the '
                       'family costs on the critical path (no kernel has data-dependent control flow) - results are garbage'),
    'VFS_DEBUG_NOMASK': (None, 'flag', 'debug', 'BatchNorm backward without reading the activation as ReLU mask (what-if timing) - WRONG '
                         'gradients'),
}


def _raw(name):
    return os.environ.get(name, TABLE[name][0])


def _parsed(conv, name):
    v = _raw(name)
    try:
        return conv(v)
    except ValueError:
        raise ValueError(f'{name}={v!r} is no {conv.__name__}') from None


def flag(name):
    """on if and only if the value is '1'"""
    return _raw(name) == '1'


def text(name):
    """the value of a str / choice knob as it stands (None: unset and no default)"""
    return _raw(name)


def integer(name):
    return _parsed(int, name)


def number(name):
    return _parsed(float, name)


def optional(name, otherwise=None):
    """int, or `otherwise` when the knob is unset"""
    return otherwise if _raw(name) is None else _parsed(int, name)


def items(name):
    """the non-empty entries of a comma list"""
    return [s for s in _raw(name).split(',') if s]


if __name__ == '__main__':
    print('| name | default | kind | class | effect |\n|---|---|---|---|---|')
    for name, (default, kind, cls, doc) in TABLE.items():
        print(f'| `{name}` | {"unset" if default is None else default or "empty"} | {kind} | {cls} | {doc} |')
