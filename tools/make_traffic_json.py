#!/usr/bin/env python3
"""gpurun_out/pmc_<model>.json (tools/gpu_pmc.sh: per-kernel FETCH_SIZE / WRITE_SIZE sums) ->
profiles/<tag>_traffic_<model>.json: HBM bytes per kernel launch and per bench.py roofline class.

Units / corrections as MI355X_MICROARCH.md prescribes: the counters are KiB; on gfx950 FETCH_SIZE
tallies the 128-byte read requests at 64 bytes, so fetched bytes = 2 x FETCH_SIZE x 1024."""
import json
import os
import sys

CLASSES = {   # bench.py's Engine.timed() classes (= kernel families) -> kernels launched under them
    'conv_igemm': ('conv_igemm_kernel', 'conv_skinny_kernel', 'conv_pw_kernel', 'linear_bn_act_kernel'),
    'conv3x3_halo': ('conv3x3_halo_kernel',),
    'stem_fwd': ('stem_fwd_direct_kernel',),
    'conv_wgrad': ('conv_wgrad_kernel', 'conv_wgrad_ring_kernel'),          # (the table-driven reduction of the partials is its own class)
    'conv3x3_wgrad_halo': ('conv3x3_wgrad_halo_kernel',),
    'stem_wgrad': ('stem_wgrad_fused_kernel',),
    'wgrad_reduce': ('wgrad_reduce_',),
    'bn_act': ('bn_act_kernel',),
    'bn_bwd_apply': ('bn_bwd_apply_kernel',),
    'bn_bwd_reduce': ('bn_bwd_reduce_kernel', 'stem_pool_bn_bwd_reduce'),
    'bn_stats': ('bn_reduce_', 'bn_stats_raw', 'bn_finalize'),
    'bn_relu_maxpool': ('bn_relu_maxpool_kernel',),
    'pack_weights': ('pack_weights_kernel',),
    'sgd': ('sgd_kernel',),
    # the fp32 DAVIS workload (bench.py --workload davis; `make_traffic_json.py davis_<model> <tag>`)
    'labelprop_f32': ('labelprop_f32_kernel', 'labelprop_f32_merge_kernel'),
    'labelprop_2pass': ('lp2_score_kernel', 'lp2_refine_kernel', 'lp2_seed_kernel'),
    'conv_f32': ('conv_f32_kernel', 'conv_f32_db_kernel'),
    'seg_postprocess': ('seg_minmax_exact_kernel', 'seg_argmax_exact_kernel'),
}
# families whose timed launch is SEVERAL kernels: bytes of all of them per launch of the first one
LAUNCH_KERNEL = {'labelprop_f32': 'labelprop_f32_kernel', 'labelprop_2pass': 'lp2_score_kernel', 'seg_postprocess': 'seg_minmax_exact_kernel'}
NOT_A_LAUNCH = ()


def aggregate(kernels):
    classes = {}
    for cls, names in CLASSES.items():
        tot, launches = 0.0, 0
        for k, v in kernels.items():
            if any(n in k for n in names):
                tot += (v['fetch_bytes_per_launch'] + v['write_bytes_per_launch']) * v['calls']
                if cls not in LAUNCH_KERNEL or LAUNCH_KERNEL[cls] in k:
                    launches += v['calls']
        if launches:
            classes[cls] = {'launches': launches, 'hbm_bytes_per_launch': tot / launches}
    return classes


def main():
    if sys.argv[1] == '--reaggregate':      # recompute the class table of existing files from their per-kernel entries
        for path in sys.argv[2:]:
            d = json.load(open(path))
            d['classes'] = aggregate(d['kernels'])
            json.dump(d, open(path, 'w'), indent=1)
            print(path, json.dumps(d['classes']))
        return
    model, tag = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else 'r02')
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = json.load(open(os.path.join(repo, 'gpurun_out', f'pmc_{model}.json')))
    kernels = {}
    for name, v in raw.get('FETCH_SIZE', {}).items():
        w = raw.get('WRITE_SIZE', {}).get(name, {'sum': 0.0, 'calls': v['calls']})
        kernels[name] = {'calls': v['calls'], 'fetch_bytes_per_launch': 2.0 * v['sum'] * 1024 / v['calls'],
                         'write_bytes_per_launch': w['sum'] * 1024 / max(w['calls'], 1)}
    classes = aggregate(kernels)
    cmd = (f'bench.py --workload davis --model {model[6:]} --precision fp32 --steps 49 --warmup 0 --full` (tools/gpu_pmc.sh {model[6:]} davis: '
           'every launch of the warm-up, the untimed and the timed pass over the 31-frame clip)' if model.startswith('davis_') else
           f'bench.py --model {model.split("_")[0]} --steps 3 --warmup 1' + (f' --size {model.split("_")[1]}' if '_' in model else '') + '` (tools/gpu_pmc.sh; default schedule: command-tape replay, weight gradients on the side stream)')
    out = {'source': 'rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes, --kernel-trace only) on `' + cmd + '; '
                     'counters are KiB; FETCH_SIZE doubled per MI355X_MICROARCH.md (gfx950 tallies 128-B requests at 64 B)',
           'kernels': kernels, 'classes': classes}
    # the whole train step: every kernel's bytes / the number of backward passes the run executed (one cosine_loss_bwd each;
    # the two recording passes have no optimizer step, the difference is < 1 %)
    passes = sum(v['calls'] for k, v in kernels.items() if 'cosine_loss_bwd' in k)
    if passes and not model.startswith('davis_'):
        out['passes'] = passes
        out['step_total_bytes'] = sum((v['fetch_bytes_per_launch'] + v['write_bytes_per_launch']) * v['calls'] for v in kernels.values()) / passes
    path = os.path.join(repo, 'profiles', f'{tag}_traffic_{model}.json')
    json.dump(out, open(path, 'w'), indent=1)
    print(path, json.dumps(classes))


if __name__ == '__main__':
    main()
