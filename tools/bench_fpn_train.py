"""Dev tool: time forward + backward of the trainable FPNNeck (csrc/fpn.hip + csrc/fpn_bwd.hip) beside torch's neck (nn.Conv2d laterals
and 3 x 3 output convolutions, interpolate + add, channels-last, fp16 autocast, ``.backward()``) on the same inputs, weights and output
gradients, and write one JSON line to profiles/fpn_backward.json.

Shapes: 6 and 48 images of the r50 pyramid of a 256 x 704 image, fp16 channels-last in, fp16 out, with and without input gradients.
The legs alternate in one process after a warm-up; a figure is the median of three rounds' medians and every round is kept.  Per-kernel
times come from a ``rocprofv3 --kernel-trace --stats`` run of its own (a child process running ``--launch-only``); the record also
carries the compiler's register / scratch / LDS figures of both translation units (the forward's must not move) and the largest
error / bound per stage of tests/test_gpu_fpn_bwd.py's stage-by-stage comparison against fp64.

    python tools/bench_fpn_train.py [--iters 10] [--out profiles/fpn_backward.json] [--no-trace]
    python tools/bench_fpn_train.py --resources-only          (no GPU needed: times are written as "NOT measured")
    python tools/bench_fpn_train.py --launch-only --images 6  (five steps of both legs and nothing else: the program beneath the profiler)
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch                                  # noqa: E402

import bench_fpn as BF                        # noqa: E402  (shapes, the torch neck, the timer)

DEV = BF.DEV
STEPS_UNDER_PROFILER = 5


def kernel_resources(unit):
    from sparsebev_amd.csrc import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build._hipcc()] + build.COMMON + build.UNITS[unit] + ['-Rpass-analysis=kernel-resource-usage', '-c', os.path.join(build.HERE, unit),
                                                                     '-o', os.path.join(tmp, 'unit.o')]
        text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    out, cur = {}, None
    keys = {'VGPRs': 'vgprs', 'AGPRs': 'agprs', 'ScratchSize [bytes/lane]': 'scratch_bytes_per_lane', 'LDS Size [bytes/block]': 'lds_bytes_per_block',
            'Occupancy [waves/SIMD]': 'occupancy_waves_per_simd', 'TotalSGPRs': 'sgprs'}
    for line in text.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = subprocess.run(['c++filt', m.group(1)], stdout=subprocess.PIPE).stdout.decode().strip() or m.group(1)
            name = re.sub(r'\(anonymous namespace\)::', '', name)
            cur = out.setdefault(re.sub(r'\(.*', '', name).replace('void ', ''), {})
            continue
        for k, v in keys.items():
            m = re.search(r'remark:\s+' + re.escape(k) + r': (\d+)', line)
            if m and cur is not None:
                cur[v] = int(m.group(1))
    return out


def counts(n, input_grads):
    """FLOP of one backward for n images, from the shapes: the 3x3 data and weight gradients, the lateral weight gradient, and the
    lateral data gradient when the inputs train"""
    px = [n * h * w for h, w in BF.PLANES]
    conv = sum(2 * p * 9 * 256 * 256 for p in px)
    lat = sum(2 * p * c * 256 for p, c in zip(px, BF.CIN))
    fwd = BF.counts(n)['flop']
    bwd = 2 * conv + lat + (lat if input_grads else 0)
    return dict(forward_flop=fwd, backward_flop=bwd, flop=fwd + bwd)


def legs(n, input_grads):
    from sparsebev_amd import FPNNeck
    g = torch.Generator(device=DEV).manual_seed(n)
    inputs = [torch.randn(n, h, w, c, device=DEV, generator=g).half().permute(0, 3, 1, 2).requires_grad_(input_grads) for c, (h, w) in zip(BF.CIN, BF.PLANES)]
    R = [(torch.randn(n, h, w, 256, device=DEV, generator=g) * 1e-3).half().permute(0, 3, 1, 2) for h, w in BF.PLANES]
    ref = BF.TorchNeck().to(DEV).train().to(memory_format=torch.channels_last)
    neck = FPNNeck(BF.CIN, 256, 4, trainable=True).to(DEV).train()
    state = {}
    for i in range(4):
        state['lateral_convs.%d.conv.weight' % i], state['lateral_convs.%d.conv.bias' % i] = ref.lateral[i].weight.detach().float(), ref.lateral[i].bias.detach().float()
        state['fpn_convs.%d.conv.weight' % i], state['fpn_convs.%d.conv.bias' % i] = ref.fpn[i].weight.detach().float(), ref.fpn[i].bias.detach().float()
    neck.load_state_dict(state, strict=True)

    def clear(module):
        module.zero_grad(set_to_none=True)
        for x in inputs:
            x.grad = None

    def ours():
        clear(neck)
        torch.autograd.backward(neck(inputs, out_dtype=torch.float16), R)
        return neck

    def ours_forward():
        with torch.no_grad():
            return neck(inputs, out_dtype=torch.float16)

    def torch_neck():
        clear(ref)
        with torch.autocast('cuda', dtype=torch.float16):
            outs = ref(inputs)
        torch.autograd.backward(outs, R)
        return ref

    return ours, torch_neck, ours_forward, inputs


def agreement(neck, ref, inputs, snapshot):
    """largest |difference| / largest |value| between the two legs' gradients (they share weights, inputs and output gradients; they
    differ by the fp16 roundings they do not share)"""
    out = {}
    pairs = [('fpn_convs.%d.weight' % i, neck.fpn_convs[i].conv.weight.grad, ref.fpn[i].weight.grad) for i in range(4)]
    pairs += [('lateral_convs.%d.weight' % i, neck.lateral_convs[i].conv.weight.grad, ref.lateral[i].weight.grad) for i in range(4)]
    pairs += [('fpn_convs.%d.bias' % i, neck.fpn_convs[i].conv.bias.grad, ref.fpn[i].bias.grad) for i in range(4)]
    pairs += [('lateral_convs.%d.bias' % i, neck.lateral_convs[i].conv.bias.grad, ref.lateral[i].bias.grad) for i in range(4)]
    for name, a, b in pairs:
        out[name] = float('%.3e' % (float((a.float() - b.float()).abs().max()) / max(float(b.float().abs().max()), 1e-30)))
    for i, (a, x) in enumerate(zip(snapshot, inputs)):
        if a is not None and x.grad is not None:
            out['input_%d' % i] = float('%.3e' % (float((a.float() - x.grad.float()).abs().max()) / max(float(x.grad.float().abs().max()), 1e-30)))
    return out


def bench_shape(n, iters, input_grads):
    with torch.enable_grad():
        ours, torch_neck, ours_forward, inputs = legs(n, input_grads)
        for _ in range(2):
            neck = ours()
        snapshot = [None if x.grad is None else x.grad.clone() for x in inputs]
        for _ in range(2):
            ref = torch_neck()
        torch.cuda.synchronize()
        agree = agreement(neck, ref, inputs, snapshot)
        ours()
        rounds = {'fpn_neck_step': [], 'torch_neck_step': [], 'fpn_neck_forward': []}
        for _ in range(3):
            for name, fn in (('fpn_neck_step', ours), ('torch_neck_step', torch_neck), ('fpn_neck_forward', ours_forward)):
                rounds[name].append(statistics.median(BF.timed(fn, iters) for _ in range(3)))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    c = counts(n, input_grads)
    t = med['fpn_neck_step'] * 1e-3
    return dict(images=n, input_grads=input_grads, **c, median_ms={k: round(v, 4) for k, v in med.items()},
                rounds_ms={k: [round(x, 4) for x in v] for k, v in rounds.items()},
                spread={k: round((max(v) - min(v)) / statistics.median(v), 3) for k, v in rounds.items()},
                fpn_neck_backward_ms=round(med['fpn_neck_step'] - med['fpn_neck_forward'], 4),
                torch_over_fpn_neck=round(med['torch_neck_step'] / med['fpn_neck_step'], 2), fpn_neck_TFLOPs=round(c['flop'] / t / 1e12, 1),
                fpn_neck_fraction_of_f16_peak=round(c['flop'] / t / BF.PEAK_F16_FLOPS, 3), relative_difference_between_legs=agree)


def launch_only(n):
    with torch.enable_grad():
        ours, torch_neck, _, _ = legs(n, True)
        for _ in range(STEPS_UNDER_PROFILER):
            ours()
            torch_neck()
        torch.cuda.synchronize()


def kernel_trace(n):
    """per-kernel times of both legs from a rocprofv3 --kernel-trace --stats run of its own (a fresh child process)"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'fpn', '--', sys.executable, os.path.abspath(__file__),
               '--launch-only', '--images', str(n)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        except (OSError, subprocess.TimeoutExpired) as e:
            return 'NOT measured (%s)' % e
        files = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        if p.returncode != 0 or not files:
            return 'NOT measured (rocprofv3 exit %d: %s)' % (p.returncode, p.stdout.decode(errors='replace')[-300:])
        rows = []
        with open(files[0]) as f:
            for r in csv.DictReader(f):
                rows.append(dict(name=re.sub(r'\(anonymous namespace\)::', '', r.get('Name', ''))[:120], calls=int(r.get('Calls', 0)),
                                 average_us=round(float(r.get('AverageNs', 0)) / 1e3, 2), total_us=round(float(r.get('TotalDurationNs', 0)) / 1e3, 1)))
    ours = [r for r in rows if 'fpn_' in r['name'] or 'grad_scale_' in r['name']]      # grad_scale.hip: the scale's two kernels, shared with the backbone
    rest = [r for r in rows if r not in ours]
    k = STEPS_UNDER_PROFILER
    return dict(steps=k, input_grads=True, fpn_neck_kernels=sorted(ours, key=lambda r: -r['total_us']),
                torch_kernels=sorted(rest, key=lambda r: -r['total_us'])[:14],
                fpn_neck_kernel_us_per_step=round(sum(r['total_us'] for r in ours if 'pack' not in r['name']) / k, 1),
                torch_kernel_us_per_step=round(sum(r['total_us'] for r in rest) / k, 1))


def errors():
    """largest error / bound per stage over every case and dtype pair of the stage-by-stage test"""
    import fpn_bwd_cases as BC
    import fpn_cases as FC
    import test_gpu_fpn_bwd as T
    worst = {}
    for case in FC.CASES:
        xs, params, gP = T.real_case(case.name)
        neck = BC.make_trainable_neck(case, params, DEV)
        for in_dtype, g_dtype in T.DTYPES:
            run = BC.DeviceBackward(neck, case, xs, gP, in_dtype, g_dtype, DEV)
            for stage, ratio in T.stage_rows(run, case, xs, params, gP, in_dtype, g_dtype):
                key = stage.rstrip('0123456789_')
                worst[key] = max(worst.get(key, 0.0), round(ratio, 4))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fpn_backward.json'))
    ap.add_argument('--images', type=int, default=6)
    ap.add_argument('--resources-only', action='store_true')
    ap.add_argument('--launch-only', action='store_true')
    ap.add_argument('--no-trace', action='store_true')
    a = ap.parse_args()
    if a.launch_only:
        return launch_only(a.images)
    res = {unit: kernel_resources(unit) for unit in ('fpn.hip', 'fpn_bwd.hip')}
    rec = {'tool': 'bench_fpn_train', 'kernel_resources': res,
           'scratch_free': all(v.get('scratch_bytes_per_lane') == 0 for unit in res.values() for v in unit.values()),
           'f16_peak_PFLOPs': BF.PEAK_F16_FLOPS / 1e15}
    # the forward kernels' figures recorded on the commit before the helpers moved to fpn_common.hpp travel with the record
    committed = os.path.join(ROOT, 'profiles', 'fpn_backward.json')
    if os.path.exists(committed):
        with open(committed) as f:
            parent = json.loads(f.readline()).get('forward_kernel_resources_parent')
        if parent is not None:
            rec.update(forward_kernel_resources_parent=parent, forward_kernels_unchanged=parent == res['fpn.hip'])
    if a.resources_only or not torch.cuda.is_available():
        rec.update(device=None, shapes='NOT measured (no GPU run)', kernel_trace='NOT measured (no GPU run)',
                   largest_error_over_bound_per_stage='NOT measured (no GPU run)')
    else:
        prop = torch.cuda.get_device_properties(0)
        rec.update(device=torch.cuda.get_device_name(0), compute_units=prop.multi_processor_count, hip=torch.version.hip, torch=torch.__version__,
                   iters=a.iters, rounds=3, timing='HIP events, legs alternated in one process, median of the rounds\' medians',
                   shapes=[bench_shape(n, a.iters if n == 6 else max(3, a.iters // 3), ig) for n in (6, 48) for ig in (True, False)],
                   kernel_trace='NOT measured (--no-trace)' if a.no_trace else {'images_%d' % n: kernel_trace(n) for n in (6, 48)},
                   largest_error_over_bound_per_stage=errors())
    line = json.dumps(rec)
    print(line)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
