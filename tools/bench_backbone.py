"""Dev tool: time sparsebev_amd.ResNetBackbone (csrc/resnet.hip: 54 launches on v_mfma_f32_32x32x16_f16, BatchNorm folded) beside the
stand-in's ResNet-50 stages (tools/backbone_standin.py: nn.Conv2d + BatchNorm2d in eval mode, ReLU, add, channels-last, fp16 autocast,
MIOpen) on the same weights and images, and write one JSON line to profiles/backbone.json.

Shapes: 6 and 48 images of 3 x 256 x 704, fp16 NCHW in, the four fp16 channels-last stage maps out.  The two legs alternate in one process
after a warm-up; a figure is the median of three rounds' medians and every round is kept, so the spread is in the record.  FLOP are
counted by the plan (sbev_resnet_plan's multiply-adds, twice).  A third leg times uint8 images -> ImageFrontEnd -> ResNetBackbone ->
FPNNeck -> pyramid end to end.  Per-kernel times come from a ``rocprofv3 --kernel-trace --stats`` run of its own (a child process
running ``--launch-only``); the record also carries the compiler's register / scratch / LDS figures of resnet.hip beside fpn.hip's, and
the launch-by-launch errors against fp64 of tests/resnet_cases.py.

    python tools/bench_backbone.py [--iters 10] [--out profiles/backbone.json] [--no-trace]
    python tools/bench_backbone.py --resources-only          (no GPU needed: times are written as "NOT measured")
    python tools/bench_backbone.py --launch-only --images 6  (ten forwards of both legs and nothing else: the program beneath the profiler)
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
import torch.nn.functional as F               # noqa: E402

PEAK_F16_FLOPS = 2.5e15          # dense 16-bit matrix peak (MI355X_MICROARCH: ~2.5 PF)
DEV = 'cuda:0'
H, W = 256, 704
R50 = (3, 4, 6, 3)


def kernel_resources(unit):
    from sparsebev_amd.csrc import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build._hipcc()] + build.COMMON + build.UNITS[unit] + ['-Rpass-analysis=kernel-resource-usage', '-c', os.path.join(build.HERE, unit),
                                                                     '-o', os.path.join(tmp, 'unit.o')]
        text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    out, cur = {}, None
    keys = {'VGPRs': 'vgprs', 'AGPRs': 'agprs', 'ScratchSize [bytes/lane]': 'scratch_bytes_per_lane', 'LDS Size [bytes/block]': 'lds_bytes_per_block',
            'Occupancy [waves/SIMD]': 'occupancy_waves_per_simd'}
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


def standin_state(ref):
    """the stand-in's stem.* / stages.s.i.* entries under ResNetBackbone's names"""
    leaf = {'conv1': 'conv1', 'bn1': 'bn1', 'conv2': 'conv2', 'bn2': 'bn2', 'conv3': 'conv3', 'bn3': 'bn3', 'down.0': 'downsample.0',
            'down.1': 'downsample.1'}
    state = {}
    for k, v in ref.state_dict().items():
        m = re.match(r'stem\.([01])\.(.*)', k)
        if m:
            state[('conv1.' if m.group(1) == '0' else 'bn1.') + m.group(2)] = v
            continue
        m = re.match(r'stages\.(\d)\.(\d+)\.(down\.[01]|conv[123]|bn[123])\.(.*)', k)
        if m:
            state['layer%d.%s.%s.%s' % (int(m.group(1)) + 1, m.group(2), leaf[m.group(3)], m.group(4))] = v
    return state


def legs(n):
    import backbone_standin
    from sparsebev_amd import ResNetBackbone
    ref = backbone_standin.build(DEV)
    g = torch.Generator(device=DEV).manual_seed(n)
    with torch.no_grad():
        for m in ref.modules():                     # statistics and scales a trained net would have: the fold has work to do
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, device=DEV, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, device=DEV, generator=g))
                m.weight.copy_(0.5 + 0.5 * torch.rand(m.weight.shape, device=DEV, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, device=DEV, generator=g))
        for st in ref.stages:
            for b in st:
                b.bn3.weight.mul_(0.3)
    net = ResNetBackbone(depth=50).to(DEV)
    net.load_state_dict(standin_state(ref), strict=True)
    x = torch.randn(n, 3, H, W, device=DEV, generator=g).half()
    x_cl = x.contiguous(memory_format=torch.channels_last)
    out = [torch.empty(n, h, w, c, dtype=torch.float16, device=DEV).permute(0, 3, 1, 2) for c, h, w in net.plan(n, H, W)['outs']]

    def ours():
        return net(x, out=out)

    def torch_stages():
        with torch.autocast('cuda', dtype=torch.float16):
            y = ref.stem(x_cl)
            outs = []
            for st in ref.stages:
                y = st(y)
                outs.append(y)
            return outs

    return ours, torch_stages, net


def end_to_end(n):
    """uint8 images -> ImageFrontEnd -> ResNetBackbone -> FPNNeck -> the decoder's channels-last pyramid"""
    from sparsebev_amd import FPNNeck, ImageFrontEnd, ResNetBackbone
    front = ImageFrontEnd(dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True), out_dtype=torch.float16).to(DEV).eval()
    net = ResNetBackbone(depth=50).to(DEV)
    neck = FPNNeck([256, 512, 1024, 2048], 256, 4).to(DEV).eval()
    img = torch.randint(0, 256, (n, 3, H, W), dtype=torch.uint8, device=DEV)
    metas = [dict()]
    x = front(img, metas)
    stages = net(x)
    pyramid = neck(stages)

    def run():
        front(img, metas, out=x)
        net(x, out=stages)
        return neck(stages, out=pyramid)

    return run


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def bench_shape(n, iters):
    with torch.no_grad():
        ours, torch_stages, net = legs(n)
        whole = end_to_end(n)
        for _ in range(3):
            a, b = ours(), torch_stages()
            whole()
        torch.cuda.synchronize()
        # the two legs compute the same net: agreement to the fp16 roundings they do not share
        diff = [float((x.float() - y.float()).abs().max()) for x, y in zip(a, b)]
        scale = [float(y.float().abs().max()) for y in b]
        rounds = {'resnet_backbone': [], 'torch_stages': [], 'images_to_pyramid': []}
        for _ in range(3):
            for name, fn in (('resnet_backbone', ours), ('torch_stages', torch_stages), ('images_to_pyramid', whole)):
                rounds[name].append(statistics.median(timed(fn, iters) for _ in range(3)))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    p = net.plan(n, H, W)
    flop = 2 * p['macs']
    t = med['resnet_backbone'] * 1e-3
    return dict(images=n, launches=p['launches'], flop=flop, workspace_bytes=p['workspace_bytes'], pack_bytes=p['pack_bytes'],
                median_ms={k: round(v, 4) for k, v in med.items()}, rounds_ms={k: [round(x, 4) for x in v] for k, v in rounds.items()},
                spread={k: round((max(v) - min(v)) / statistics.median(v), 3) for k, v in rounds.items()},
                torch_over_resnet_backbone=round(med['torch_stages'] / med['resnet_backbone'], 3),
                resnet_backbone_TFLOPs=round(flop / t / 1e12, 1), resnet_backbone_fraction_of_f16_peak=round(flop / t / PEAK_F16_FLOPS, 4),
                torch_stages_fraction_of_f16_peak=round(flop / (med['torch_stages'] * 1e-3) / PEAK_F16_FLOPS, 4),
                max_abs_difference_between_legs_per_stage=diff, largest_output_per_stage=scale)


def launch_only(n):
    with torch.no_grad():
        ours, torch_stages, _ = legs(n)
        for _ in range(10):
            ours()
            torch_stages()
        torch.cuda.synchronize()


def kernel_trace(n):
    """per-kernel times of both legs from a rocprofv3 --kernel-trace --stats run of its own (a fresh child process)"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'backbone', '--', sys.executable,
               os.path.abspath(__file__), '--launch-only', '--images', str(n)]
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
    ours = [r for r in rows if 'resnet_' in r['name']]
    rest = [r for r in rows if 'resnet_' not in r['name']]
    # ten forwards of each leg: per-forward kernel time = total / 10 (the fold + pack launches run once, in the first forward)
    return dict(forwards=10, resnet_backbone_kernels=sorted(ours, key=lambda r: -r['total_us']),
                torch_kernels=sorted(rest, key=lambda r: -r['total_us'])[:12],
                resnet_backbone_kernel_us_per_forward=round(sum(r['total_us'] for r in ours if 'pack' not in r['name']) / 10, 1),
                torch_kernel_us_per_forward=round(sum(r['total_us'] for r in rest) / 10, 1))


def errors():
    """tests/test_gpu_resnet.py's whole-network check: the largest error / bound ratio per launch kind"""
    import resnet_cases as RC
    params = RC.real_params(R50, seed=5)
    x = torch.randn(2, 3, 40, 72, generator=torch.Generator().manual_seed(6))
    net = RC.make_backbone(R50, params, DEV)
    keep = []
    with torch.no_grad():
        net(x.to(DEV), keep=keep)
    worst = {}
    for r in RC.layer_errors(keep, x, params, R50):
        w = worst.setdefault(r['kind'], dict(launches=0, max_error=0.0, error_over_bound=0.0))
        w['launches'] += 1
        w['max_error'] = max(w['max_error'], float('%.3e' % r['max']))
        w['error_over_bound'] = max(w['error_over_bound'], round(r['ratio'], 4))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'backbone.json'))
    ap.add_argument('--images', type=int, default=6)
    ap.add_argument('--resources-only', action='store_true')
    ap.add_argument('--launch-only', action='store_true')
    ap.add_argument('--no-trace', action='store_true')
    a = ap.parse_args()
    if a.launch_only:
        return launch_only(a.images)
    res = {unit: kernel_resources(unit) for unit in ('resnet.hip', 'fpn.hip')}
    rec = {'tool': 'bench_backbone', 'kernel_resources': res,
           'scratch_free': all(v.get('scratch_bytes_per_lane') == 0 for unit in res.values() for v in unit.values()),
           'f16_peak_PFLOPs': PEAK_F16_FLOPS / 1e15}
    if a.resources_only or not torch.cuda.is_available():
        rec.update(device=None, shapes='NOT measured (no GPU run)', kernel_trace='NOT measured (no GPU run)', errors_vs_fp64='NOT measured (no GPU run)')
    else:
        prop = torch.cuda.get_device_properties(0)
        rec.update(device=torch.cuda.get_device_name(0), compute_units=prop.multi_processor_count, hip=torch.version.hip, torch=torch.__version__,
                   iters=a.iters, rounds=3, timing='HIP events, legs alternated in one process, median of the rounds\' medians',
                   shapes=[bench_shape(n, a.iters if n == 6 else max(3, a.iters // 4)) for n in (6, 48)],
                   kernel_trace='NOT measured (--no-trace)' if a.no_trace else {'images_%d' % n: kernel_trace(n) for n in (6, 48)},
                   errors_vs_fp64=errors())
    line = json.dumps(rec)
    print(line)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
