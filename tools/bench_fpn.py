"""Dev tool: time sparsebev_amd.FPNNeck (csrc/fpn.hip: L + 1 launches on v_mfma_f32_32x32x16_f16) beside the stand-in's neck layers
(tools/backbone_standin.py: nn.Conv2d laterals and 3 x 3 output convolutions, interpolate + add, channels-last, fp16 autocast, MIOpen) on
identical inputs, and write one JSON line to profiles/fpn_neck.json.

Shapes: 6 and 48 images of the r50 pyramid of a 256 x 704 image (64 x 176, 32 x 88, 16 x 44, 8 x 22; 256 / 512 / 1024 / 2048 channels),
fp16 channels-last in, fp16 out.  The two legs alternate in one process after a warm-up; a figure is the median of three rounds' medians
and every round is kept, so the spread is in the record.  FLOP and bytes are counted from the shapes (bytes: every input read once,
the merged laterals written and read once, every output written once, the weight image once).  Per-kernel times come from a
``rocprofv3 --kernel-trace --stats`` run of its own (a child process running ``--launch-only``); the record also carries the compiler's
register / scratch / LDS figures and the stage-by-stage errors against fp64 of tests/fpn_cases.py's cases.

    python tools/bench_fpn.py [--iters 20] [--out profiles/fpn_neck.json] [--no-trace]
    python tools/bench_fpn.py --resources-only          (no GPU needed: times are written as "NOT measured")
    python tools/bench_fpn.py --launch-only --images 6  (ten forwards of both legs and nothing else: the program beneath the profiler)
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
import torch                                  # noqa: E402
import torch.nn as nn                         # noqa: E402
import torch.nn.functional as F               # noqa: E402

CIN = [256, 512, 1024, 2048]
PLANES = [(64, 176), (32, 88), (16, 44), (8, 22)]
PEAK_F16_FLOPS = 2.5e15          # dense 16-bit matrix peak (MI355X_MICROARCH: ~2.5 PF)
DEV = 'cuda:0'


def kernel_resources():
    from sparsebev_amd.csrc import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build._hipcc()] + build.COMMON + build.UNITS['fpn.hip'] + ['-Rpass-analysis=kernel-resource-usage', '-c',
                                                                          os.path.join(build.HERE, 'fpn.hip'), '-o', os.path.join(tmp, 'unit.o')]
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


def counts(n):
    """FLOP and bytes of one forward for n images, from the shapes"""
    px = [n * h * w for h, w in PLANES]
    lat = sum(2 * p * c * 256 for p, c in zip(px, CIN))
    conv = sum(2 * p * 9 * 256 * 256 for p in px)
    weights = (sum(CIN) * 256 + len(CIN) * 9 * 256 * 256) * 2
    moved = sum(p * c * 2 for p, c in zip(px, CIN)) + sum(p * 256 * 2 for p in px) * 3 + weights
    return dict(pixels=sum(px), lateral_flop=lat, conv_flop=conv, flop=lat + conv, bytes=moved)


class TorchNeck(nn.Module):
    """the neck layers of tools/backbone_standin.py::ResNet50FPN"""

    def __init__(self):
        super().__init__()
        self.lateral = nn.ModuleList(nn.Conv2d(c, 256, 1) for c in CIN)
        self.fpn = nn.ModuleList(nn.Conv2d(256, 256, 3, padding=1) for _ in CIN)

    def forward(self, outs):
        lat = [l(o) for l, o in zip(self.lateral, outs)]
        for i in range(len(lat) - 1, 0, -1):
            lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[-2:], mode='nearest')
        return [f(l) for f, l in zip(self.fpn, lat)]


def legs(n):
    from sparsebev_amd import FPNNeck
    g = torch.Generator(device=DEV).manual_seed(n)
    inputs = [torch.randn(n, h, w, c, device=DEV, generator=g).half().permute(0, 3, 1, 2) for c, (h, w) in zip(CIN, PLANES)]
    ref = TorchNeck().to(DEV).eval().to(memory_format=torch.channels_last)
    neck = FPNNeck(CIN, 256, 4).to(DEV).eval()
    state = {}
    for i in range(4):
        state['lateral_convs.%d.conv.weight' % i], state['lateral_convs.%d.conv.bias' % i] = ref.lateral[i].weight.detach().float(), ref.lateral[i].bias.detach().float()
        state['fpn_convs.%d.conv.weight' % i], state['fpn_convs.%d.conv.bias' % i] = ref.fpn[i].weight.detach().float(), ref.fpn[i].bias.detach().float()
    neck.load_state_dict(state, strict=True)
    out = [torch.empty(n, h, w, 256, dtype=torch.float16, device=DEV).permute(0, 3, 1, 2) for h, w in PLANES]

    def ours():
        return neck(inputs, out=out)

    def torch_neck():
        with torch.autocast('cuda', dtype=torch.float16):
            return ref(inputs)

    return ours, torch_neck


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
        ours, torch_neck = legs(n)
        for _ in range(3):
            a, b = ours(), torch_neck()
        torch.cuda.synchronize()
        # the two legs compute the same neck: agreement to the fp16 roundings they do not share
        diff = max(float((x.float() - y.float()).abs().max()) for x, y in zip(a, b))
        scale = max(float(y.float().abs().max()) for y in b)
        rounds = {'fpn_neck': [], 'torch_neck': []}
        for _ in range(3):
            for name, fn in (('fpn_neck', ours), ('torch_neck', torch_neck)):
                rounds[name].append(statistics.median(timed(fn, iters) for _ in range(3)))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    c = counts(n)
    t = med['fpn_neck'] * 1e-3
    return dict(images=n, **c, median_ms={k: round(v, 4) for k, v in med.items()}, rounds_ms={k: [round(x, 4) for x in v] for k, v in rounds.items()},
                spread={k: round((max(v) - min(v)) / statistics.median(v), 3) for k, v in rounds.items()},
                torch_over_fpn_neck=round(med['torch_neck'] / med['fpn_neck'], 2), fpn_neck_TFLOPs=round(c['flop'] / t / 1e12, 1),
                fpn_neck_fraction_of_f16_peak=round(c['flop'] / t / PEAK_F16_FLOPS, 3), fpn_neck_TBps=round(c['bytes'] / t / 1e12, 2),
                max_abs_difference_between_legs=diff, largest_output=scale)


def launch_only(n):
    with torch.no_grad():
        ours, torch_neck = legs(n)
        for _ in range(10):
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
    ours = [r for r in rows if 'fpn_' in r['name']]
    rest = [r for r in rows if 'fpn_' not in r['name']]
    # ten forwards of each leg: per-forward kernel time = total / 10 (the pack launches run once, in the first forward)
    return dict(forwards=10, fpn_neck_kernels=ours, torch_kernels=sorted(rest, key=lambda r: -r['total_us'])[:12],
                fpn_neck_kernel_us_per_forward=round(sum(r['total_us'] for r in ours if 'pack' not in r['name']) / 10, 1),
                torch_kernel_us_per_forward=round(sum(r['total_us'] for r in rest) / 10, 1))


def errors():
    import fpn_cases as FC
    out = {}
    with torch.no_grad():
        for case in FC.CASES:
            xs, params = FC.real_data(case, seed=5)
            neck = FC.make_neck(case, params, DEV)
            for in_dtype, out_dtype in ((torch.float16, torch.float16), (torch.float32, torch.float32)):
                rows = FC.stage_errors(neck, case, xs, params, in_dtype, out_dtype, DEV)
                out['%s %s->%s' % (case.name, str(in_dtype)[6:], str(out_dtype)[6:])] = [
                    dict(stage=r['stage'], max=float('%.3e' % r['max']), rms=float('%.3e' % r['rms']), error_over_bound=round(r['ratio'], 4)) for r in rows]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fpn_neck.json'))
    ap.add_argument('--images', type=int, default=6)
    ap.add_argument('--resources-only', action='store_true')
    ap.add_argument('--launch-only', action='store_true')
    ap.add_argument('--no-trace', action='store_true')
    a = ap.parse_args()
    if a.launch_only:
        return launch_only(a.images)
    res = kernel_resources()
    rec = {'tool': 'bench_fpn', 'kernel_resources': res, 'scratch_free': all(v.get('scratch_bytes_per_lane') == 0 for v in res.values()),
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
