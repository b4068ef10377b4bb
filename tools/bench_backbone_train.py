"""Dev tool: time forward + backward of the trainable ResNetBackbone (csrc/resnet.hip + csrc/resnet_bwd.hip, frozen_stages=1: the
reference recipe) beside torch's stages (tools/backbone_standin.py: nn.Conv2d + BatchNorm2d in eval mode, channels-last, fp16 autocast,
``.backward()``, stem and stage 1 frozen) on the same weights, images and output gradients, and write one JSON line to
profiles/backbone_backward.json.

Shapes: 6 and 48 images of 3 x 256 x 704, fp16 NCHW in, fp16 channels-last output gradients.  The legs alternate in one process after a
warm-up; a figure is the median of three rounds' medians and every round is kept.  A third leg times the trainable forward alone, a fourth
images -> ImageFrontEnd -> ResNetBackbone -> FPNNeck(trainable=True) forward and backward.  Per-kernel times come from a ``rocprofv3
--kernel-trace --stats`` run of its own (a child process running ``--launch-only``).  The record carries the compiler's register / scratch
/ LDS figures of resnet_bwd.hip, resnet.hip's beside the ones profiles/backbone.json recorded for the forward (the forward's kernels are
untouched), the planned bytes, and tests/test_gpu_resnet_bwd.py's largest error / bound per kernel family with the scaled-domain amax range.

    python tools/bench_backbone_train.py [--iters 10] [--out profiles/backbone_backward.json] [--no-trace]
    python tools/bench_backbone_train.py --resources-only          (no GPU needed: times are written as "NOT measured")
    python tools/bench_backbone_train.py --launch-only --images 6  (ten steps of both legs and nothing else: the program beneath the profiler)
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

import bench_backbone as BB                   # noqa: E402

DEV, H, W = BB.DEV, BB.H, BB.W
FROZEN = 1


def legs(n):
    import backbone_standin
    from sparsebev_amd import ResNetBackbone
    ref = backbone_standin.build(DEV)
    g = torch.Generator(device=DEV).manual_seed(n)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, device=DEV, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, device=DEV, generator=g))
                m.weight.copy_(0.5 + 0.5 * torch.rand(m.weight.shape, device=DEV, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, device=DEV, generator=g))
        for st in ref.stages:
            for b in st:
                b.bn3.weight.mul_(0.3)
    for p in ref.parameters():
        p.requires_grad_(False)
    for st in list(ref.stages)[FROZEN:]:
        for p in st.parameters():
            p.requires_grad_(True)
    net = ResNetBackbone(depth=50, trainable=True, frozen_stages=FROZEN).to(DEV)
    net.load_state_dict(BB.standin_state(ref), strict=True)
    x = torch.randn(n, 3, H, W, device=DEV, generator=g).half()
    x_cl = x.contiguous(memory_format=torch.channels_last)
    gouts = [(1e-3 * torch.randn(n, h, w, c, device=DEV, generator=g)).half().permute(0, 3, 1, 2) for c, h, w in net.plan(n, H, W)['outs']]
    ours_params = [p for p in net.parameters() if p.requires_grad]
    ref_params = [p for p in ref.parameters() if p.requires_grad]

    def ours():
        for p in ours_params:
            p.grad = None
        torch.autograd.backward(net(x), gouts)

    def ours_forward():
        return net(x)

    def torch_stages():
        for p in ref_params:
            p.grad = None
        with torch.autocast('cuda', dtype=torch.float16):
            y = ref.stem(x_cl)
            outs = []
            for st in ref.stages:
                y = st(y)
                outs.append(y)
        live = [(o, g) for o, g in zip(outs, gouts) if o.requires_grad]          # the frozen stage's map has no graph behind it
        torch.autograd.backward([o for o, _ in live], [g for _, g in live])

    return ours, ours_forward, torch_stages, net, ref


def end_to_end(n):
    """uint8 images -> ImageFrontEnd -> ResNetBackbone -> FPNNeck(trainable=True), forward and backward"""
    from sparsebev_amd import FPNNeck, ImageFrontEnd, ResNetBackbone
    front = ImageFrontEnd(dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True), out_dtype=torch.float16).to(DEV).eval()
    net = ResNetBackbone(depth=50, trainable=True, frozen_stages=FROZEN).to(DEV)
    neck = FPNNeck([256, 512, 1024, 2048], 256, 4, trainable=True).to(DEV)
    img = torch.randint(0, 256, (n, 3, H, W), dtype=torch.uint8, device=DEV)
    metas = [dict()]
    with torch.no_grad():
        x = front(img, metas)
    with torch.enable_grad():
        pyramid = neck(net(x))
    gP = [1e-3 * torch.randn_like(p) for p in pyramid]
    params = [p for p in list(net.parameters()) + list(neck.parameters()) if p.requires_grad]

    def run():
        for p in params:
            p.grad = None
        with torch.no_grad():
            front(img, metas, out=x)
        torch.autograd.backward(neck(net(x)), gP)

    return run


def bench_shape(n, iters):
    with torch.enable_grad():
        ours, ours_forward, torch_stages, net, ref = legs(n)
        whole = end_to_end(n)
        for _ in range(3):
            ours()
            torch_stages()
            whole()
        torch.cuda.synchronize()
        # the two legs compute the same gradients: agreement to the fp16 roundings they do not share
        names = ('layer2.0.conv2.weight', 'layer3.3.bn2.weight', 'layer4.2.conv3.weight', 'layer4.0.downsample.1.bias')
        mine = dict(net.named_parameters())
        by_ptr = {p.data_ptr(): p for p in ref.parameters()}
        theirs = {k: by_ptr[v.data_ptr()] for k, v in BB.standin_state(ref).items() if v.data_ptr() in by_ptr}
        agreement = {}
        for k in names:
            a, b = mine[k].grad.float(), theirs[k].grad.float()
            agreement[k] = dict(max_abs_difference=float((a - b).abs().max()), largest=float(b.abs().max()))
        legs_ = (('resnet_forward_backward', ours), ('torch_forward_backward', torch_stages), ('resnet_forward_train', ours_forward),
                 ('images_to_pyramid_forward_backward', whole))
        rounds = {k: [] for k, _ in legs_}
        for _ in range(3):
            for name, fn in legs_:
                rounds[name].append(statistics.median(BB.timed(fn, iters) for _ in range(3)))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    p, bp = net.plan(n, H, W), net.backward_plan(n, H, W)
    return dict(images=n, forward_launches=p['launches'], backward_launches=bp['launches'], kept_activation_bytes=bp['acts_bytes'],
                backward_workspace_bytes=bp['workspace_bytes'], backward_pack_bytes=bp['pack_bytes'], forward_workspace_bytes=p['workspace_bytes'],
                median_ms={k: round(v, 4) for k, v in med.items()}, rounds_ms={k: [round(x, 4) for x in v] for k, v in rounds.items()},
                spread={k: round((max(v) - min(v)) / statistics.median(v), 3) for k, v in rounds.items()},
                resnet_backward_ms=round(med['resnet_forward_backward'] - med['resnet_forward_train'], 4),
                backward_over_forward=round((med['resnet_forward_backward'] - med['resnet_forward_train']) / med['resnet_forward_train'], 3),
                torch_over_resnet=round(med['torch_forward_backward'] / med['resnet_forward_backward'], 3),
                gradient_agreement_between_legs=agreement)


def launch_only(n):
    with torch.enable_grad():
        ours, _, torch_stages, _, _ = legs(n)
        for _ in range(10):
            ours()
            torch_stages()
        torch.cuda.synchronize()


def kernel_trace(n):
    """per-kernel times of both legs from a rocprofv3 --kernel-trace --stats run of its own (a fresh child process)"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'backbone_train', '--', sys.executable,
               os.path.abspath(__file__), '--launch-only', '--images', str(n)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=400)
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
    backward = lambda r: 'rb_' in r['name'] or 'grad_scale_' in r['name']      # grad_scale.hip: the scale's two kernels, shared with the neck
    ours = [r for r in rows if 'resnet_' in r['name'] or backward(r)]
    rest = [r for r in rows if r not in ours]
    steps = lambda rs: round(sum(r['total_us'] for r in rs if 'pack' not in r['name']) / 10, 1)
    return dict(steps=10, resnet_kernels=sorted(ours, key=lambda r: -r['total_us']), torch_kernels=sorted(rest, key=lambda r: -r['total_us'])[:16],
                resnet_forward_kernel_us_per_step=steps([r for r in ours if 'resnet_' in r['name']]),
                resnet_backward_kernel_us_per_step=steps([r for r in ours if backward(r)]),
                torch_kernel_us_per_step=round(sum(r['total_us'] for r in rest) / 10, 1))


def errors():
    """tests/test_gpu_resnet_bwd.py's operation-by-operation check: the largest error / bound per kernel family, the scaled-domain amax range"""
    import test_gpu_resnet_bwd as T
    out = {}
    for frozen in (1, 0):
        ratios, amax = T.operation_errors(frozen)
        out['frozen_stages_%d' % frozen] = dict(error_over_bound={k: round(v, 4) for k, v in sorted(ratios.items())},
                                                scaled_amax_largest=max(amax.values()), scaled_amax_smallest=min(amax.values()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'backbone_backward.json'))
    ap.add_argument('--images', type=int, default=6)
    ap.add_argument('--resources-only', action='store_true')
    ap.add_argument('--launch-only', action='store_true')
    ap.add_argument('--no-trace', action='store_true')
    a = ap.parse_args()
    if a.launch_only:
        return launch_only(a.images)
    res = {unit: BB.kernel_resources(unit) for unit in ('resnet_bwd.hip', 'resnet.hip')}
    with open(os.path.join(ROOT, 'profiles', 'backbone.json')) as f:
        before = json.loads(f.readline())['kernel_resources']['resnet.hip']
    from sparsebev_amd import resnet
    planned = {'images_%d' % n: {k: v for k, v in resnet.backward_plan(50, n, H, W, first_trainable_stage=FROZEN + 1).items() if k != 'layers'}
               for n in (6, 48)}
    rec = {'tool': 'bench_backbone_train', 'frozen_stages': FROZEN, 'kernel_resources': res,
           'forward_kernel_resources_in_profiles_backbone_json': before, 'forward_kernel_resources_unchanged': before == res['resnet.hip'],
           'scratch_free': all(v.get('scratch_bytes_per_lane') == 0 for unit in res.values() for v in unit.values()), 'planned': planned}
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
