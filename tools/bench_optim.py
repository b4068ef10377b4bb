"""Dev tool: time sparsebev_amd.optim.FusedAdamW (csrc/optim.hip) and write one JSON line to profiles/optim_step.json.

(a) The three launches on the training head's real parameter list (Q = 900, T = 8: 51 tensors, ~17.7 M elements), interleaved in one
    process with torch.nn.utils.clip_grad_norm_(foreach=True) + torch.optim.AdamW(fused=True, capturable=True) on a twin list; medians
    of three rounds.  The update launch is also timed alone and reported as bytes / time (28 bytes per element) and as a fraction of
    the 6.29 TB/s float4 copy rate measured for this part.
(b) The captured head step (train_graph.CapturedHeadTrainStep, B = 1, 40 boxes, capacity 40 -- tools/bench_head_train.py --captured's
    shape): with the optimizer inside the graph, with torch's optimizer after replay(), and without any optimizer.
The record also carries the compiler's register / scratch / LDS figures of the three kernels.  Nothing here is a gate.

    python tools/bench_optim.py [--steps 30] [--out profiles/optim_step.json]
    python tools/bench_optim.py --resources-only          (no GPU needed)
"""
import argparse
import copy
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s, float4 copy on one MI355X


def kernel_resources():
    from sparsebev_amd.csrc import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build._hipcc()] + build.COMMON + build.UNITS['optim.hip'] + ['-Rpass-analysis=kernel-resource-usage', '-c',
                                                                            os.path.join(build.HERE, 'optim.hip'), '-o', os.path.join(tmp, 'unit.o')]
        text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    out, cur = {}, None
    keys = {'VGPRs': 'vgprs', 'TotalSGPRs': 'sgprs', 'ScratchSize [bytes/lane]': 'scratch_bytes_per_lane', 'LDS Size [bytes/block]': 'lds_bytes_per_block'}
    for line in text.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = subprocess.run(['c++filt', m.group(1)], stdout=subprocess.PIPE).stdout.decode().strip() or m.group(1)
            cur = out.setdefault((re.findall(r'(\w+)\(', name) or [name])[0], {})
            continue
        for k, v in keys.items():
            m = re.search(r'remark:\s+' + re.escape(k) + r': (\d+)', line)
            if m and cur is not None:
                cur[v] = int(m.group(1))
    return out


def timed(fn, inner=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def make_head(a, sizes, **kw):
    from sparsebev_amd import synthetic as S
    from sparsebev_amd.head_train import SparseBEVTrainHead
    return SparseBEVTrainHead(num_classes=10, in_channels=256, num_query=a.q, query_denoising_groups=a.groups, code_size=10,
                              code_weights=[2.0, 2.0] + [1.0] * 8,
                              transformer=dict(type='SparseBEVTransformer', embed_dims=256, num_frames=a.t, num_points=4, num_layers=6,
                                               num_levels=len(sizes), num_classes=10, code_size=10, pc_range=S.PC_RANGE),
                              bbox_coder=dict(type='NMSFreeCoder', post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_num=300,
                                              num_classes=10, pc_range=S.PC_RANGE), assign_on='device', **kw)


RECIPE = dict(lr=2e-4, weight_decay=0.01)
KEYS = {'sampling_offset': dict(lr_mult=0.1)}


def torch_optimizer(named):
    from sparsebev_amd import optim
    groups = [{k: v for k, v in g.items() if k != 'names'} for g in optim.param_groups(named, 2e-4, 0.01, KEYS)]
    return torch.optim.AdamW(groups, fused=True, capturable=True, **RECIPE)


def launches(a, head):
    """(a): the optimizer step alone on the head's parameter list"""
    import ctypes
    from sparsebev_amd import _lib, optim
    dev = 'cuda:0'
    twin = copy.deepcopy(head)
    gen = torch.Generator(device=dev).manual_seed(0)
    for m in (head, twin):
        for p in m.parameters():
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-2
    opt = optim.FusedAdamW(optim.param_groups(head.named_parameters(), 2e-4, 0.01, KEYS), max_grad_norm=35.0, loss_scale=512.0, **RECIPE)
    topt = torch_optimizer(twin.named_parameters())
    tparams = [p for p in twin.parameters() if p.requires_grad]
    numel = sum(p.numel() for p, _ in opt._params())
    opt.step()
    lib = _lib.load()
    VP = ctypes.c_void_p

    def update_only():
        stream = VP(torch.cuda.current_stream().cuda_stream)
        b1, b2 = opt.param_groups[0]['betas']
        for t in opt._tables:
            _lib.check(lib.sbev_optim_adamw(t['p'], t['g'], t['m'], t['v'], t['numel'], t['group'], t['n'], len(opt.param_groups), b1, b2,
                                            opt.param_groups[0]['eps'], VP(opt._hyper.data_ptr()), VP(opt._header.data_ptr()), stream), 'sbev_optim_adamw')

    def torch_step():
        torch.nn.utils.clip_grad_norm_(tparams, 35.0, foreach=True)
        topt.step()

    legs = {'fused_step': opt.enqueue, 'fused_update_launch': update_only, 'torch_clip_plus_adamw_fused': torch_step}
    rounds = {k: [] for k in legs}
    for _ in range(3):
        times = {k: [] for k in legs}
        for i in range(a.warmup + a.steps):
            for k, fn in legs.items():
                t = timed(fn, inner=4)
                if i >= a.warmup:
                    times[k].append(t)
        for k in legs:
            rounds[k].append(statistics.median(times[k]))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    upd = med['fused_update_launch'] * 1e-3
    return {'tensors': len(opt._params()), 'elements': numel, 'chunks': opt._chunks, 'launches_per_list_kernel': len(opt._tables),
            'median_ms': {k: round(v, 4) for k, v in med.items()}, 'rounds_ms': {k: [round(x, 4) for x in v] for k, v in rounds.items()},
            'update_bytes': 28 * numel, 'update_TBps': round(28 * numel / upd / 1e12, 3), 'update_fraction_of_copy_rate': round(28 * numel / upd / COPY_RATE, 3),
            'skipped': int(opt.skipped.item())}


def captured(a, state, sizes):
    """(b): the captured head step with and without the optimizer"""
    from sparsebev_amd import optim, synthetic as S
    from sparsebev_amd.train_graph import CapturedHeadTrainStep
    import bench_head_train as BH
    dev = 'cuda:0'
    ih, iw, _ = S.PYRAMIDS[a.pyr]
    B, gts = 1, 40
    feats = S.make_features(B, a.t, sizes, seed=0, device=dev)
    gt_boxes, gt_labels = BH.make_gt(B, gts, 1, dev)
    boxes, labels = [t.cpu() for t in gt_boxes], [t.cpu() for t in gt_labels]
    metas = S.make_img_metas(B, a.t, ih, iw)
    for m, b, l in zip(metas, boxes, labels):
        m['gt_bboxes_3d'], m['gt_labels_3d'] = b, l

    def build(with_opt):
        head = make_head(a, sizes, gt_capacity=gts)
        head.load_state_dict(state, strict=True)
        head = head.to(dev).train()
        opt = optim.FusedAdamW(optim.param_groups(head.named_parameters(), 2e-4, 0.01, KEYS), max_grad_norm=35.0, **RECIPE) if with_opt else None
        return head, CapturedHeadTrainStep(head, feats, metas, optimizer=opt)

    _, inside = build(True)
    head_t, plain_t = build(False)
    _, plain = build(False)
    topt = torch_optimizer(head_t.named_parameters())
    tparams = [p for p in head_t.parameters() if p.requires_grad]

    def torch_after():
        plain_t.replay(boxes, labels, metas)
        torch.nn.utils.clip_grad_norm_(tparams, 35.0, foreach=True)
        topt.step()

    legs = {'captured_optimizer_inside': lambda: inside.replay(boxes, labels, metas), 'captured_then_torch_optimizer': torch_after,
            'captured_no_optimizer': lambda: plain.replay(boxes, labels, metas)}
    rounds = {k: [] for k in legs}
    for _ in range(3):
        times = {k: [] for k in legs}
        for i in range(a.warmup + a.steps):
            for k, fn in legs.items():
                t = timed(fn)
                if i >= a.warmup:
                    times[k].append(t)
        for k in legs:
            rounds[k].append(statistics.median(times[k]))
    assert inside.captures == 1 and int(inside.optimizer.skipped.item()) == 0
    return {'B': B, 'gts': gts, 'capacity': gts, 'median_ms': {k: round(statistics.median(v), 4) for k, v in rounds.items()},
            'rounds_ms': {k: [round(x, 4) for x in v] for k, v in rounds.items()}, 'optimizer_steps': int(inside.optimizer.step_count.item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--q', type=int, default=900)
    ap.add_argument('--t', type=int, default=8)
    ap.add_argument('--groups', type=int, default=10)
    ap.add_argument('--pyr', default='r50_704x256')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_step.json'))
    ap.add_argument('--resources-only', action='store_true')
    a = ap.parse_args()
    res = kernel_resources()
    if a.resources_only:
        print(json.dumps(res))
        return
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from sparsebev_amd import synthetic as S
    _, _, sizes = S.PYRAMIDS[a.pyr]
    head = make_head(a, sizes)
    head.init_weights()
    S.randomize_zero_init(head.transformer, std=0.02, seed=0)
    with torch.no_grad():
        head.init_query_bbox.weight[:, 2] = 0.5
    state = head.state_dict()
    rec = {'tool': 'bench_optim', 'device': torch.cuda.get_device_name(0), 'Q': a.q, 'T': a.t, 'steps': a.steps, 'rounds': 3,
           'timing': 'HIP events, legs interleaved in one process, median of the rounds\' medians',
           'optimizer_launches': launches(a, copy.deepcopy(head).to('cuda:0').train()),
           'captured_head_step': captured(a, state, sizes), 'kernel_resources': res}
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
