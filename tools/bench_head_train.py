"""Dev tool: time the training head (sparsebev_amd.head_train.SparseBEVTrainHead) at the c2 training shape -- Q = 900, B = 1,
T = 8, 6 layers, 10 denoising groups, 40 gts -- beside a plain-torch restatement of the reference's flow on the same tensors:
per layer and sample ~40 cost ops -> .cpu() -> solver, target construction in Python loops, torch focal / L1 losses
(models/sparsebev_head.py:224-460, hungarian_assigner_3d.py:27-93).  Both sides are timed interleaved in the same run with HIP
events, medians of --steps: `loss()` alone on fixed head outputs, and the whole step (forward + loss + backward; the forward and
the decoder backward are the same HIP path on both sides).  Nobody has measured either side before: the record is the point, no
ratio is required.  Writes one JSON line (default profiles/head_train.json) that also carries the compiler's per-kernel resource
figures of csrc/head_train.hip and csrc/head_assign.hip (VGPRs, SGPRs, scratch, LDS).

--assign-on device times the head with the assignment solved on the device (csrc/head_assign.hip) instead of on the host; both adds
`loss_hip_device` / `step_hip_device` legs to the same timed loop, alternating with the host legs, after asserting that the two heads
return identical loss dicts.

    python tools/bench_head_train.py [--steps 50] [--assign-on host|device|both] [--out profiles/head_train.json]
    python tools/bench_head_train.py --captured [--steps 50]   (the captured step beside the eager one -> profiles/head_step_captured.json)
    python tools/bench_head_train.py --resources-only          (no GPU needed)
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
import torch.nn.functional as F               # noqa: E402


def kernel_resources():
    """{kernel: {vgprs, sgprs, scratch_bytes_per_lane, lds_bytes_per_block}} from hipcc's kernel-resource-usage remarks."""
    from sparsebev_amd.csrc import build
    text = ''
    with tempfile.TemporaryDirectory() as tmp:
        for unit in ('head_train.hip', 'head_assign.hip'):
            cmd = [build._hipcc()] + build.COMMON + build.UNITS[unit] + ['-Rpass-analysis=kernel-resource-usage', '-c',
                                                                         os.path.join(build.HERE, unit), '-o', os.path.join(tmp, 'unit.o')]
            text += subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    out, cur = {}, None
    keys = {'VGPRs': 'vgprs', 'TotalSGPRs': 'sgprs', 'ScratchSize [bytes/lane]': 'scratch_bytes_per_lane', 'LDS Size [bytes/block]': 'lds_bytes_per_block'}
    for line in text.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = subprocess.run(['c++filt', m.group(1)], stdout=subprocess.PIPE).stdout.decode().strip() or m.group(1)
            cur = out.setdefault((re.findall(r'(\w+(?:<[^()]*>)?)\(', name) or [name])[0], {})      # `kernel` or `kernel<template arguments>`
            continue
        for k, v in keys.items():
            m = re.search(r'remark:\s+' + re.escape(k) + r': (\d+)', line)
            if m and cur is not None:
                cur[v] = int(m.group(1))
    return out


# ---- the reference's flow in plain torch ops (device tensors, fp32) ----------------------------------------------------------

def normalize_bbox(b):
    return torch.cat([b[..., 0:2], b[..., 3:5].log(), b[..., 2:3], b[..., 5:6].log(), b[..., 6:7].sin(), b[..., 6:7].cos(), b[..., 7:9]], dim=-1)


def focal_loss(pred, target, nc, avg, alpha=0.25, gamma=2.0, weight=2.0):
    t = F.one_hot(target, num_classes=nc + 1)[:, :nc].type_as(pred)
    p = pred.sigmoid()
    pt = (1 - p) * t + p * (1 - t)
    fw = (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma)
    return weight * (F.binary_cross_entropy_with_logits(pred, t, reduction='none') * fw).sum() / avg


def torch_assign(bbox_pred, cls_pred, gt_bboxes, gt_labels, cw, solver):
    """hungarian_assigner_3d.py:27-93"""
    n = bbox_pred.size(0)
    gt_inds = bbox_pred.new_full((n,), 0, dtype=torch.long)
    if gt_bboxes.size(0) == 0:
        return gt_inds
    p = cls_pred.sigmoid()
    neg = -(1 - p + 1e-12).log() * 0.75 * p.pow(2)
    pos = -(p + 1e-12).log() * 0.25 * (1 - p).pow(2)
    cls_cost = (pos[:, gt_labels] - neg[:, gt_labels]) * 2.0
    reg_cost = torch.cdist(bbox_pred * cw, normalize_bbox(gt_bboxes) * cw, p=1) * 0.25
    cost = torch.nan_to_num((cls_cost + reg_cost).detach().cpu(), nan=100.0, posinf=100.0, neginf=-100.0)
    rows, cols = solver(cost)
    gt_inds[torch.as_tensor(rows).to(bbox_pred.device)] = torch.as_tensor(cols).to(bbox_pred.device) + 1
    return gt_inds


def torch_loss_single(cls_scores, bbox_preds, gt_boxes, gt_labels, cw, nc, solver):
    """:301-402 for one layer"""
    labels_l, targets_l, weights_l, num_pos = [], [], [], 0
    for b in range(cls_scores.size(0)):
        gt_inds = torch_assign(bbox_preds[b], cls_scores[b], gt_boxes[b], gt_labels[b], cw, solver)
        pos = torch.nonzero(gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        labels = gt_boxes[b].new_full((bbox_preds.size(1),), nc, dtype=torch.long)
        labels[pos] = gt_labels[b][gt_inds[pos] - 1]
        targets, weights = torch.zeros_like(bbox_preds[b])[..., :9], torch.zeros_like(bbox_preds[b])
        weights[pos] = 1.0
        targets[pos] = gt_boxes[b][gt_inds[pos] - 1]
        labels_l.append(labels), targets_l.append(targets), weights_l.append(weights)
        num_pos += pos.numel()
    labels, targets, weights = torch.cat(labels_l), torch.cat(targets_l), torch.cat(weights_l)
    avg = max(cls_scores.new_tensor([num_pos * 1.0]), 1)
    loss_cls = focal_loss(cls_scores.reshape(-1, nc), labels, nc, avg)
    num_pos = torch.clamp(cls_scores.new_tensor([num_pos]), min=1).item()
    ngt = normalize_bbox(targets)
    ok = torch.isfinite(ngt).all(dim=-1)
    bp = bbox_preds.reshape(-1, 10)
    loss_bbox = 0.25 * ((bp[ok] - ngt[ok]).abs() * (weights * cw)[ok]).sum() / num_pos
    return torch.nan_to_num(loss_cls), torch.nan_to_num(loss_bbox)


def torch_loss(head, gt_boxes, gt_labels, preds, solver):
    """:224-299,405-460"""
    cw, nc = head.code_weights, head.num_classes
    all_cls, all_box = preds['all_cls_scores'], preds['all_bbox_preds']
    out = {}
    L = all_cls.size(0)
    md = preds.get('dn_mask_dict')
    if md is not None:
        cls, box = md['output_known_lbs_bboxes']
        known_labels, known_bboxs = md['known_lbs_bboxes']
        bid = md['batch_idx'][md['known_indice']]
        cls = cls.permute(1, 2, 0, 3)[(bid, md['map_known_indice'])].permute(1, 0, 2)
        box = box.permute(1, 2, 0, 3)[(bid, md['map_known_indice'])].permute(1, 0, 2)
        num_tgt = md['known_indice'].numel()
        for l in range(L):
            n = torch.clamp(cls.new_tensor([num_tgt]), min=1.0).item()
            lc = focal_loss(cls[l].reshape(-1, nc), known_labels.long(), nc, n)
            ngt = normalize_bbox(known_bboxs)
            ok = torch.isfinite(ngt).all(dim=-1)
            lb = 0.25 * ((box[l][ok] - ngt[ok]).abs() * (torch.ones_like(box[l]) * cw)[ok]).sum() / n
            pre = '' if l == L - 1 else 'd%d.' % l
            out[pre + 'loss_cls_dn'], out[pre + 'loss_bbox_dn'] = torch.nan_to_num(lc), torch.nan_to_num(lb)
    for l in range(L):
        lc, lb = torch_loss_single(all_cls[l], all_box[l], gt_boxes, gt_labels, cw, nc, solver)
        pre = '' if l == L - 1 else 'd%d.' % l
        out[pre + 'loss_cls'], out[pre + 'loss_bbox'] = lc, lb
    return out


def make_gt(B, gts, seed, dev):
    g = torch.Generator().manual_seed(seed)
    gt_boxes, gt_labels = [], []
    for _ in range(B):
        bx = torch.empty(gts, 9)
        bx[:, 0:2] = (torch.rand(gts, 2, generator=g) * 2 - 1) * 50
        bx[:, 2] = torch.rand(gts, generator=g) * 6 - 4.5
        bx[:, 3:6] = torch.rand(gts, 3, generator=g) * 4 + 0.4
        bx[:, 6] = (torch.rand(gts, generator=g) * 2 - 1) * 3.1
        bx[:, 7:9] = torch.randn(gts, 2, generator=g)
        gt_boxes.append(bx.to(dev))
        gt_labels.append(torch.randint(0, 10, (gts,), generator=g).to(dev))
    return gt_boxes, gt_labels


def captured(a, res):
    """--captured: the head's whole training step as ONE graph (train_graph.CapturedHeadTrainStep on SparseBEVTrainHead(gt_capacity=...))
    beside the eager assign_on='device' step of the same tree at the same counts, interleaved in one run, at both recorded shapes (B = 1
    with 40 boxes, B = 2 with 200) and with the capacity at the batch's maximum and at twice it.  The eager step gets its ground truth
    device-resident, as the recorded runs did; the replay gets it host-resident (the loader's case: the slab packs on the host)."""
    from sparsebev_amd import synthetic as S
    from sparsebev_amd.head_train import SparseBEVTrainHead
    from sparsebev_amd.train_graph import CapturedHeadTrainStep
    dev = 'cuda:0'
    ih, iw, sizes = S.PYRAMIDS[a.pyr]

    def make_head(**kw):
        return SparseBEVTrainHead(num_classes=10, in_channels=256, num_query=a.q, query_denoising_groups=a.groups, code_size=10,
                                  code_weights=[2.0, 2.0] + [1.0] * 8,
                                  transformer=dict(type='SparseBEVTransformer', embed_dims=256, num_frames=a.t, num_points=4, num_layers=6,
                                                   num_levels=len(sizes), num_classes=10, code_size=10, pc_range=S.PC_RANGE),
                                  bbox_coder=dict(type='NMSFreeCoder', post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_num=300,
                                                  num_classes=10, pc_range=S.PC_RANGE), assign_on='device', **kw)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    eager = make_head()
    eager.init_weights()
    S.randomize_zero_init(eager.transformer, std=0.02, seed=0)
    with torch.no_grad():
        eager.init_query_bbox.weight[:, 2] = 0.5
    state = eager.state_dict()
    eager = eager.to(dev).train()
    shapes = []
    for B, gts in ((1, 40), (2, 200)):
        feats = S.make_features(B, a.t, sizes, seed=0, device=dev)
        gt_boxes, gt_labels = make_gt(B, gts, 1, dev)
        host_boxes, host_labels = [t.cpu() for t in gt_boxes], [t.cpu() for t in gt_labels]
        metas = S.make_img_metas(B, a.t, ih, iw)
        host_metas = copy.deepcopy(metas)
        for m, hm, bx, lb, hb, hl in zip(metas, host_metas, gt_boxes, gt_labels, host_boxes, host_labels):
            m['gt_bboxes_3d'], m['gt_labels_3d'] = bx, lb
            hm['gt_bboxes_3d'], hm['gt_labels_3d'] = hb, hl
        steps = {}
        for cap in (gts, 2 * gts):
            head = make_head(gt_capacity=cap)
            head.load_state_dict(state, strict=True)
            steps[cap] = CapturedHeadTrainStep(head.to(dev).train(), feats, host_metas)

        def eager_step():
            for p in eager.parameters():
                p.grad = None
            outs = eager(feats, copy.deepcopy(metas))
            sum(eager.loss(gt_boxes, gt_labels, outs).values()).backward()

        times = {'step_eager_device': []}
        times.update({'step_captured_cap%d' % cap: [] for cap in steps})
        for i in range(a.warmup + a.steps):
            row = {'step_eager_device': timed(eager_step)}
            for cap, st in steps.items():
                row['step_captured_cap%d' % cap] = timed(lambda: st.replay(host_boxes, host_labels, host_metas))
            if i >= a.warmup:
                for k, v in row.items():
                    times[k].append(v)
        for cap, st in steps.items():
            assert st.captures == 1 and st.head.plan_status.tolist() == [0] and all(bool(torch.isfinite(v)) for v in st.losses.values())
        shapes.append({'B': B, 'gts': gts, 'capacities': sorted(steps), 'pad_sizes': {str(cap): cap * a.groups for cap in sorted(steps)},
                       'median_ms': {k: round(statistics.median(v), 4) for k, v in times.items()},
                       'min_ms': {k: round(min(v), 4) for k, v in times.items()}})
        del steps
    rec = {'tool': 'bench_head_train --captured', 'device': torch.cuda.get_device_name(0), 'Q': a.q, 'T': a.t, 'layers': 6, 'dn_groups': a.groups,
           'steps': a.steps, 'dropout': 'on', 'timing': 'HIP events around each step, eager and captured interleaved in one run',
           'shapes': shapes, 'kernel_resources': res}
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--q', type=int, default=900)
    ap.add_argument('--t', type=int, default=8)
    ap.add_argument('--b', type=int, default=1)
    ap.add_argument('--gts', type=int, default=40)
    ap.add_argument('--groups', type=int, default=10)
    ap.add_argument('--pyr', default='r50_704x256')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'head_train.json'))
    ap.add_argument('--assign-on', choices=('host', 'device', 'both'), default='host')
    ap.add_argument('--resources-only', action='store_true')
    ap.add_argument('--captured', action='store_true', help='time the step captured as one graph beside the eager device-assignment step, at both '
                                                            'recorded shapes and two capacities (default --out profiles/head_step_captured.json)')
    a = ap.parse_args()
    res = kernel_resources()
    if a.resources_only:
        print(json.dumps(res))
        return
    if a.captured:
        if a.out == ap.get_default('out'):
            a.out = os.path.join(ROOT, 'profiles', 'head_step_captured.json')
        captured(a, res)
        return
    from sparsebev_amd import synthetic as S
    from sparsebev_amd.head_train import SparseBEVTrainHead, lsa_solve
    try:
        from scipy.optimize import linear_sum_assignment as solver
        solver_name = 'scipy'
    except ImportError:
        import numpy as np

        def solver(cost):
            col = lsa_solve(cost.numpy())
            rows = np.nonzero(col >= 0)[0]
            return rows, col[rows]
        solver_name = 'sbev_lsa_solve'
    dev = 'cuda:0'
    ih, iw, sizes = S.PYRAMIDS[a.pyr]
    head = SparseBEVTrainHead(num_classes=10, in_channels=256, num_query=a.q, query_denoising_groups=a.groups, code_size=10,
                              code_weights=[2.0, 2.0] + [1.0] * 8,
                              transformer=dict(type='SparseBEVTransformer', embed_dims=256, num_frames=a.t, num_points=4, num_layers=6,
                                               num_levels=len(sizes), num_classes=10, code_size=10, pc_range=S.PC_RANGE),
                              bbox_coder=dict(type='NMSFreeCoder', post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_num=300,
                                              num_classes=10, pc_range=S.PC_RANGE), assign_on='device' if a.assign_on == 'device' else 'host')
    head.init_weights()
    S.randomize_zero_init(head.transformer, std=0.02, seed=0)
    with torch.no_grad():
        head.init_query_bbox.weight[:, 2] = 0.5
    head = head.to(dev).train()
    feats = S.make_features(a.b, a.t, sizes, seed=0, device=dev)
    gt_boxes, gt_labels = make_gt(a.b, a.gts, 1, dev)
    metas = S.make_img_metas(a.b, a.t, ih, iw)
    for m, bx, lb in zip(metas, gt_boxes, gt_labels):
        m['gt_bboxes_3d'], m['gt_labels_3d'] = bx, lb

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def step(loss_fn, head=head):
        for p in head.parameters():
            p.grad = None
        outs = head(feats, copy.deepcopy(metas))
        sum(loss_fn(outs).values()).backward()

    ours = lambda outs: head.loss(gt_boxes, gt_labels, outs)
    theirs = lambda outs: torch_loss(head, gt_boxes, gt_labels, outs, solver)
    outs = head(feats, copy.deepcopy(metas))
    fixed = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in outs.items()}
    md = dict(outs['dn_mask_dict'])
    md['output_known_lbs_bboxes'] = tuple(t.detach() for t in md['output_known_lbs_bboxes'])
    fixed['dn_mask_dict'] = md
    la, lb = ours(fixed), theirs(fixed)
    worst = max(abs(la[k].item() - lb[k].item()) / max(1.0, abs(lb[k].item())) for k in lb)
    assert sorted(la) == sorted(lb) and worst < 1e-4, (worst, la, lb)
    times = {'loss_hip': [], 'loss_torch': [], 'step_hip': [], 'step_torch': []}
    if a.assign_on == 'both':       # a second head on the same parameters (the modules are shared, nothing is copied) that solves on the device
        twin = copy.copy(head)
        twin.assign_on = 'device'
        ours_device = lambda outs: twin.loss(gt_boxes, gt_labels, outs)
        ld = ours_device(fixed)
        assert sorted(ld) == sorted(la) and all(torch.equal(ld[k], la[k]) for k in la), (ld, la)
        assert bool((twin.assign_status == 0).all())
        times.update(loss_hip_device=[], step_hip_device=[])
    for i in range(a.warmup + a.steps):
        row = {'loss_hip': timed(lambda: ours(fixed)), 'loss_torch': timed(lambda: theirs(fixed)),
               'step_hip': timed(lambda: step(ours)), 'step_torch': timed(lambda: step(theirs))}
        if a.assign_on == 'both':
            row.update(loss_hip_device=timed(lambda: ours_device(fixed)), step_hip_device=timed(lambda: step(ours_device, twin)))
        if i >= a.warmup:
            for k, v in row.items():
                times[k].append(v)
    rec = {'tool': 'bench_head_train', 'device': torch.cuda.get_device_name(0), 'Q': a.q, 'B': a.b, 'T': a.t, 'layers': 6, 'dn_groups': a.groups,
           'gts': a.gts, 'pad_size': md['pad_size'], 'steps': a.steps, 'torch_side_solver': solver_name, 'loss_dict_max_rel_diff': worst,
           'median_ms': {k: round(statistics.median(v), 4) for k, v in times.items()},
           'min_ms': {k: round(min(v), 4) for k, v in times.items()},
           'kernel_resources': res}
    if a.assign_on != 'host':
        rec['assign_on'] = a.assign_on
    assert all(r.get('scratch_bytes_per_lane') == 0 for r in res.values()), res
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
