"""Generate fixture G15 (g15_head_train.npz) by running the REFERENCE's own training head: prepare_for_dn_input,
prepare_for_dn_loss, HungarianAssigner3D.assign and SparseBEVHead.loss.

Runs only in the authoring container (needs /root/reference and scipy; never on the GPU box).  The reference package is
imported without its mmcv / mmdet / mmdet3d dependencies, in the style of make_golden.py: stub packages with ``__path__``,
``force_fp32`` as identity, ``multi_apply``, ``reduce_mean`` as identity, registries, a ``DETRHead`` stand-in that is an
``nn.Module``, a minimal box class, a pseudo sampler, and mmdet's sigmoid focal loss, L1 loss and ``FocalLossCost`` restated
(mmdet is not vendored by the reference: parity is unpinned at that boundary only).  The head instance is made without the
mmdet constructor and its attributes are set by hand.  ``torch.rand_like`` and ``torch.randint_like`` are patched during
``prepare_for_dn_input`` so that the recorded noise is what the reference consumes.

For every recorded assignment the margin to the second-best assignment is computed (re-solve with each matched pair forbidden,
smallest increase of the total) and the seed is chosen such that it is >= 1e-3.  A gt whose velocity is NaN has a cost column
of all 100s: which query it takes does not change the total, so its pair is left out of the margin; the solver's choice there
is by scan order, which the library's solver shares with scipy's.

    python tests/golden/make_golden_head_train.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import head_train_cases as C   # noqa: E402  (shapes and input generators only)

REF = '/root/reference'
D, L, Q = 16, 2, 36


def _stub(name, path=None, **attrs):
    m = types.ModuleType(name)
    if path:
        m.__path__ = [path]
    m.__dict__.update(attrs)
    sys.modules[name] = m


class _Registry:
    def register_module(self):
        return lambda cls: cls


class Boxes:
    """what the head reads of LiDARInstance3DBoxes: .tensor [n,9] with bottom-centre z, .gravity_center"""

    def __init__(self, tensor):
        self.tensor = tensor

    @property
    def gravity_center(self):
        t = self.tensor
        return torch.cat([t[:, :2], t[:, 2:3] + t[:, 5:6] * 0.5], dim=1)


class AssignResult:
    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


class PseudoSampler:
    """mmdet's PseudoSampler / SamplingResult, the fields _get_target_single reads"""

    def sample(self, assign_result, bboxes, gt_bboxes):
        r = types.SimpleNamespace()
        r.pos_inds = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        r.neg_inds = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        r.pos_assigned_gt_inds = assign_result.gt_inds[r.pos_inds] - 1
        r.pos_gt_bboxes = gt_bboxes[r.pos_assigned_gt_inds].view(-1, gt_bboxes.shape[-1])
        return r


class FocalLoss(nn.Module):
    """mmdet FocalLoss(use_sigmoid=True): py_sigmoid_focal_loss + weight_reduce_loss(avg_factor)"""

    def __init__(self, gamma=2.0, alpha=0.25, loss_weight=1.0):
        super().__init__()
        self.gamma, self.alpha, self.loss_weight = gamma, alpha, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        nc = pred.size(1)
        t = F.one_hot(target, num_classes=nc + 1)[:, :nc].type_as(pred)
        p = pred.sigmoid()
        pt = (1 - p) * t + p * (1 - t)
        fw = (self.alpha * t + (1 - self.alpha) * (1 - t)) * pt.pow(self.gamma)
        loss = F.binary_cross_entropy_with_logits(pred, t, reduction='none') * fw
        if weight is not None:
            loss = loss * weight.view(-1, 1)
        return self.loss_weight * loss.sum() / avg_factor


class L1Loss(nn.Module):
    def __init__(self, loss_weight=1.0):
        super().__init__()
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        if target.numel() == 0:
            return pred.sum() * 0
        return self.loss_weight * ((pred - target).abs() * weight).sum() / avg_factor


class FocalLossCost:
    def __init__(self, weight=1., alpha=0.25, gamma=2, eps=1e-12):
        self.weight, self.alpha, self.gamma, self.eps = weight, alpha, gamma, eps

    def __call__(self, cls_pred, gt_labels):
        cls_pred = cls_pred.sigmoid()
        neg = -(1 - cls_pred + self.eps).log() * (1 - self.alpha) * cls_pred.pow(self.gamma)
        pos = -(cls_pred + self.eps).log() * self.alpha * (1 - cls_pred).pow(self.gamma)
        return (pos[:, gt_labels] - neg[:, gt_labels]) * self.weight


def multi_apply(func, *args, **kwargs):
    from functools import partial
    results = map(partial(func, **kwargs) if kwargs else func, *args)
    return tuple(map(list, zip(*results)))


def import_reference():
    class BaseModule(nn.Module):
        def __init__(self, init_cfg=None):
            super().__init__()

    class DETRHead(nn.Module):
        pass

    def build_match_cost(cfg):
        cfg = dict(cfg)
        kind = cfg.pop('type')
        if kind == 'FocalLossCost':
            return FocalLossCost(**cfg)
        if kind == 'BBox3DL1Cost':
            return importlib.import_module('models.bbox.match_costs.match_cost').BBox3DL1Cost(**cfg)
        return None                                            # IoUCost at weight 0: never called by the assigner

    _stub('models', REF + '/models'); _stub('models.bbox', REF + '/models/bbox')
    _stub('models.bbox.assigners', REF + '/models/bbox/assigners'); _stub('models.bbox.match_costs', REF + '/models/bbox/match_costs')
    _stub('mmcv'); _stub('mmcv.runner', BaseModule=BaseModule, force_fp32=lambda **kw: (lambda f: f))
    _stub('mmdet'); _stub('mmdet.core', multi_apply=multi_apply, reduce_mean=lambda t: t)
    _stub('mmdet.models', HEADS=_Registry()); _stub('mmdet.models.dense_heads', DETRHead=DETRHead)
    _stub('mmdet.core.bbox'); _stub('mmdet.core.bbox.builder', BBOX_ASSIGNERS=_Registry())
    _stub('mmdet.core.bbox.assigners', AssignResult=AssignResult, BaseAssigner=object)
    _stub('mmdet.core.bbox.match_costs', build_match_cost=build_match_cost); _stub('mmdet.core.bbox.match_costs.builder', MATCH_COST=_Registry())
    _stub('mmdet3d'); _stub('mmdet3d.core'); _stub('mmdet3d.core.bbox'); _stub('mmdet3d.core.bbox.coders', build_bbox_coder=lambda cfg: None)
    _stub('mmdet3d.core.bbox.structures'); _stub('mmdet3d.core.bbox.structures.lidar_box3d', LiDARInstance3DBoxes=Boxes)
    head = importlib.import_module('models.sparsebev_head')
    assigner = importlib.import_module('models.bbox.assigners.hungarian_assigner_3d')
    importlib.import_module('models.bbox.match_costs.match_cost')
    butils = importlib.import_module('models.bbox.utils')
    return head, assigner, butils


def make_head(mod, amod, NC, N, init_w, label_w):
    head = mod.SparseBEVHead.__new__(mod.SparseBEVHead)
    nn.Module.__init__(head)
    head.num_query, head.num_classes, head.cls_out_channels, head.embed_dims, head.code_size = Q, NC, NC, D, 10
    head.code_weights = nn.Parameter(torch.tensor(C.CODE_WEIGHTS), requires_grad=False)
    head.pc_range = C.PC_RANGE
    head.dn_enabled, head.dn_group_num, head.dn_weight, head.dn_bbox_noise_scale, head.dn_label_noise_scale = True, N, 1.0, 0.5, 0.5
    head.bg_cls_weight, head.sync_cls_avg_factor = 0, True
    head.loss_cls, head.loss_bbox = FocalLoss(gamma=2.0, alpha=0.25, loss_weight=2.0), L1Loss(loss_weight=0.25)
    head.assigner = amod.HungarianAssigner3D(cls_cost=dict(type='FocalLossCost', weight=2.0), reg_cost=dict(type='BBox3DL1Cost', weight=0.25),
                                             iou_cost=dict(type='IoUCost', weight=0.0))
    head.sampler = PseudoSampler()
    head.init_query_bbox, head.label_enc = nn.Embedding(Q, 10), nn.Embedding(NC + 1, D - 1)
    with torch.no_grad():
        head.init_query_bbox.weight.copy_(init_w)
        head.label_enc.weight.copy_(label_w)
    return head.train()


def margin_of(cost, rows, cols, skip_cols):
    """smallest increase of the total when one matched pair is forbidden (pairs of the columns in skip_cols left out)"""
    base = cost[rows, cols].sum()
    best = np.inf
    for r, c in zip(rows, cols):
        if c in skip_cols:
            continue
        alt = cost.copy()
        alt[r, c] = 1e6
        rr, cc = linear_sum_assignment(alt)
        best = min(best, alt[rr, cc].sum() - base)
    return best


def run_case(mod, amod, butils, tag, counts, N, seed, nan_vel_at):
    NC = 10
    boxes, labels = C.make_gt(counts, NC, seed, nan_vel_at)            # gravity-centred [n,9]
    init_w, label_w = C.make_embeddings(Q, NC, D, seed + 1)
    G = sum(counts)
    u_box, u_lab, new_lab = C.make_noise(N, G, NC, seed + 2)
    head = make_head(mod, amod, NC, N, init_w, label_w)
    metas = [{'gt_bboxes_3d': types.SimpleNamespace(gravity_center=b[:, :3].clone(), tensor=b.clone()), 'gt_labels_3d': l.clone()}
             for b, l in zip(boxes, labels)]
    # the reference draws rand_like over nine columns and computes `rand * 2 - 1.0`: hand it the uniform draw u_box was made from
    u9 = torch.rand(N * G, 9)
    u9[:, :3] = torch.rand(N * G, 3, generator=torch.Generator().manual_seed(seed + 2))
    assert torch.equal(u9[:, :3] * 2 - 1.0, u_box)
    calls = {'rand': 0}

    def rand_like(t, *a, **k):
        calls['rand'] += 1
        return u9.clone() if calls['rand'] == 1 else u_lab.clone()

    def randint_like(t, lo, hi, **k):
        return new_lab.long()[t]                                       # t = chosen_indice

    saved = torch.rand_like, torch.randint_like, torch.Tensor.cuda
    torch.rand_like, torch.randint_like, torch.Tensor.cuda = rand_like, randint_like, lambda self, *a, **k: self
    try:
        with torch.no_grad():
            qb, qf, mask, md = head.prepare_for_dn_input(len(counts), head.init_query_bbox.weight.clone(), head.label_enc, metas)
    finally:
        torch.rand_like, torch.randint_like, torch.Tensor.cuda = saved
    pad = md['pad_size']
    g = torch.Generator().manual_seed(seed + 3)
    cls = torch.randn(L, len(counts), pad + Q, NC, generator=g) * 2 - 2
    box = torch.randn(L, len(counts), pad + Q, 10, generator=g)
    box[..., 0:2] *= 30
    preds = {'all_cls_scores': cls[:, :, pad:], 'all_bbox_preds': box[:, :, pad:], 'enc_cls_scores': None, 'enc_bbox_preds': None}
    out = {}
    if pad > 0:
        md['output_known_lbs_bboxes'] = (cls[:, :, :pad], box[:, :, :pad])
        preds['dn_mask_dict'] = md
        _, _, g_cls, g_box, num_tgt = head.prepare_for_dn_loss(md)
        out.update(dn_gather_cls=g_cls, dn_gather_box=g_box, num_tgt=num_tgt)
    # the assignment per layer and sample, and its margin
    assign = torch.full((L, len(counts), Q), -1, dtype=torch.int64)
    margin = np.inf
    for l in range(L):
        for b in range(len(counts)):
            res = head.assigner.assign(preds['all_bbox_preds'][l, b], preds['all_cls_scores'][l, b], boxes[b], labels[b], None, head.code_weights, True)
            assign[l, b] = res.gt_inds - 1
            if counts[b]:
                cost = head.assigner.cls_cost(preds['all_cls_scores'][l, b], labels[b]) + head.assigner.reg_cost(
                    preds['all_bbox_preds'][l, b] * head.code_weights, butils.normalize_bbox(boxes[b]) * head.code_weights)
                cost = torch.nan_to_num(cost, nan=100.0, posinf=100.0, neginf=-100.0).double().numpy()
                rows = np.nonzero(assign[l, b].numpy() >= 0)[0]
                skip = set(np.nonzero(~torch.isfinite(boxes[b]).all(dim=1).numpy())[0].tolist())
                margin = min(margin, margin_of(cost, rows, assign[l, b].numpy()[rows], skip))
    gt_boxes_list = [types.SimpleNamespace(gravity_center=b[:, :3], tensor=b) for b in boxes]
    losses = head.loss(gt_boxes_list, [l.clone() for l in labels], preds)
    out.update(counts=np.array(counts), N=N, NC=NC, gt_boxes=torch.cat(boxes), gt_labels=torch.cat(labels), init_w=init_w, label_w=label_w,
               u_box=u_box, u_lab=u_lab, new_lab=new_lab, query_bbox=qb, query_feat=qf, attn_mask=mask, known_indice=md['known_indice'],
               batch_idx=md['batch_idx'], map_known_indice=md['map_known_indice'] if G else torch.zeros(0, dtype=torch.long),
               known_labels=md['known_lbs_bboxes'][0], known_bboxs=md['known_lbs_bboxes'][1], pad_size=pad, cls=cls, box=box,
               assign=assign, margin=margin if np.isfinite(margin) else -1.0, loss_keys=np.array(sorted(losses)),
               loss_values=np.array([float(losses[k]) for k in sorted(losses)], dtype=np.float32))
    return {tag + '_' + k: v for k, v in out.items()}, margin


def main():
    torch.manual_seed(0)
    mod, amod, butils = import_reference()
    arrays = {}
    for tag, counts, N, nan_at in (('a', (5, 3), 10, (0, 2)), ('b', (0, 4), 2, None), ('c', (0, 0), 10, None)):
        for seed in range(1500, 1600):
            case, margin = run_case(mod, amod, butils, tag, counts, N, seed, nan_at)
            if margin >= 1e-3:
                break
        else:
            raise RuntimeError('no seed with a margin >= 1e-3 for case ' + tag)
        print('case %s: seed %d, margin %.3g' % (tag, seed, margin))
        case[tag + '_seed'] = seed
        arrays.update(case)
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}
    path = os.path.join(HERE, 'g15_head_train.npz')
    np.savez_compressed(path, **out)
    print('g15_head_train %.1f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
