"""Shapes for the training-head tests and an independent torch restatement of the training head's three device stages, written
from the formulas (not from the kernels) with the reference's line numbers cited:

  * ``dn_prepare``   denoising queries, attention mask and mask_dict (models/sparsebev_head.py:119-222, bbox/utils.py:46-60)
  * ``match_cost``   FocalLossCost + BBox3DL1Cost on normalize_bbox(gt) * code_weights (hungarian_assigner_3d.py:54-74,
                     match_cost.py:6-27, bbox/utils.py:4-20), ``assign`` with a small pure-Python Hungarian solver
  * ``set_loss``     sigmoid focal loss + L1 loss per layer from row codes (models/sparsebev_head.py:239-275,349-402)

Everything runs in the dtype of its inputs: fp64 for the tolerance checks, fp32 where a bit-equal comparison is made.
"""
import itertools

import numpy as np
import torch

PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
CODE_WEIGHTS = [2.0, 2.0] + [1.0] * 8
FIXTURE_CASES = ('a', 'b', 'c')          # B = 2, Q = 36, NC = 10: gts (5, 3) N = 10 with one NaN velocity; (0, 4) N = 2; (0, 0) N = 10

# generated denoising cases: (name, B, N, NC, counts, box_scale, label_scale)
DN_CASES = [
    ('b1_n1_nc1', 1, 1, 1, (1,), 0.5, 0.5),
    ('b3_n2_nc10', 3, 2, 10, (7, 0, 2), 0.5, 0.5),
    ('b3_n10_nc65', 3, 10, 65, (7, 0, 2), 0.5, 0.5),
    ('b1_n10_nc10_noise_off', 1, 10, 10, (1,), 0.0, 0.0),
    ('b3_n2_nc65_box_off', 3, 2, 65, (7, 0, 2), 0.0, 0.5),
]


def make_gt(counts, NC, seed, nan_vel_at=None):
    """Per-sample ground truth: boxes [n,9] (gravity centre inside the range, positive sizes, rot, velocity), labels [n] long."""
    g = torch.Generator().manual_seed(seed)
    boxes, labels = [], []
    for n in counts:
        b = torch.empty(n, 9)
        b[:, 0:2] = (torch.rand(n, 2, generator=g) * 2 - 1) * 50
        b[:, 2] = torch.rand(n, generator=g) * 6 - 4.5
        b[:, 3:6] = torch.rand(n, 3, generator=g) * 4 + 0.4
        b[:, 6] = (torch.rand(n, generator=g) * 2 - 1) * 3.1
        b[:, 7:9] = torch.randn(n, 2, generator=g) * 3
        boxes.append(b)
        labels.append(torch.randint(0, NC, (n,), generator=g))
    if nan_vel_at is not None:
        boxes[nan_vel_at[0]][nan_vel_at[1], 7:9] = float('nan')
    return boxes, labels


def make_noise(N, G, NC, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(N * G, 3, generator=g) * 2 - 1.0, torch.rand(N * G, generator=g), torch.randint(0, NC, (N * G,), generator=g).int())


def make_embeddings(Q, NC, D, seed):
    g = torch.Generator().manual_seed(seed)
    init = torch.rand(Q, 10, generator=g)
    return init, torch.randn(NC + 1, D - 1, generator=g)


# ---- section 1 ------------------------------------------------------------------------------------------------------------

def encode_bbox(b, pc_range):
    """models/bbox/utils.py:46-60; the python-float range constants act as scalars of the tensor's dtype."""
    xyz = torch.stack([(b[:, i] - pc_range[i]) / (pc_range[3 + i] - pc_range[i]) for i in range(3)], dim=1)
    return torch.cat([xyz, b[:, 3:6].log(), b[:, 6:7].sin(), b[:, 6:7].cos(), b[:, 7:9]], dim=1)


def dn_prepare(init_w, label_w, boxes, labels, noise, N, NC, pc_range=PC_RANGE, box_scale=0.5, label_scale=0.5):
    """-> dict(query_bbox [B,pad+Q,10], query_feat [B,pad+Q,D], attn_mask bool, known_indice, batch_idx, map_known_indice, known_labels,
    known_bboxs, noised_labels, pad_size), differentiable in init_w and label_w."""
    dt, B, Q, D = init_w.dtype, len(boxes), init_w.shape[0], label_w.shape[1] + 1
    counts = [int(b.shape[0]) for b in boxes]
    G, single = sum(counts), max(counts) if counts else 0
    pad = single * N
    gtb = torch.cat([b.to(dt) for b in boxes]) if G else torch.zeros(0, 9, dtype=dt)
    gtl = torch.cat([l.long() for l in labels]) if G else torch.zeros(0, dtype=torch.long)
    u_box, u_lab, new_lab = noise
    known = gtb.repeat(N, 1)                                                   # j = r * G + i (:149-152)
    centre = known[:, 0:3]
    if box_scale > 0:
        centre = centre + (u_box.to(dt) * (known[:, 3:6] / 2)) * box_scale     # :158-160
    enc = encode_bbox(torch.cat([centre, known[:, 3:]], dim=1), pc_range)
    enc = torch.cat([enc[:, 0:3].clamp(min=0.0, max=1.0), enc[:, 3:]], dim=1)  # :164-165
    lab = gtl.repeat(N)
    noised = torch.where(u_lab < label_scale, new_lab.long(), lab) if label_scale > 0 else lab      # :169-173
    feat = torch.cat([label_w[noised], torch.ones(N * G, 1, dtype=dt)], dim=1)                      # :175-177
    batch_idx = torch.cat([torch.full((c,), i, dtype=torch.long) for i, c in enumerate(counts)]) if counts else torch.zeros(0, dtype=torch.long)
    within = torch.cat([torch.arange(c) for c in counts]) if counts else torch.zeros(0, dtype=torch.long)
    map_idx = torch.cat([within + single * r for r in range(N)]).long()                            # :188-189
    bid = batch_idx.repeat(N)
    qb = torch.cat([torch.zeros(pad, 10, dtype=dt), init_w], dim=0).repeat(B, 1, 1)                 # :182-185
    qf = torch.cat([torch.zeros(pad, D, dtype=dt), torch.cat([label_w[NC].repeat(Q, 1), torch.zeros(Q, 1, dtype=dt)], dim=1)], dim=0).repeat(B, 1, 1)
    if G:
        qb = qb.index_put((bid, map_idx), enc)                                                      # :191-193
        qf = qf.index_put((bid, map_idx), feat)
    T = pad + Q
    r, c = torch.arange(T)[:, None], torch.arange(T)[None, :]
    mask = (c < pad) & ((r >= pad) | (r // max(single, 1) != c // max(single, 1)))                   # :195-207
    return dict(query_bbox=qb, query_feat=qf, attn_mask=mask, known_indice=torch.arange(G).repeat(N), batch_idx=batch_idx,
                map_known_indice=map_idx, known_labels=lab, known_bboxs=known, noised_labels=noised, pad_size=pad)


# ---- section 3 ------------------------------------------------------------------------------------------------------------

def normalize_bbox(b):
    """models/bbox/utils.py:4-20"""
    return torch.cat([b[:, 0:2], b[:, 3:5].log(), b[:, 2:3], b[:, 5:6].log(), b[:, 6:7].sin(), b[:, 6:7].cos(), b[:, 7:9]], dim=1)


def match_cost(cls, box, gt_boxes, gt_labels, cw, w_cls=2.0, w_reg=0.25, alpha=0.25, gamma=2.0):
    """cost [Q, g] of one layer and sample (hungarian_assigner_3d.py:54-74 with mmdet's FocalLossCost, eps = 1e-12)."""
    p = cls.sigmoid()
    neg = -(1 - p + 1e-12).log() * (1 - alpha) * p.pow(gamma)
    pos = -(p + 1e-12).log() * alpha * (1 - p).pow(gamma)
    cc = (pos[:, gt_labels.long()] - neg[:, gt_labels.long()]) * w_cls
    ngt = normalize_bbox(gt_boxes.to(cls.dtype)) * cw
    rc = ((box * cw)[:, None, :] - ngt[None, :, :]).abs().sum(-1) * w_reg      # torch.cdist(p = 1)
    return torch.nan_to_num(cc + rc, nan=100.0, posinf=100.0, neginf=-100.0)


def hungarian(cost):
    """Minimum-cost assignment of a [n, m] matrix, n <= m: every row gets its own column (the O(n^2 m) potentials method).  Pure
    Python on purpose: independent of the library's solver and of scipy."""
    n, m = len(cost), len(cost[0]) if len(cost) else 0
    INF = float('inf')
    u, v, p, way = [0.0] * (n + 1), [0.0] * (m + 1), [0] * (m + 1), [0] * (m + 1)
    for i in range(1, n + 1):
        p[0] = i
        j0, minv, used = 0, [INF] * (m + 1), [False] * (m + 1)
        while True:
            used[j0] = True
            i0, delta, j1 = p[j0], INF, 0
            for j in range(1, m + 1):
                if not used[j]:
                    cur = cost[i0 - 1][j - 1] - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            for j in range(m + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    col = [-1] * n
    for j in range(1, m + 1):
        if p[j]:
            col[p[j] - 1] = j - 1
    return col


def solve(cost):
    """col_of_row (numpy int, -1 unmatched) of a [n, m] cost matrix of any shape."""
    c = np.asarray(cost, dtype=np.float64)
    n, m = c.shape
    out = np.full(n, -1, dtype=np.int64)
    if n == 0 or m == 0:
        return out
    if n <= m:
        out[:] = hungarian(c.tolist())
    else:
        for j, i in enumerate(hungarian(c.T.tolist())):
            out[i] = j
    return out


def brute_force_total(cost):
    """Minimum total of min(n, m) pairs by enumeration (n, m <= 6)."""
    c = np.asarray(cost, dtype=np.float64)
    n, m = c.shape
    if n == 0 or m == 0:
        return 0.0
    if n > m:
        c, n, m = c.T, m, n
    return min(sum(c[i, perm[i]] for i in range(n)) for perm in itertools.permutations(range(m), n))


def assign(all_cls, all_box, boxes, labels, cw, **kw):
    """[L, B, Q] long: -1 background, g matched gt of the sample (models/sparsebev_head.py:301-347 per layer and sample)."""
    L, B, Q, _ = all_cls.shape
    out = torch.full((L, B, Q), -1, dtype=torch.long)
    for l in range(L):
        for b in range(B):
            if boxes[b].shape[0]:
                out[l, b] = torch.from_numpy(solve(match_cost(all_cls[l, b], all_box[l, b], boxes[b], labels[b], cw, **kw).numpy()))
    return out


# ---- section 4 ------------------------------------------------------------------------------------------------------------

def focal(x, t, alpha=0.25, gamma=2.0):
    """mmdet's py_sigmoid_focal_loss, elementwise, through softplus"""
    p = x.sigmoid()
    pt = (1 - p) * t + p * (1 - t)
    bce = torch.nn.functional.softplus(x) * (1 - t) + torch.nn.functional.softplus(-x) * t
    return bce * (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma)


def set_loss(cls, box, codes, boxes, labels, cw, a_cls, a_box, w_fl=2.0, alpha=0.25, gamma=2.0, w_l1=0.25, scale=1.0):
    """[L, 2] (loss_cls, loss_bbox).  cls [L,B,R,NC], box [L,B,R,10]; codes long [B,R] or [L,B,R]: -2 skip, -1 background, g target gt g
    of sample b (:239-275,349-402).  The averaging factors are clamped to >= 1 here as the head does before the loss call."""
    L, B, R, NC = cls.shape
    dt = cls.dtype
    codes = codes.expand(L, B, R) if codes.dim() == 2 else codes
    out = []
    for l in range(L):
        s_cls, s_box = cls.new_zeros(()), cls.new_zeros(())
        for b in range(B):
            code = codes[l, b]
            keep = code >= -1
            pos = code >= 0
            t = torch.zeros(R, NC, dtype=dt)
            if pos.any():
                t[pos, labels[b].long()[code[pos]]] = 1.0
            s_cls = s_cls + focal(cls[l, b][keep], t[keep], alpha, gamma).sum()
            if pos.any():
                ngt = normalize_bbox(boxes[b].to(dt))[code[pos]]
                fin = torch.isfinite(ngt).all(dim=-1)                          # isnotnan (:263,389)
                s_box = s_box + ((box[l, b][pos][fin] - ngt[fin]).abs() * cw).sum()
        lc = torch.nan_to_num(w_fl * s_cls / max(float(a_cls), 1.0))
        lb = torch.nan_to_num(w_l1 * s_box / max(float(a_box), 1.0))
        out.append(torch.stack([scale * lc, scale * lb]))
    return torch.stack(out)


def dn_codes(counts, N):
    """[B, single * N]: k at (b, r * single + k) for k < g_b, -2 elsewhere -- what prepare_for_dn_loss's gather selects (:224-237)"""
    single = max(counts) if counts else 0
    k = torch.arange(single)
    return torch.stack([torch.where(k < c, k, torch.full_like(k, -2)).repeat(N) for c in counts]) if counts else torch.zeros(0, 0, dtype=torch.long)


def host_plan(counts, Q, cap, N, bg):
    """A step's plan restated: (codes int32 [B, N * cap], avg fp32 [2,2]) -- the numpy code table at ``single = cap`` and the two pairs
    of averaging factors, (A_cls, A_box) of the matching loss and (A, A) of the denoising loss, as np.float32 of python doubles.  What
    ``GroundTruth.plan`` computes on the host and ``capacity_plan`` on the device."""
    B = len(counts)
    k = np.arange(cap, dtype=np.int32)
    codes = np.stack([np.tile(np.where(k < c, k, -2).astype(np.int32), N) for c in counts]).reshape(B, N * cap)
    num_pos = sum(min(c, Q) for c in counts)
    num_neg = B * Q - num_pos
    num_tgt = float(N * sum(counts))
    avg = np.array([[num_pos * 1.0 + num_neg * bg, float(num_pos)], [num_tgt, num_tgt]], dtype=np.float32)
    return torch.from_numpy(codes), torch.from_numpy(avg)


def loss_dict(all_cls, all_box, dn_cls, dn_box, boxes, labels, cw, N, dn_weight=1.0, **kw):
    """The head's loss dict (:290-297,434-460) from the split outputs; dn_cls None = no dn_mask_dict.  bg_cls_weight = 0."""
    L, B, Q, _ = all_cls.shape
    counts = [int(b.shape[0]) for b in boxes]
    a = assign(all_cls.detach(), all_box.detach(), boxes, labels, cw)
    num_pos = float(sum(min(c, Q) for c in counts))
    m = set_loss(all_cls, all_box, a, boxes, labels, cw, num_pos, num_pos, **kw)
    out = {}
    if dn_cls is not None:
        num_tgt = float(N * sum(counts))
        d = set_loss(dn_cls, dn_box, dn_codes(counts, N), boxes, labels, cw, num_tgt, num_tgt, scale=dn_weight, **kw)
        out['loss_cls_dn'], out['loss_bbox_dn'] = d[L - 1, 0], d[L - 1, 1]
        for i in range(L - 1):
            out['d%d.loss_cls_dn' % i], out['d%d.loss_bbox_dn' % i] = d[i, 0], d[i, 1]
    out['loss_cls'], out['loss_bbox'] = m[L - 1, 0], m[L - 1, 1]
    for i in range(L - 1):
        out['d%d.loss_cls' % i], out['d%d.loss_bbox' % i] = m[i, 0], m[i, 1]
    return out


def fixture_case(g, tag):
    """The arrays of one recorded case out of the loaded fixture, gt split per sample."""
    c = {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + '_')}
    counts = [int(v) for v in c['counts']]
    offs = np.concatenate([[0], np.cumsum(counts)])
    c['boxes'] = [c['gt_boxes'][offs[i]:offs[i + 1]] for i in range(len(counts))]
    c['labels'] = [c['gt_labels'][offs[i]:offs[i + 1]] for i in range(len(counts))]
    c['counts'] = counts
    c['N'], c['NC'], c['pad'] = int(c['N']), int(c['NC']), int(c['pad_size'])
    return c
