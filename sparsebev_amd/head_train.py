"""Training side of ``SparseBEVHead`` on the device (csrc/head_train.hip): denoising queries, matching cost, set loss.

``SparseBEVTrainHead(SparseBEVHead)`` has the base head's constructor keywords plus the reference config's loss and assigner
settings (``loss_cls``, ``loss_bbox``, ``loss_iou``, ``sync_cls_avg_factor``, ``bg_cls_weight``, ``train_cfg['assigner']`` or
``train_cfg['pts']['assigner']``; configs/r50_nuimg_704x256.py:93-111), the same 51 state-dict keys (a checkpoint moves
between the two classes with ``load_state_dict(strict=True)``) and, in ``eval()``, exactly the base class's behaviour.
In ``train()``:

  * ``forward(mlvl_feats, img_metas)`` (models/sparsebev_head.py:69-117): ground truth from ``img_metas[i]['gt_bboxes_3d']``
    (an object with ``.gravity_center`` and ``.tensor``, or a plain ``[n, 9]`` tensor that is already gravity-centred) and
    ``['gt_labels_3d']``; ONE launch builds denoising + matching queries and the attention mask (``:119-222``), the decoder runs
    its differentiable path, and the outputs are split at ``pad_size`` (``:96-108``);
  * ``loss(gt_bboxes_list, gt_labels_list, preds_dicts)`` (``:405-460``): one cost launch for all layers and samples, ONE
    device -> host copy into pinned memory and ONE synchronisation, the linear sum assignment on the host (the library's own
    solver, as the reference solves it on the host with scipy), then two launches per loss pair (matching, denoising) that
    produce the ``2 * L`` scalars and their gradients together.  With ``assign_on='device'`` the assignment is one more launch
    (csrc/head_assign.hip: the host solver restated in parallel, the same table bit for bit) and ``loss()`` makes no device ->
    host copy and no synchronisation.

Both methods have ONE body that reads the ground truth through one of two sources (``_GroundTruthSource``).  ``GroundTruth`` is the
batch's own upload: every shape follows its counts, and the step's plan (dn codes, averaging factors) is host arithmetic that goes over
in one copy.  ``SparseBEVTrainHead(gt_capacity=C, assign_on='device')`` reads a ``GroundTruthSlab`` instead (``C`` boxes per sample at a
fixed address, refreshed in place): ``single`` is ``C`` and ``pad_size`` is ``C * N`` always, and the plan is one more launch
(``capacity_plan``) that reads the counts on the device -- what ``train_graph.CapturedHeadTrainStep`` needs to replay the whole step as
one graph.  So the capacity path is the dynamic path with ``single`` forced to ``C``: unused pad rows are zero rows inside their
group's attention, and a batch without ground truth keeps its ``*_dn`` keys, at 0.

mmdet's sigmoid ``FocalLoss``, ``L1Loss`` and ``FocalLossCost`` are restated in the kernels (mmdet is not vendored by the
reference: parity is unpinned at that third-party boundary, as the mmcv attention is).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .head import SparseBEVHead, _HEADS, _dev, _p, _register, _stream, head_postprocess
from .parallel import reduce_mean
from .utils import frame_source

_PERM_INV = (0, 1, 4, 2, 3, 5, 6, 7, 8, 9)      # head column j reads decoder column (0, 1, 3, 4, 2, 5, ...)[j]; this is its inverse


class _Stage:
    """Host -> device staging of a step's small arrays: the arrays of one call are packed into ONE page-locked buffer and go over in
    ONE asynchronous copy.  A ring of DEPTH buffers, each with an event that is waited for only when the ring wraps onto a copy
    still in flight; a buffer grows to the next power of two when a call does not fit and is replaced, never added to, so the pinned
    memory held is DEPTH x the largest call ever seen, whatever shapes the ground truth takes from step to step."""

    DEPTH = 16        # a training step makes up to six calls

    def __init__(self):
        self._slots, self._next = [None] * self.DEPTH, 0

    def __call__(self, arrays, device):
        device = torch.device(device)
        arrays = [np.ascontiguousarray(a) for a in arrays]
        if device.type != 'cuda':
            return [torch.from_numpy(a.copy()) for a in arrays]
        offs, total = [], 0
        for a in arrays:
            offs.append(total)
            total += (a.nbytes + 15) // 16 * 16
        if total == 0:
            return [torch.from_numpy(a.copy()).to(device) for a in arrays]
        i = self._next
        self._next = (i + 1) % self.DEPTH
        slot = self._slots[i]
        if slot is None or slot[0].numel() < total:
            slot = self._slots[i] = [torch.empty(max(4096, 1 << (total - 1).bit_length()), dtype=torch.uint8).pin_memory(), torch.cuda.Event()]
        else:
            slot[1].synchronize()
        host = slot[0].numpy()
        for a, o in zip(arrays, offs):
            host[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
        dev = slot[0][:total].to(device, non_blocking=True)
        slot[1].record(torch.cuda.current_stream(device))
        return [dev[o:o + a.nbytes].view(torch.from_numpy(a[:0].reshape(-1)).dtype).view(a.shape) for a, o in zip(arrays, offs)]


_stage = _Stage()


def _i32(t):
    if not t.is_cuda:
        raise RuntimeError('sparsebev_amd.head_train needs device tensors (there is no CPU path)')
    if t.dtype != torch.int32:
        raise RuntimeError('sparsebev_amd.head_train needs int32 index tensors (got %s)' % t.dtype)


def _gt_tensors(boxes_list, labels_list):
    """(boxes as [n,9] tensors, labels as [n] tensors, counts) of what a head is handed as ground truth"""
    boxes = []
    for bx in boxes_list:
        if hasattr(bx, 'gravity_center') and hasattr(bx, 'tensor'):          # duck-typed LiDARInstance3DBoxes (:131-132,421-423)
            bx = torch.cat([bx.gravity_center, bx.tensor[:, 3:]], dim=1)
        bx = torch.as_tensor(bx)
        if bx.dim() != 2 or bx.shape[1] != 9:
            raise ValueError('ground-truth boxes must be [n, 9] (gravity centre, w, l, h, rot, vx, vy), got %s' % (tuple(bx.shape),))
        boxes.append(bx.detach())
    labels = [torch.as_tensor(lb).detach().reshape(-1) for lb in labels_list]
    counts = [int(b.shape[0]) for b in boxes]
    if counts != [int(lb.shape[0]) for lb in labels]:
        raise ValueError('ground-truth boxes and labels disagree in length')
    return boxes, labels, counts


class _GroundTruthSource:
    """What the head's kernels and ``loss()`` read of a batch's ground truth, whichever way it reached the device:

      * device tensors ``boxes`` [G,9] fp32, ``labels`` [G] int32 and ``offsets`` [B+1] int32, the samples concatenated sample-major;
      * ``B`` samples, ``G`` rows, and ``single``, the per-sample row count that every tensor and launch is sized by;
      * on the host ``counts`` (a list of B ints) and ``offsets_host`` (numpy int32 [B+1]), and ``source``: the (boxes, labels) lists
        the contents were built from, where those were recorded.

    ``plan(Q, N, bg_cls_weight)`` is the step's plan: (codes int32 [B, N*single], avg fp32 [2,2], status).  ``codes`` are the denoising
    rows' codes (k at (b, r*single + k) for k < counts[b], -2 elsewhere: prepare_for_dn_loss's gather, :224-237), row 0 of ``avg`` is
    (A_cls, A_box) of the matching loss and row 1 (A, A) of the denoising loss, both before the reduction over the ranks
    (:247,371-384), and ``status`` is None or an int32 [1] tensor of PLAN_* bits."""

    def _set_host(self, counts, source=None):
        self.counts, self.offsets_host, self.source = counts, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), source

    def same_as(self, boxes_list, labels_list):
        """whether these lists hold the very objects this ground truth was built from (``from_metas`` / ``update`` record them)"""
        src = self.source
        return src is not None and len(src[0]) == len(boxes_list) and len(src[1]) == len(labels_list) \
            and all(a is b for a, b in zip(src[0], boxes_list)) and all(a is b for a, b in zip(src[1], labels_list))

    def dn_indices(self, N):
        """the mask_dict's index tensors (interface parity with the reference's; nothing here reads them): none by default"""
        return {}


class GroundTruth(_GroundTruthSource):
    """The batch's ground truth concatenated sample-major on the device: boxes [G,9] fp32, labels [G] int32, offsets [B+1] int32
    and the per-sample counts on the host.  Host-resident ground truth (the data loader's normal case) is concatenated on the host and
    goes over with the offsets in ONE asynchronous pinned upload; device-resident ground truth is concatenated where it is."""

    def __init__(self, boxes_list, labels_list, device):
        boxes, labels, counts = _gt_tensors(boxes_list, labels_list)
        self._set_host(counts)
        self.B, self.G, self.single = len(boxes), sum(counts), max(counts) if boxes else 0
        if all(not t.is_cuda for t in boxes + labels):
            hb = torch.cat([b.float() for b in boxes]).numpy() if boxes else np.zeros((0, 9), np.float32)
            hl = torch.cat([lb.to(torch.int32) for lb in labels]).numpy() if labels else np.zeros(0, np.int32)
            self.boxes, self.labels, self.offsets = _stage([hb, hl, self.offsets_host], device)
        else:
            self.boxes = torch.cat([b.to(device=device, dtype=torch.float32) for b in boxes]).contiguous()
            self.labels = torch.cat([lb.to(device=device, dtype=torch.int32) for lb in labels]).contiguous()
            self.offsets, = _stage([self.offsets_host], device)

    @classmethod
    def from_metas(cls, img_metas, device):
        boxes, labels = [m['gt_bboxes_3d'] for m in img_metas], [m['gt_labels_3d'] for m in img_metas]
        gt = cls(boxes, labels, device)
        gt.source = (boxes, labels)          # loss() reuses this ground truth when it is handed the same objects
        return gt

    def plan(self, Q, N, bg_cls_weight=0.0):
        """the plan from the host's counts: numpy's code table and python doubles rounded once to fp32, in ONE pinned upload"""
        k = np.arange(self.single, dtype=np.int32)
        codes = np.array([np.tile(np.where(k < c, k, -2), N) for c in self.counts], dtype=np.int32).reshape(self.B, N * self.single)
        num_pos = sum(min(c, Q) for c in self.counts)
        num_neg = self.B * Q - num_pos
        num_tgt = float(N * self.G)
        avg = np.array([[num_pos * 1.0 + num_neg * bg_cls_weight, float(num_pos)], [num_tgt, num_tgt]], dtype=np.float32)
        return (*_stage([codes, avg], self.offsets.device), None)

    def dn_indices(self, N):
        G, idx = self.G, np.arange(self.G, dtype=np.int64)
        within = idx - np.repeat(self.offsets_host[:-1].astype(np.int64), self.counts)
        pack = np.concatenate([np.tile(idx, N), np.repeat(np.arange(self.B, dtype=np.int64), self.counts),
                               np.concatenate([within + self.single * r for r in range(N)]) if N else idx[:0]])
        pack, = _stage([pack], self.offsets.device)
        return {'known_indice': pack[:N * G], 'batch_idx': pack[N * G:N * G + G], 'map_known_indice': pack[N * G + G:],
                'known_lbs_bboxes': (self.labels.long().repeat(N), self.boxes.repeat(N, 1))}


class GroundTruthSlab(_GroundTruthSource):
    """``GroundTruth`` at a fixed capacity: boxes [B*capacity, 9] fp32, labels [B*capacity] int32 and offsets [B+1] int32 live in ONE
    device buffer whose address never changes, so a captured graph can read them on every replay.  The samples stay concatenated
    sample-major, as every kernel reads them; the rows behind ``offsets[B]`` are capacity (zero, never read).  ``single`` is the
    capacity and ``G`` is ``B * capacity``: every tensor and launch that is sized by them has the same shape whatever the batch holds,
    and the per-sample counts in ``offsets`` on the device are the only thing that changes.  ``counts`` / ``offsets_host`` are kept for
    host callers; nothing on the capacity path sizes a tensor or a launch by them."""

    def __init__(self, B, capacity, device):
        B, capacity = int(B), int(capacity)
        if B < 0 or capacity < 0:
            raise ValueError('GroundTruthSlab: B = %d, capacity = %d' % (B, capacity))
        self.B, self.capacity, self.single, self.G, self.device = B, capacity, capacity, B * capacity, torch.device(device)
        sizes, self._segs, n = (self.G * 9, self.G, B + 1), [], 0
        for k in sizes:                                  # int32 words, segments padded to 16 bytes
            self._segs.append(n)
            n += (k + 3) // 4 * 4
        self._words = n
        self.buffer = torch.zeros(n, dtype=torch.int32, device=self.device)
        o = self._segs
        self.boxes = self.buffer[o[0]:o[0] + sizes[0]].view(torch.float32).view(self.G, 9)
        self.labels = self.buffer[o[1]:o[1] + sizes[1]]
        self.offsets = self.buffer[o[2]:o[2] + sizes[2]]
        self._set_host([0] * B)

    def __deepcopy__(self, memo):                        # a copy of the head starts with an empty slab of its own
        return GroundTruthSlab(self.B, self.capacity, self.device)

    def update(self, boxes_list, labels_list):
        """Refresh the three buffers in place from one batch (what ``GroundTruth`` accepts; device-resident lists are brought to the
        host, which waits for them): packed on the host, ONE pinned asynchronous upload.  ``ValueError`` before any copy or launch when
        the batch does not fit."""
        boxes, labels, counts = _gt_tensors(boxes_list, labels_list)
        if len(counts) != self.B:
            raise ValueError('ground truth of %d samples for a slab of %d' % (len(counts), self.B))
        if any(c > self.capacity for c in counts):
            raise ValueError('a sample has %d ground-truth boxes, the capacity is %d' % (max(counts), self.capacity))
        if self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('GroundTruthSlab.update inside a graph capture: update the slab before the capture / the replay')
        from .transformer import _upload
        host = np.zeros(self._words, dtype=np.int32)
        total, o = sum(counts), self._segs
        if total:
            host[o[0]:o[0] + total * 9].view(np.float32)[:] = torch.cat([b.float().cpu() for b in boxes]).numpy().reshape(-1)
            host[o[1]:o[1] + total] = torch.cat([lb.to(torch.int32).cpu() for lb in labels]).numpy()
        host[o[2] + 1:o[2] + self.B + 1] = np.cumsum(counts)
        _upload(host, self.device, out=self.buffer)
        self._set_host(counts, (list(boxes_list), list(labels_list)))
        return self

    def plan(self, Q, N, bg_cls_weight=0.0):
        """the plan from the device's counts: one launch, no host value follows the counts"""
        return capacity_plan(self.offsets, self.B, Q, self.single, N, bg_cls_weight)


class _DnQueries(torch.autograd.Function):
    """sbev_head_dn_prepare / sbev_head_dn_prepare_bwd: (query_bbox, query_feat, attn_mask, noised labels) from the two embeddings."""

    @staticmethod
    def forward(ctx, init_w, label_w, gt_boxes, gt_labels, gt_offsets, u_box, u_lab, new_lab, cfg):
        B, N, single, NC, pc_range, box_scale, label_scale = cfg
        _dev(init_w, label_w, gt_boxes, u_box, u_lab)
        _i32(gt_labels), _i32(gt_offsets), _i32(new_lab)
        Q, D, G = init_w.shape[0], label_w.shape[1] + 1, gt_boxes.shape[0]
        if label_w.shape[0] != NC + 1 or u_box.shape != (N * G, 3) or u_lab.shape != (N * G,) or new_lab.shape != (N * G,):
            raise RuntimeError('dn_prepare: label_enc %s / noise shapes do not fit NC=%d, N=%d, G=%d' % (tuple(label_w.shape), NC, N, G))
        T, dev = single * N + Q, init_w.device
        qb = torch.empty(B, T, 10, device=dev, dtype=torch.float32)
        qf = torch.empty(B, T, D, device=dev, dtype=torch.float32)
        mask = torch.empty(T, T, device=dev, dtype=torch.bool)
        noised = torch.empty(N * G, device=dev, dtype=torch.int32)
        rng = (ctypes.c_double * 6)(*[float(v) for v in pc_range])
        iw, lw = init_w.detach().contiguous(), label_w.detach().contiguous()
        st = _lib.load().sbev_head_dn_prepare(_p(iw), _p(lw), _p(gt_boxes.contiguous()), _p(gt_labels.contiguous()), _p(gt_offsets),
                                              _p(u_box.contiguous()), _p(u_lab.contiguous()), _p(new_lab.contiguous()), rng,
                                              float(box_scale), float(label_scale), B, Q, D, NC, G, N, single,
                                              _p(qb), _p(qf), _p(noised), _p(mask), _stream())
        _lib.check(st, 'sbev_head_dn_prepare')
        ctx.save_for_backward(noised)
        ctx.gt_offsets = gt_offsets      # an input without gradient; not a saved tensor: a GroundTruthSlab is refreshed in place between steps
        ctx.dims = (B, Q, D, NC, G, N, single)
        ctx.mark_non_differentiable(mask, noised)
        return qb, qf, mask, noised

    @staticmethod
    def backward(ctx, g_qb, g_qf, _gm, _gn):
        (noised,), gt_offsets = ctx.saved_tensors, ctx.gt_offsets
        B, Q, D, NC, G, N, single = ctx.dims
        T, dev = single * N + Q, noised.device
        g_qb = torch.zeros(B, T, 10, device=dev) if g_qb is None else g_qb.contiguous()
        g_qf = torch.zeros(B, T, D, device=dev) if g_qf is None else g_qf.contiguous()
        _dev(g_qb, g_qf)
        g_init = torch.empty(Q, 10, device=dev, dtype=torch.float32)
        g_label = torch.empty(NC + 1, D - 1, device=dev, dtype=torch.float32)
        st = _lib.load().sbev_head_dn_prepare_bwd(_p(g_qb), _p(g_qf), _p(noised), _p(gt_offsets), B, Q, D, NC, G, N, single,
                                                  _p(g_init), _p(g_label), _stream())
        _lib.check(st, 'sbev_head_dn_prepare_bwd')
        return g_init, g_label, None, None, None, None, None, None, None


def dn_prepare(init_w, label_w, gt, u_box, u_lab, new_lab, B, N, num_classes, pc_range, box_scale=0.5, label_scale=0.5):
    """(query_bbox [B,pad+Q,10], query_feat [B,pad+Q,D], attn_mask bool [pad+Q,pad+Q], noised labels int32 [N*G]); differentiable in
    the two embeddings.  ``gt``: a GroundTruth (``gt.B == B``; one without boxes gives the eval-branch rows only)."""
    if gt.B != B:
        raise ValueError('ground truth of %d samples for a batch of %d' % (gt.B, B))
    return _DnQueries.apply(init_w, label_w, gt.boxes, gt.labels, gt.offsets, u_box, u_lab, new_lab,
                            (B, N, gt.single, num_classes, pc_range, box_scale, label_scale))


class _Denorm(torch.autograd.Function):
    """sbev_head_denorm forward; the backward is its transpose, a column permutation and three scales, in two torch ops."""

    @staticmethod
    def forward(ctx, bbox, pc_range):
        ctx.pc_range = pc_range
        return head_postprocess(bbox, pc_range)

    @staticmethod
    def backward(ctx, g):
        perm, scale = _denorm_constants(g, ctx.pc_range)
        return g.index_select(-1, perm) * scale, None


_DENORM_CONSTANTS = {}


def _denorm_constants(g, r):
    """(column permutation, ten scales) of _Denorm's backward on g's device: uploaded once per range, so that a captured backward holds
    no host -> device copy"""
    key = (g.device, g.dtype, tuple(float(v) for v in r))
    c = _DENORM_CONSTANTS.get(key)
    if c is None:
        c = _DENORM_CONSTANTS[key] = (torch.tensor(_PERM_INV, dtype=torch.long, device=g.device),
                                      g.new_tensor([r[3] - r[0], r[4] - r[1], r[5] - r[2]] + [1.0] * 7))
    return c


def _rows_view(t, last):
    """(tensor to pass, rows per sample of its buffer): a [L,B,R,last] slice along dim 2 of a contiguous [L,B,T,last] tensor is passed
    as it is, with T as the leading dimension; anything else is made contiguous."""
    L, B, R, _ = t.shape
    s = t.stride()
    if s[3] == 1 and s[2] == last and s[1] % last == 0 and s[1] // last >= R and s[0] == B * s[1]:
        return t, s[1] // last
    return t.contiguous(), R


def _rows_views(cls_scores, bbox_preds):
    """(cls, box, rows per sample of both buffers) of a step's [L,B,R,NC] scores and [L,B,R,10] boxes, detached: the two views where they
    agree on the leading dimension, two contiguous copies where they do not"""
    R, NC = cls_scores.shape[2:]
    cls, ld = _rows_view(cls_scores.detach(), NC)
    box, ld2 = _rows_view(bbox_preds.detach(), 10)
    if ld != ld2:
        cls, box, ld = cls.contiguous(), box.contiguous(), R
    return cls, box, ld


def match_cost(cls_scores, bbox_preds, gt, code_weights, w_cls=2.0, w_reg=0.25, alpha=0.25, gamma=2.0):
    """cost [L,B,Q,Gmax] of all decoder layers and samples in one launch (sbev_head_match_cost)."""
    _dev(cls_scores, bbox_preds, code_weights)
    L, B, Q, NC = cls_scores.shape
    cls, box, ld = _rows_views(cls_scores, bbox_preds)
    cost = torch.empty(L, B, Q, gt.single, device=cls.device, dtype=torch.float32)
    st = _lib.load().sbev_head_match_cost(_p(cls), _p(box), ld, _p(gt.boxes), _p(gt.labels), _p(gt.offsets), _p(code_weights.contiguous()),
                                          w_cls, w_reg, alpha, gamma, L, B, Q, NC, gt.single, _p(cost), _stream())
    _lib.check(st, 'sbev_head_match_cost')
    return cost


def lsa_solve(cost):
    """col_of_row (numpy int32, -1 = unmatched) of a host cost matrix (numpy float32 [n_rows, n_cols], rows may be strided)."""
    cost = np.asarray(cost)
    if cost.dtype != np.float32 or cost.ndim != 2 or (cost.size and cost.strides[1] != 4) or (cost.size and cost.strides[0] % 4):
        cost = np.ascontiguousarray(cost, dtype=np.float32)
    n, m = cost.shape
    ld = cost.strides[0] // 4 if cost.size and n > 1 else max(m, 1)
    out = np.full(n, -1, dtype=np.int32)
    st = _lib.load().sbev_lsa_solve(ctypes.c_void_p(cost.ctypes.data), ld, n, m, ctypes.c_void_p(out.ctypes.data))
    _lib.check(st, 'sbev_lsa_solve')
    return out


class _Assigner:
    """Pinned staging of one step's cost matrices and assignment table: one device -> host copy, one synchronisation."""

    def __init__(self):
        self._cost, self._assign, self._event = None, None, None

    # the staging buffers and the event are scratch of the running process: a copy or a pickle of the module starts with none
    def __deepcopy__(self, memo):
        return _Assigner()

    def __getstate__(self):
        return {}

    def __setstate__(self, state):
        self.__init__()

    def __call__(self, cost, gt):
        L, B, Q, Gmax = cost.shape
        n = cost.numel()
        if self._cost is None or self._cost.numel() < n:
            self._cost = torch.empty(n, dtype=torch.float32).pin_memory()
        if self._assign is None or self._assign.numel() < L * B * Q:
            self._assign = torch.empty(L * B * Q, dtype=torch.int32).pin_memory()
            self._event = torch.cuda.Event()
        else:
            self._event.synchronize()                 # the previous step's upload has left the staging buffer
        host = self._cost[:n]
        host.copy_(cost.reshape(-1), non_blocking=True)
        torch.cuda.current_stream(cost.device).synchronize()        # THE synchronisation of the step
        assign = self._assign[:L * B * Q]
        counts = np.asarray(gt.counts, dtype=np.int32)
        st = _lib.load().sbev_head_assign(ctypes.c_void_p(host.data_ptr()), ctypes.c_void_p(counts.ctypes.data), L, B, Q, Gmax,
                                          ctypes.c_void_p(assign.data_ptr()))
        _lib.check(st, 'sbev_head_assign')
        out = assign.to(cost.device, non_blocking=True).view(L, B, Q)
        self._event.record(torch.cuda.current_stream(cost.device))
        return out


def assign_device(cost, gt, status=None):
    """int32 [L,B,Q] on the device: the table ``sbev_head_assign`` returns for the same costs (-1 background, g matched gt of the sample),
    solved by one launch with one workgroup per (layer, sample) that reads the counts from ``gt.offsets`` on the device.  No host copy,
    no synchronisation.  ``status``: an int32 [L*B] device tensor to receive 0 (solved) / 1 (non-finite cost or infeasible: the row is
    all -1), or None."""
    _dev(cost)
    _i32(gt.offsets)
    if cost.dim() != 4 or cost.shape[1] != gt.B:
        raise RuntimeError('assign_device: cost %s is not [L, B=%d, Q, Gmax]' % (tuple(cost.shape), gt.B))
    L, B, Q, Gmax = cost.shape
    if status is not None:
        _i32(status)
        if status.numel() != L * B or not status.is_contiguous():
            raise RuntimeError('assign_device: status must be a contiguous int32 tensor of L * B = %d elements' % (L * B))
    lib, cost = _lib.load(), cost.contiguous()
    nbytes = lib.sbev_head_assign_device_workspace(L, B, Q, Gmax)
    if nbytes < 0:
        raise RuntimeError('assign_device: sizes L=%d B=%d Q=%d Gmax=%d are out of range' % (L, B, Q, Gmax))
    ws = torch.empty(max(1, nbytes), device=cost.device, dtype=torch.uint8)
    out = torch.empty(L, B, Q, device=cost.device, dtype=torch.int32)
    st = lib.sbev_head_assign_device(_p(cost), _p(gt.offsets), L, B, Q, Gmax, _p(out), _p(status), _p(ws), _stream())
    _lib.check(st, 'sbev_head_assign_device')
    return out


class _SetLoss(torch.autograd.Function):
    """sbev_head_set_loss: the [L,2] losses and, from the same launch, their gradients for unit upstream gradient."""

    @staticmethod
    def forward(ctx, cls_scores, bbox_preds, codes, gt_boxes, gt_labels, gt_offsets, code_weights, avg, cfg):
        w_fl, alpha, gamma, w_l1, scale = cfg
        _dev(cls_scores, bbox_preds, code_weights, avg)
        _i32(codes), _i32(gt_offsets)
        L, B, R, NC = cls_scores.shape
        if bbox_preds.shape != (L, B, R, 10) or avg.numel() != 2 or code_weights.numel() != 10:
            raise RuntimeError('set_loss: shapes %s / %s do not fit' % (tuple(cls_scores.shape), tuple(bbox_preds.shape)))
        if codes.dim() == 2 and codes.shape == (B, R):
            stride = 0
        elif codes.shape == (L, B, R):
            stride = B * R
        else:
            raise RuntimeError('set_loss: codes %s is neither [B,R] nor [L,B,R]' % (tuple(codes.shape),))
        cls, box, ld = _rows_views(cls_scores, bbox_preds)
        dev, lib = cls.device, _lib.load()
        loss = torch.empty(L, 2, device=dev, dtype=torch.float32)
        finite = torch.empty(L, 2, device=dev, dtype=torch.float32)
        d_cls = torch.empty(L, B, R, NC, device=dev, dtype=torch.float32)
        d_box = torch.empty(L, B, R, 10, device=dev, dtype=torch.float32)
        ws = torch.empty(max(1, L * lib.sbev_head_set_loss_workspace(B, R) // 4), device=dev, dtype=torch.float32)
        st = lib.sbev_head_set_loss(_p(cls), _p(box), ld, _p(codes.contiguous()), stride, _p(gt_boxes), _p(gt_labels), _p(gt_offsets),
                                    _p(code_weights.contiguous()), _p(avg), w_fl, alpha, gamma, w_l1, scale, L, B, R, NC,
                                    _p(loss), _p(finite), _p(d_cls), _p(d_box), _p(ws), _stream())
        _lib.check(st, 'sbev_head_set_loss')
        ctx.save_for_backward(finite, d_cls, d_box)
        return loss

    @staticmethod
    def backward(ctx, g):
        finite, d_cls, d_box = ctx.saved_tensors
        g = g * finite                                   # torch.nan_to_num passes no gradient where it replaced the value
        return d_cls * g[:, 0].view(-1, 1, 1, 1), d_box * g[:, 1].view(-1, 1, 1, 1), None, None, None, None, None, None, None


def set_loss(cls_scores, bbox_preds, codes, gt, code_weights, avg, w_fl=2.0, alpha=0.25, gamma=2.0, w_l1=0.25, scale=1.0):
    """[L,2] (loss_cls, loss_bbox) per layer; ``codes`` int32 [B,R] or [L,B,R] (-2 skip, -1 background, g target gt g of the sample),
    ``avg`` a device tensor [A_cls, A_box] (clamped to >= 1 in the kernel)."""
    return _SetLoss.apply(cls_scores, bbox_preds, codes, gt.boxes, gt.labels, gt.offsets, code_weights, avg,
                          (float(w_fl), float(alpha), float(gamma), float(w_l1), float(scale)))


PLAN_COUNT_ABOVE_CAPACITY, PLAN_OFFSETS_NOT_MONOTONE, PLAN_TOTAL_ABOVE_CAPACITY = 1, 2, 4      # bits of capacity_plan's status


def capacity_plan(gt_offsets, B, Q, capacity, N, bg_cls_weight=0.0):
    """(codes int32 [B, N*capacity], avg fp32 [2,2], status int32 [1]) of a step at a fixed ground-truth capacity, from the counts in
    ``gt_offsets`` on the device (sbev_head_capacity_plan): the denoising rows' codes, (A_cls, A_box) of the matching and of the
    denoising loss, and 0 or PLAN_* bits.  One launch, no host copy."""
    _i32(gt_offsets)
    if gt_offsets.numel() != B + 1 or not gt_offsets.is_contiguous():
        raise RuntimeError('capacity_plan: gt_offsets must be a contiguous int32 tensor of B + 1 = %d elements' % (B + 1))
    dev = gt_offsets.device
    codes = torch.empty(B, N * capacity, device=dev, dtype=torch.int32)
    avg = torch.empty(2, 2, device=dev, dtype=torch.float32)
    status = torch.empty(1, device=dev, dtype=torch.int32)
    st = _lib.load().sbev_head_capacity_plan(_p(gt_offsets), B, Q, capacity, N, float(bg_cls_weight), _p(codes), _p(avg), _p(status), _stream())
    _lib.check(st, 'sbev_head_capacity_plan')
    return codes, avg, status


def reduce_avg(pair, sync_cls=True):
    """a device [A_cls, A_box] averaged over the ranks where the reference does (:247,371-384): A_box always, A_cls with
    ``sync_cls_avg_factor`` (the denoising pair: always)"""
    return reduce_mean(pair) if sync_cls else torch.stack([pair[0], reduce_mean(pair[1:2])[0]])


def _named(out, losses, suffix):
    """the reference's keys for an [L,2] loss tensor: the last layer's pair first, then d0.. (:290-297,448-460)"""
    L = losses.shape[0]
    out['loss_cls' + suffix], out['loss_bbox' + suffix] = losses[L - 1, 0], losses[L - 1, 1]
    for i in range(L - 1):
        out['d%d.loss_cls%s' % (i, suffix)], out['d%d.loss_bbox%s' % (i, suffix)] = losses[i, 0], losses[i, 1]


def _typed(cfg, default_type, allowed, what):
    cfg = dict(cfg or {})
    kind = cfg.pop('type', default_type)
    if kind not in allowed:
        raise ValueError('sparsebev_amd.SparseBEVTrainHead: %s type %r is not supported (%s)' % (what, kind, ' / '.join(allowed)))
    return kind, cfg


class SparseBEVTrainHead(SparseBEVHead):
    """``SparseBEVHead`` that trains (models/sparsebev_head.py:14-460).  The xyz de-normalisation of the training forward runs
    ``sbev_head_denorm`` behind an autograd Function whose backward is a column permutation and scale in torch ops."""

    def __init__(self, *args, loss_cls=None, loss_bbox=None, loss_iou=None, sync_cls_avg_factor=True, bg_cls_weight=0.0,
                 train_cfg=None, assign_on='host', gt_capacity=None, **kwargs):
        if assign_on not in ('host', 'device'):
            raise ValueError("sparsebev_amd.SparseBEVTrainHead: assign_on is 'host' or 'device', not %r" % (assign_on,))
        if gt_capacity is not None:
            if isinstance(gt_capacity, bool) or not isinstance(gt_capacity, (int, np.integer)) or gt_capacity < 0:
                raise ValueError('sparsebev_amd.SparseBEVTrainHead: gt_capacity is None or a non-negative integer, not %r' % (gt_capacity,))
            if assign_on != 'device':
                raise ValueError("sparsebev_amd.SparseBEVTrainHead: gt_capacity needs assign_on='device' (the host solver reads the counts)")
        _, fl = _typed(loss_cls, 'FocalLoss', ('FocalLoss',), 'loss_cls')
        if not fl.get('use_sigmoid', True):
            raise ValueError('sparsebev_amd.SparseBEVTrainHead: loss_cls must be the sigmoid FocalLoss')
        _, l1 = _typed(loss_bbox, 'L1Loss', ('L1Loss',), 'loss_bbox')
        _, iou = _typed(loss_iou, 'GIoULoss', ('GIoULoss',), 'loss_iou')
        if float(iou.get('loss_weight', 0.0)) != 0.0:
            raise ValueError('sparsebev_amd.SparseBEVTrainHead: loss_iou is accepted at weight 0 only')
        tc = dict(train_cfg or {})
        assigner = dict(tc.get('assigner') or (tc.get('pts') or {}).get('assigner') or {})
        if assigner.pop('type', 'HungarianAssigner3D') != 'HungarianAssigner3D':
            raise ValueError('sparsebev_amd.SparseBEVTrainHead: the assigner is HungarianAssigner3D')
        _, cc = _typed(assigner.get('cls_cost'), 'FocalLossCost', ('FocalLossCost',), 'cls_cost')
        _, rc = _typed(assigner.get('reg_cost'), 'BBox3DL1Cost', ('BBox3DL1Cost',), 'reg_cost')
        _, ic = _typed(assigner.get('iou_cost'), 'IoUCost', ('IoUCost',), 'iou_cost')
        if float(ic.get('weight', 0.0)) != 0.0:
            raise ValueError('sparsebev_amd.SparseBEVTrainHead: iou_cost is accepted at weight 0 only')
        super().__init__(*args, train_cfg=train_cfg, **kwargs)
        self.loss_cls_weight, self.focal_gamma, self.focal_alpha = float(fl.get('loss_weight', 2.0)), float(fl.get('gamma', 2.0)), float(fl.get('alpha', 0.25))
        self.loss_bbox_weight = float(l1.get('loss_weight', 0.25))
        self.cls_cost_weight, self.reg_cost_weight = float(cc.get('weight', 2.0)), float(rc.get('weight', 0.25))
        self.cost_alpha, self.cost_gamma = float(cc.get('alpha', 0.25)), float(cc.get('gamma', 2.0))
        self.sync_cls_avg_factor, self.bg_cls_weight = bool(sync_cls_avg_factor), float(bg_cls_weight)
        self.dn_weight, self.dn_bbox_noise_scale, self.dn_label_noise_scale = 1.0, 0.5, 0.5        # :45-47
        self._assigner = _Assigner()
        # where the linear sum assignment is solved: 'host' (one copy + one synchronisation per step) or 'device' (one launch, neither)
        self.assign_on = assign_on
        self.assign_status = None            # 'device': the last launch's int32 [L*B] status; nobody reads it on the hot path
        # None: every shape follows the batch's ground truth.  An integer: the ground truth lives in a GroundTruthSlab of that many boxes
        # per sample, pad_size is gt_capacity * dn_group_num always, and the counts are read on the device only
        self.gt_capacity = None if gt_capacity is None else int(gt_capacity)
        self.plan_status = None              # gt_capacity: the last plan launch's int32 [1] status (PLAN_* bits)
        self.dn_noise = None                 # (u_box, u_lab, new_lab) for forward() to read instead of drawing (a captured step's static tensors)
        self.decoder_ctx = None              # a transformer.DecoderContext for forward() to use instead of uploading img_metas (the same)
        self._slab = None

    # ---- section 1: denoising queries ------------------------------------------------------------------------------
    def draw_noise(self, G, device):
        """(u_box [N*G,3] in [-1,1), u_lab [N*G] in [0,1), new_lab int32 [N*G] in [0,NC)) from torch's device generator."""
        n = self.dn_group_num * G
        return (torch.rand(n, 3, device=device) * 2 - 1.0, torch.rand(n, device=device),
                torch.randint(0, self.num_classes, (n,), device=device, dtype=torch.int32))

    def gt_slab(self, B, device):
        """the head's GroundTruthSlab for batches of B samples (gt_capacity boxes each), made on first use"""
        device = torch.device(device)
        if self._slab is None or self._slab.B != B or self._slab.device != device:
            self._slab = GroundTruthSlab(B, self.gt_capacity, device)
        return self._slab

    def _forward_gt(self, batch_size, img_metas, device, dn):
        """the ground-truth source of a forward: an empty one without denoising, the batch's own upload, or at ``gt_capacity`` the head's
        slab refreshed in place"""
        if not dn:
            return GroundTruth([torch.zeros(0, 9)] * batch_size, [torch.zeros(0, dtype=torch.int32)] * batch_size, device)
        if self.gt_capacity is None:
            return GroundTruth.from_metas(img_metas, device)
        slab = self.gt_slab(batch_size, device)
        boxes, labels = [m['gt_bboxes_3d'] for m in img_metas], [m['gt_labels_3d'] for m in img_metas]
        if not (torch.cuda.is_current_stream_capturing() and slab.same_as(boxes, labels)):
            slab.update(boxes, labels)               # under capture the slab holds these objects already, or update() refuses
        return slab

    def prepare_for_dn_input(self, batch_size, init_query_bbox, label_enc, img_metas, noise=None):
        """:119-222 -> (query_bbox, query_feat, attn_mask, mask_dict).  ``noise``: (u_box, u_lab, new_lab) to replay a recorded case.
        The mask_dict holds pad_size (``single * N``), the source (``'gt'``) and, where the source has them, the reference's index tensors."""
        device = init_query_bbox.device
        label_w = label_enc.weight if hasattr(label_enc, 'weight') else label_enc
        dn = self.training and self.dn_enabled
        gt = self._forward_gt(batch_size, img_metas, device, dn)
        N = self.dn_group_num if dn else 1
        if noise is None and dn:
            noise = self.dn_noise
        if noise is None:
            noise = self.draw_noise(gt.G, device) if dn else (torch.zeros(0, 3, device=device), torch.zeros(0, device=device),
                                                              torch.zeros(0, dtype=torch.int32, device=device))
        u_box, u_lab, new_lab = [t.to(device) for t in noise]
        qb, qf, mask, _ = dn_prepare(init_query_bbox, label_w, gt, u_box.float(), u_lab.float(), new_lab.to(torch.int32), batch_size, N,
                                     self.num_classes, self.pc_range, self.dn_bbox_noise_scale, self.dn_label_noise_scale)
        if not dn:
            return qb, qf, None, None
        return qb, qf, mask, dict(gt.dn_indices(N), pad_size=gt.single * N, gt=gt)

    # ---- section 2: training forward ------------------------------------------------------------------------------------
    def forward(self, mlvl_feats, img_metas):
        if not self.training:
            return super().forward(mlvl_feats, img_metas)
        B = mlvl_feats[0].shape[0] if frame_source(mlvl_feats).kind == 'list' else mlvl_feats.B
        query_bbox, query_feat, attn_mask, mask_dict = self.prepare_for_dn_input(B, self.init_query_bbox.weight, self.label_enc, img_metas)
        if self.decoder_ctx is None:
            cls_scores, bbox_preds = self.transformer(query_bbox, query_feat, mlvl_feats, attn_mask=attn_mask, img_metas=img_metas)
        else:                                    # SparseBEVTransformer.forward's training path on an uploaded context
            from .transformer import FeaturePyramid
            cls_scores, bbox_preds = self.transformer.decoder.forward_differentiable(query_bbox, query_feat, mlvl_feats, FeaturePyramid(list(mlvl_feats)),
                                                                                     attn_mask, self.decoder_ctx)
            cls_scores, bbox_preds = torch.nan_to_num(cls_scores), torch.nan_to_num(bbox_preds)
        bbox_preds = _Denorm.apply(bbox_preds, self.pc_range)
        outs = {'all_cls_scores': cls_scores, 'all_bbox_preds': bbox_preds, 'enc_cls_scores': None, 'enc_bbox_preds': None}
        if mask_dict is not None and mask_dict['pad_size'] > 0:
            pad = mask_dict['pad_size']
            mask_dict['output_known_lbs_bboxes'] = (cls_scores[:, :, :pad, :], bbox_preds[:, :, :pad, :])
            outs.update(all_cls_scores=cls_scores[:, :, pad:, :], all_bbox_preds=bbox_preds[:, :, pad:, :], dn_mask_dict=mask_dict)
        return outs

    # ---- sections 3-5: assignment and losses --------------------------------------------------------------------------
    def assign(self, all_cls_scores, all_bbox_preds, gt):
        """int32 [L,B,Q]: -1 background, g = index of the matched gt of that sample (:301-347 for every layer and sample)."""
        L, B, Q, _ = all_cls_scores.shape
        if gt.G == 0 or Q == 0:
            return torch.full((L, B, Q), -1, dtype=torch.int32, device=all_cls_scores.device)
        cost = match_cost(all_cls_scores, all_bbox_preds, gt, self.code_weights, self.cls_cost_weight, self.reg_cost_weight,
                          self.cost_alpha, self.cost_gamma)
        if self.assign_on == 'device':
            self.assign_status = torch.empty(L * B, dtype=torch.int32, device=cost.device)
            return assign_device(cost, gt, self.assign_status)
        return self._assigner(cost, gt)

    def loss(self, gt_bboxes_list, gt_labels_list, preds_dicts, gt_bboxes_ignore=None):
        """:405-460.  The matching pair reads the ground truth of these arguments, the denoising pair the forward's (``md['gt']``, as
        the reference reads its mask dict).  They are one source when the forward was handed the same objects, and always at
        ``gt_capacity``, where the slab is refreshed in place; then there is one plan."""
        assert gt_bboxes_ignore is None, '%s only supports for gt_bboxes_ignore setting to None.' % self.__class__.__name__
        all_cls, all_box = preds_dicts['all_cls_scores'], preds_dicts['all_bbox_preds']
        L, B, Q, _ = all_cls.shape
        md = preds_dicts.get('dn_mask_dict')
        at_capacity = self.gt_capacity is not None
        gt = md['gt'] if md is not None else self.gt_slab(B, all_cls.device) if at_capacity else None
        if not at_capacity and (gt is None or not gt.same_as(gt_bboxes_list, gt_labels_list)):
            gt = GroundTruth(gt_bboxes_list, gt_labels_list, all_cls.device)
        if gt.B != B:
            raise ValueError('ground truth of %d samples for a batch of %d' % (gt.B, B))
        if at_capacity and not gt.same_as(gt_bboxes_list, gt_labels_list):
            gt.update(gt_bboxes_list, gt_labels_list)
        assign = self.assign(all_cls, all_box, gt)
        dgt = md['gt'] if md is not None else gt
        N = max(md['pad_size'] // max(dgt.single, 1), 1) if md is not None else 1
        codes, avg, status = gt.plan(Q, N, self.bg_cls_weight)
        if status is not None:
            self.plan_status = status
        # other objects than the forward's: the dn pair keeps the forward's codes and factors
        dn_codes, dn_avg = (codes, avg) if dgt is gt else dgt.plan(Q, N, self.bg_cls_weight)[:2]
        losses = set_loss(all_cls, all_box, assign, gt, self.code_weights, reduce_avg(avg[0], self.sync_cls_avg_factor), self.loss_cls_weight,
                          self.focal_alpha, self.focal_gamma, self.loss_bbox_weight, 1.0)
        out = {}
        if md is not None:
            dn_cls, dn_box = md['output_known_lbs_bboxes']
            dn = set_loss(dn_cls, dn_box, dn_codes, dgt, self.code_weights, reduce_avg(dn_avg[1]), self.loss_cls_weight, self.focal_alpha,
                          self.focal_gamma, self.loss_bbox_weight, self.dn_weight)
            _named(out, dn, '_dn')
        _named(out, losses, '')
        return out


SparseBEVTrainHead = _register(_HEADS, SparseBEVTrainHead)
