"""One training step of the decoder -- forward + backward through all layers -- as ONE hipGraph replay.

The differentiable path (transformer.forward_differentiable, sparsebev_amd.autograd) is ~550 kernel launches per step at config 2;
issued one by one from Python and the autograd engine they cost 10.5-11.2 ms for 8.6 ms of kernel time.  Captured once and replayed,
the same launches take 8.2 ms (tools/bench_train.py --graph; profiles/r4_train_step.log), with gradients bit-identical to the eager
step's.  This is torch.cuda.graphs' whole-network recipe; what this module adds is what the decoder needs to be capturable:

  * the per-call constants (camera matrices, time stamps: host data in ``img_metas``) are uploaded OUTSIDE the graph into one device
    buffer that later steps refresh in place (transformer.DecoderContext(..., out=buffer));
  * everything -- warm-up, capture, replay -- runs on ONE side stream: the parameters' AccumulateGrad nodes remember the stream they
    were created on, and a backward under capture that has to hop to another, non-capturing stream does not end with an error but
    with a crash inside hipStreamEndCapture; the warm-up watches for torch's stream-mismatch warning and refuses to capture instead;
  * dropout: the differentiable path draws one host seed per layer call, which a capture freezes -- so with dropout on, the step is
    captured with a DEVICE seed installed (autograd.device_seed): every dropout launch hashes host seed + one int64 word in device
    memory, and ``replay`` draws a new word (one small torch launch, torch's CUDA generator) before it replays the graph.  Forward and
    backward of a step see the same word.

  * the feature-gradient mode (ops.deterministic_feature_grad, or torch.use_deterministic_algorithms) is whatever is on at capture;
    ``replay`` refuses to run the graph under the other one.

  * derived weight images: W^T for grad_x, the fp16 fragment images of the two mixing weights and the packed rows are cached per
    process, keyed on the parameters' ``_version`` (autograd._transposed / _f16_frags, dense._cat_rows).  A capture on warm caches
    would record no transpose and no pack and replay on the images of the weights AS THEY WERE AT CAPTURE, whatever an optimizer has
    done since.  So warm-up, capture and therefore every replay run inside ``autograd.step_images()``: each image is derived once per
    step by launches of the step itself, from the capture's pool, and the caches are neither read nor filled.

Inputs are STATIC tensors: write the next batch into them with ``copy_()`` (the features, the queries), pass the next ``img_metas`` to
``replay``.  Gradients land in the same ``.grad`` tensors every replay and OVERWRITE them (they were ``None`` at capture); never
``zero_grad(set_to_none=True)`` -- that would detach ``.grad`` from the graph's buffers.

The parameter update: either any optimizer after ``replay()`` (in-place updates are seen by the next replay, see above), or
``optimizer=optim.FusedAdamW(...)`` over exactly the captured parameters, whose three launches (gradient norm, header, AdamW with
clipping / loss scale / overflow skip: csrc/optim.hip) then END the captured step.  The warm-up runs them with the optimizer's ``hold``
word set -- the skip path a non-finite norm takes: kernels loaded and exercised, nothing written -- and the capture pass executes
nothing, so construction leaves parameters, moments and counters bit-identical (``skipped`` is reset).  ``replay`` refreshes lr /
weight_decay / scale in the optimizer's device buffer from ``param_groups`` next to the camera block, and bumps every parameter's
``_version`` after the graph (the launches write through raw pointers).  ``step.grads`` after a replay are the gradients the update
consumed.  With ``optimizer=`` a process group of more than one rank is refused: DDP's gradient all-reduce is not in the graph.

``CapturedHeadTrainStep`` does the same for the training head's whole step (dn prepare, decoder forward + backward, denorm, matching
cost, assignment, plan, both set-loss calls, the embeddings' backward) on a ``SparseBEVTrainHead(gt_capacity=...)``: there the ground
truth is one more per-call constant, a ``head_train.GroundTruthSlab`` refreshed in place outside the graph, with the dn noise beside it.

``CapturedDetectorTrainStep`` is the whole detector's step (``detector.SparseBEV``): image front end, backbone, neck, the head's step,
their backward and the update.  The backbone's and the neck's weight packs are derived images like the ones above: inside ``step_images()``
they are made by the step's own launches (resnet.py, fpn.py).

Reference counterpart: the training loop around SparseBEVTransformer.forward (models/sparsebev_transformer.py:86-101) and its
backward through msmv_sampling (models/csrc/wrapper.py:51-61); the reference has no graph capture.
"""
import warnings

import torch

from . import autograd as AG
from . import ops
from .transformer import DecoderContext, FeaturePyramid, _upload
from .utils import VERSION

class _CapturedStep:
    """What the captured steps share: ONE side stream for warm-up, capture and replay, the warm-up that watches for torch's
    stream-mismatch warning, the dropout word in device memory, and the refusal to replay under another feature-gradient mode.
    A subclass sets ``device``, ``_leaves`` and ``dropout``, implements ``_run()`` (one step: forward, loss, backward; returns what
    ``replay`` hands out) and calls ``_capture(warmup)`` once.  ``captures`` counts the graph captures of the object."""

    captures = 0

    optimizer = None

    def _refuse_ranks(self, optimizer, always=None):
        """First thing in a constructor, in a process group of more than one rank: DDP's gradient all-reduce is not in the graph, so an
        in-graph optimizer would step on one rank's gradients; ``always`` is a step's reason to refuse such a group without one too."""
        dist = torch.distributed
        if (optimizer is not None or always) and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            what, why = ('', always) if optimizer is None else \
                ('optimizer= with ', 'the gradient all-reduce is not in the graph (run the optimizer after replay() and the all-reduce)')
            raise RuntimeError('%s: %sa process group of %d ranks: %s' % (type(self).__name__, what, dist.get_world_size(), why))

    def _bind_optimizer(self, optimizer, params):
        """``optimizer=``: a FusedAdamW over exactly the captured parameters becomes the tail of the step."""
        if optimizer is None:
            return
        from .optim import FusedAdamW
        who = type(self).__name__
        if not isinstance(optimizer, FusedAdamW):
            raise TypeError('%s: optimizer= takes a sparsebev_amd.optim.FusedAdamW (its three launches are capturable); run any other '
                            'optimizer after replay()' % who)
        mine, theirs = {id(p) for p in params}, {id(p) for p, _ in optimizer._params()}
        if mine != theirs:
            raise ValueError('%s: the optimizer must hold exactly the captured trainable parameters (%d captured, %d in the optimizer, '
                             '%d in both)' % (who, len(mine), len(theirs), len(mine & theirs)))
        self.optimizer = optimizer

    def _capture(self, warmup):
        who = type(self).__name__
        opt = self.optimizer
        # the part of the dropout seeds that changes from replay to replay (see the module text); None without dropout
        self.seed_dev = torch.zeros(1, dtype=torch.int64, device=self.device).random_() if self.dropout else None
        # captured-under setting: the graph holds the launches of ONE feature-gradient mode (atomics, or the sorted-tap sum)
        self.det_feat_grad = ops.deterministic_feature_grad_active()
        self.stream = torch.cuda.Stream(device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            if opt is not None:      # warm-up steps run the optimizer's launches on the skip path: loaded and exercised, nothing written
                opt.hold = True
                opt.push_hyper()
            mismatch = False
            for i in range(max(1, warmup)):
                self._clear_grads()
                with warnings.catch_warnings(record=True) as seen:
                    warnings.simplefilter('always')
                    self._step()
                mismatch = any('AccumulateGrad' in str(w.message) and 'stream' in str(w.message) for w in seen)
            if mismatch:
                raise RuntimeError("%s: a parameter's AccumulateGrad node still belongs to another stream (an autograd graph "
                                   'of an earlier eager step is alive); capturing now would crash inside HIP.  Drop the references to earlier '
                                   'losses / outputs, or build the captured step before the first eager step.' % who)
            self._clear_grads()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=self.stream):
                out = self._step()
            self.captures += 1
            if opt is not None:
                opt.hold = False
                opt.push_hyper()
                opt.skipped.zero_()          # the warm-up's skips are not the caller's
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return out

    def _clear_grads(self):
        for t in self._leaves:
            t.grad = None

    def _step(self):
        # step_images: every derived weight image (W^T, fp16 fragments, packed rows) is made by launches of the step itself, so a replay
        # reads the weights as they are then -- never an image cached before the capture
        with AG.device_seed(self.seed_dev), AG.step_images():
            out = self._run()
            if self.optimizer is not None:
                self.optimizer.step()
            return out

    def _replay_graph(self):
        if self.optimizer is not None:
            self.optimizer.push_hyper()      # lr / weight_decay / scale from the groups: outside the graph, like the camera block
        self.graph.replay()
        if self.optimizer is not None:
            self.optimizer.bump_versions()   # the graph wrote the parameters through raw pointers

    def _check_feature_grad_mode(self):
        if ops.deterministic_feature_grad_active() != self.det_feat_grad:
            raise RuntimeError('%s.replay: the step was captured with the deterministic feature gradient %s and it is %s now '
                               '(ops.deterministic_feature_grad / torch.use_deterministic_algorithms); capture a new step'
                               % (type(self).__name__, ('off', 'on')[self.det_feat_grad], ('on', 'off')[self.det_feat_grad]))

    def _refresh_cameras(self, img_metas):
        packed, layout, image_h, image_w = DecoderContext.pack(img_metas, self.B)
        if layout != self.ctx.layout or (image_h, image_w) != (self.ctx.image_h, self.ctx.image_w):
            raise ValueError('%s.replay: img_metas with another shape than the captured step (frames, cameras, image size)' % type(self).__name__)
        _upload(packed, self.device, out=self.ctx.buffer)          # in place: the graph reads this buffer


class CapturedTrainStep(_CapturedStep):
    """``step = CapturedTrainStep(model, query_bbox, query_feat, mlvl_feats, img_metas, loss_fn)`` captures
    ``loss_fn(*model(...)).backward()``; ``loss, cls_scores, bbox_preds = step.replay(img_metas)`` runs it again on the current contents
    of the (static) input tensors.  ``step.grads`` maps parameter names to the static gradient tensors, ``step.input_grads`` holds
    ``query_feat.grad`` / the feature gradients where those inputs require grad.  ``optimizer``: a FusedAdamW over the decoder's
    trainable parameters; its update becomes the tail of the graph (module text)."""

    def __init__(self, model, query_bbox, query_feat, mlvl_feats, img_metas, loss_fn, attn_mask=None, warmup=3, optimizer=None):
        self._refuse_ranks(optimizer)
        if not torch.is_grad_enabled():
            raise RuntimeError('CapturedTrainStep: grad is disabled')
        VERSION.require_supported()
        self.model = model
        self.decoder = dec = model.decoder if hasattr(model, 'decoder') else model
        layer = dec.decoder_layer
        self.dropout = bool(dec.training and (layer.self_attn.attn_drop > 0 or layer.ffn_drop > 0))
        if not (query_bbox.is_cuda and query_bbox.dtype == torch.float32 and query_bbox.is_contiguous()
                and query_feat.dtype == torch.float32 and query_feat.is_contiguous()):
            raise ValueError('CapturedTrainStep: query_bbox / query_feat must be contiguous fp32 CUDA tensors (they are read in place)')
        self.query_bbox, self.query_feat, self.attn_mask = query_bbox, query_feat, attn_mask
        self.mlvl_feats = list(mlvl_feats)
        self.loss_fn = loss_fn
        self.B = query_bbox.shape[0]
        self.device = query_bbox.device
        self.ctx = DecoderContext(img_metas, self.B, self.device)          # host -> device: outside the graph
        self._leaves = [p for p in dec.parameters() if p.requires_grad]
        self._bind_optimizer(optimizer, self._leaves)
        self._leaves += [t for t in [query_feat, query_bbox] + self.mlvl_feats if t.requires_grad]
        self.loss, self.cls_scores, self.bbox_preds = self._capture(warmup)
        self.grads = {n: p.grad for n, p in dec.named_parameters() if p.grad is not None}
        self.input_grads = {'query_feat': query_feat.grad, 'mlvl_feats': [f.grad for f in self.mlvl_feats]}

    def _run(self):
        dec = self.decoder
        pyr = FeaturePyramid(list(self.mlvl_feats))          # the NCHW -> NHWC relayout: device work, part of the step
        cls, box = dec.forward_differentiable(self.query_bbox, self.query_feat, list(self.mlvl_feats), pyr, self.attn_mask, self.ctx)
        if dec is not self.model:                           # SparseBEVTransformer.forward's nan_to_num
            cls, box = torch.nan_to_num(cls), torch.nan_to_num(box)
        loss = self.loss_fn(cls, box)
        loss.backward()
        return loss.detach(), cls.detach(), box.detach()

    def replay(self, img_metas=None, new_masks=True):
        """Run the captured step on the current contents of the static inputs; ``img_metas`` (same batch size, frame and camera
        counts) refreshes the camera matrices / time stamps first; with dropout on, new masks are drawn unless ``new_masks=False``
        (``seed_dev`` may also be set by hand).  Returns the graph's own (loss, cls_scores, bbox_preds) tensors -- clone what has to
        survive the next replay."""
        self._check_feature_grad_mode()
        if img_metas is not None:
            self._refresh_cameras(img_metas)
        if self.seed_dev is not None and new_masks:
            self.seed_dev.random_()
        self._replay_graph()
        return self.loss, self.cls_scores, self.bbox_preds


class CapturedHeadTrainStep(_CapturedStep):
    """``step = CapturedHeadTrainStep(head, mlvl_feats, img_metas)`` captures the training head's whole step --
    ``outs = head(mlvl_feats, img_metas)``, ``losses = head.loss(gt_bboxes, gt_labels, outs)``, ``sum(losses.values()).backward()`` -- as
    one graph: the dn prepare, the decoder forward and backward, the denorm, the matching cost, the assignment, the plan, both set-loss
    calls and the embeddings' backward.  ``head``: a ``SparseBEVTrainHead(gt_capacity=...)`` in ``train()`` with denoising on; the
    ground truth is ``img_metas[i]['gt_bboxes_3d'] / ['gt_labels_3d']``.  What changes from step to step lives in static device memory
    that ``replay`` refreshes OUTSIDE the graph: the head's ``GroundTruthSlab``, the camera block, the dn noise, the dropout word; the
    features are the static tensors of ``mlvl_feats`` (write the next batch into them with ``copy_()``).

    ``step.grads`` maps every trainable parameter of the head (``init_query_bbox.weight`` and ``label_enc.weight`` included) to its
    static gradient tensor; ``step.captures`` stays 1.  One capacity per object: the graph owns the parameters' ``.grad``, and several
    capacity buckets would have to share them.  A process group of more than one rank is refused: the averaging factors' all-reduce
    would have to be captured.  ``optimizer``: a FusedAdamW over the head's trainable parameters; its update becomes the tail of the
    graph (module text)."""

    def __init__(self, head, mlvl_feats, img_metas, warmup=3, optimizer=None):
        from .head_train import SparseBEVTrainHead
        self._refuse_ranks(optimizer, always='the all-reduce of the averaging factors cannot be captured (run the eager step)')
        if not torch.is_grad_enabled():
            raise RuntimeError('CapturedHeadTrainStep: grad is disabled')
        VERSION.require_supported()
        if not isinstance(head, SparseBEVTrainHead) or head.gt_capacity is None:
            raise ValueError('CapturedHeadTrainStep: the head must be a SparseBEVTrainHead(gt_capacity=...): at a dynamic shape nothing can be replayed')
        if not (head.training and head.dn_enabled):
            raise ValueError('CapturedHeadTrainStep: the head must be in train() mode with query denoising on')
        self.head = head
        self.mlvl_feats = list(mlvl_feats)
        if not all(torch.is_tensor(f) and f.is_cuda and f.dtype == torch.float32 for f in self.mlvl_feats):
            raise ValueError('CapturedHeadTrainStep: mlvl_feats must be a list of fp32 CUDA tensors (they are read in place)')
        self._bind_head(head, self.mlvl_feats[0].shape[0], self.mlvl_feats[0].device, img_metas)
        params = [p for p in head.parameters() if p.requires_grad]
        self._bind_optimizer(optimizer, params)
        self._leaves = params + [f for f in self.mlvl_feats if f.requires_grad]
        self.losses = self._capture(warmup)
        self.grads = {n: p.grad for n, p in head.named_parameters() if p.grad is not None}
        self.input_grads = {'mlvl_feats': [f.grad for f in self.mlvl_feats]}

    def _bind_head(self, head, B, device, img_metas):
        """what a step through the training head keeps in static device memory: the ground-truth slab, the camera block, the dn noise"""
        self.B, self.device = B, device
        layer = head.transformer.decoder.decoder_layer
        self.dropout = bool(layer.self_attn.attn_drop > 0 or layer.ffn_drop > 0)
        self.slab = head.gt_slab(self.B, self.device)
        self._set_ground_truth([m['gt_bboxes_3d'] for m in img_metas], [m['gt_labels_3d'] for m in img_metas])
        self.ctx = DecoderContext(img_metas, self.B, self.device)          # host -> device: outside the graph
        self.noise = head.draw_noise(self.slab.G, self.device)            # static: replay() writes the next draw into these

    def _set_ground_truth(self, boxes, labels):
        if len(boxes) != self.B or len(labels) != self.B:
            raise ValueError('CapturedHeadTrainStep: ground truth of %d samples for a batch of %d' % (len(boxes), self.B))
        self.slab.update(boxes, labels)                                    # ValueError above the capacity, before anything is enqueued
        self._boxes, self._labels = list(boxes), list(labels)
        self._metas = [{'gt_bboxes_3d': b, 'gt_labels_3d': l} for b, l in zip(boxes, labels)]

    def _run(self):
        head = self.head
        saved = (head.dn_noise, head.decoder_ctx)
        head.dn_noise, head.decoder_ctx = self.noise, self.ctx
        try:
            outs = head(self.mlvl_feats, self._metas)
            losses = head.loss(self._boxes, self._labels, outs)
            sum(losses.values()).backward()
        finally:
            head.dn_noise, head.decoder_ctx = saved
        return {k: v.detach() for k, v in losses.items()}

    def replay(self, gt_bboxes_list, gt_labels_list, img_metas=None, new_masks=True, noise=None):
        """Run the captured step on the next batch: the slab and (with ``img_metas``) the camera block are refreshed in place, new dn
        noise is drawn into the static noise tensors (or ``noise`` = (u_box, u_lab, new_lab) at capacity is copied in; ``noise=False``
        keeps the last one), with dropout on a new word unless ``new_masks=False``, then the graph runs.  Returns the graph's own loss
        dict -- clone what has to survive the next replay.  ``ValueError`` before anything is enqueued when a sample is above the
        capacity."""
        self._check_feature_grad_mode()
        self._refresh_head(gt_bboxes_list, gt_labels_list, img_metas, new_masks, noise)
        self._replay_graph()
        return self.losses

    def _refresh_head(self, gt_bboxes_list, gt_labels_list, img_metas, new_masks, noise):
        """the slab, the camera block, the dn noise and the dropout word of the next step: in place, outside the graph"""
        self._set_ground_truth(gt_bboxes_list, gt_labels_list)
        if img_metas is not None:
            self._refresh_cameras(img_metas)
        if noise is None:
            noise = self.head.draw_noise(self.slab.G, self.device)
        if noise is not False:
            for dst, src in zip(self.noise, noise):
                dst.copy_(src.to(self.device))
        if self.seed_dev is not None and new_masks:
            self.seed_dev.random_()


class CapturedDetectorTrainStep(CapturedHeadTrainStep):
    """``step = CapturedDetectorTrainStep(detector, img, img_metas)`` captures the WHOLE detector's training step --
    ``losses = detector.forward_train(img, img_metas, gt_bboxes, gt_labels)``, ``sum(losses.values()).backward()`` and, with ``optimizer=``,
    the AdamW update -- as one graph: image front end, backbone forward, neck forward, the head's step (``CapturedHeadTrainStep``), neck
    backward, backbone backward.  ``detector``: a ``detector.SparseBEV`` whose head is a ``SparseBEVTrainHead(gt_capacity=...)`` in
    ``train()`` with denoising on; ``img``: the STATIC uint8 or fp32 [B, N, 3, H, W] device tensor; the ground truth is
    ``img_metas[i]['gt_bboxes_3d'] / ['gt_labels_3d']``.

    The backbone's and the neck's weight images are derived INSIDE the graph (``dense.step_images``: one ``sbev_resnet_repack`` launch
    and the neck's two pack calls), so a replay after an optimizer update folds the weights as they are then.  The repack launch reads
    the parameters through a device table of their addresses, uploaded during the warm-up; ``replay`` checks that no tensor has moved
    since and raises otherwise -- and, since every other launch holds its parameters' addresses as kernel arguments, the same for every
    parameter and buffer of the detector.

    ``replay(gt_bboxes, gt_labels, img=None, img_metas=None, front_params=None, noise=None, new_masks=True)`` refreshes, outside the
    graph: the static image tensor (``img``: the next images, copied in), the front end's table (``front_params``, or a fresh
    ``front.draw``), the slab, the cameras, the dn noise and the dropout word -- then replays.  ``step.grads`` maps the detector's prefixed
    parameter names to the static gradient tensors.  ``optimizer``: a FusedAdamW over exactly the detector's trainable parameters (the
    reference's recipe: ``FusedAdamW(detector.param_groups(...))``); its three launches end the graph.  More than one rank is refused."""

    def __init__(self, detector, img, img_metas, warmup=3, optimizer=None):
        from .detector import SparseBEV
        from .head_train import SparseBEVTrainHead
        from .image_front import update_metas
        who = 'CapturedDetectorTrainStep'
        self._refuse_ranks(optimizer, always='the all-reduce of the averaging factors cannot be captured (run the eager step)')
        if not torch.is_grad_enabled():
            raise RuntimeError('%s: grad is disabled' % who)
        VERSION.require_supported()
        if not isinstance(detector, SparseBEV):
            raise TypeError('%s: the detector must be a sparsebev_amd.detector.SparseBEV' % who)
        head = detector.pts_bbox_head
        if not isinstance(head, SparseBEVTrainHead) or head.gt_capacity is None:
            raise ValueError('%s: the head must be a SparseBEVTrainHead(gt_capacity=...): at a dynamic shape nothing can be replayed' % who)
        if not (detector.training and head.training and head.dn_enabled):
            raise ValueError('%s: the detector must be in train() mode with query denoising on' % who)
        if not (torch.is_tensor(img) and img.is_cuda and img.dim() == 5 and img.shape[0] == len(img_metas) and img.shape[2] == 3
                and img.dtype in (torch.uint8, torch.float32) and img.is_contiguous()):
            raise ValueError('%s: img must be a contiguous uint8 or fp32 [B, N, 3, H, W] CUDA tensor with one img_metas entry per sample '
                             '(it is read in place)' % who)
        self.detector, self.head, self.img = detector, head, img
        self.front = detector.front
        self._update_metas = lambda metas: update_metas(metas, img.shape[0], img.shape[1], img.shape[3], img.shape[4], self.front.size_divisor)
        metas = [dict(m) for m in img_metas]
        Hp, _ = self._update_metas(metas)                              # the padded image size: the camera block's
        self._Hp = Hp
        self._bind_head(head, img.shape[0], img.device, metas)
        self.front.upload(self.front.draw(img.shape[0] * img.shape[1], Hp), self.device)
        named = [(n, p) for n, p in detector.named_parameters() if p.requires_grad]
        self._bind_optimizer(optimizer, [p for _, p in named])
        self._leaves = [p for _, p in named]
        self.losses = self._capture(warmup)
        self._repack_key = detector.img_backbone.repack_key()         # the addresses the graph's repack launch reads through
        self._repack_table = detector.img_backbone.repack_table(self._repack_key)      # alive as long as the graph that reads it
        # every launch of the graph holds its parameters' and buffers' addresses as kernel arguments: none may move before a replay
        self._addresses = [(n, t.data_ptr()) for n, t in list(detector.named_parameters()) + list(detector.named_buffers())]
        self.grads = {n: p.grad for n, p in named if p.grad is not None}
        self.input_grads = {}

    def _run(self):
        head = self.head
        saved = (head.dn_noise, head.decoder_ctx)
        head.dn_noise, head.decoder_ctx = self.noise, self.ctx
        try:
            losses = self.detector.forward_train(self.img, [dict(m) for m in self._metas], self._boxes, self._labels)
            sum(losses.values()).backward()
        finally:
            head.dn_noise, head.decoder_ctx = saved
        return {k: v.detach() for k, v in losses.items()}

    def replay(self, gt_bboxes_list, gt_labels_list, img=None, img_metas=None, front_params=None, noise=None, new_masks=True):
        """Run the captured step on the next batch (class text).  Returns the graph's own loss dict -- clone what has to survive the next
        replay.  Raises before anything is enqueued: ``ValueError`` for a sample above the capacity or an ``img`` of another shape or
        dtype, ``RuntimeError`` when a backbone tensor has moved since the capture."""
        who = type(self).__name__
        self._check_feature_grad_mode()
        self.detector.img_backbone.check_repack_table(self._repack_key)
        now = dict(list(self.detector.named_parameters()) + list(self.detector.named_buffers()))
        moved = [n for n, ptr in self._addresses if n not in now or now[n].data_ptr() != ptr]
        if moved:
            raise RuntimeError('%s.replay: %d parameter / buffer tensor(s) have another address than at capture (%s%s); the graph would read '
                               'the old one: capture a new step' % (who, len(moved), ', '.join(moved[:3]), ', ...' if len(moved) > 3 else ''))
        if img is not None:
            if not torch.is_tensor(img) or tuple(img.shape) != tuple(self.img.shape) or img.dtype != self.img.dtype:
                raise ValueError('%s.replay: img must be a %s tensor of shape %s, the captured step\'s' % (who, self.img.dtype, tuple(self.img.shape)))
        n = self.img.shape[0] * self.img.shape[1]
        if front_params is not None and len(front_params) != n:
            raise ValueError('%s.replay: front_params for %d images, %d given' % (who, n, len(front_params)))
        if img_metas is not None:
            img_metas = [dict(m) for m in img_metas]
            self._update_metas(img_metas)
        self._refresh_head(gt_bboxes_list, gt_labels_list, img_metas, new_masks, noise)
        if img is not None:
            self.img.copy_(img, non_blocking=True)
        self.front.upload(self.front.draw(n, self._Hp) if front_params is None else front_params, self.device)
        self._replay_graph()
        return self.losses
