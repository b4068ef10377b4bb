"""Dev tool: time the WHOLE detector's training step -- ImageFrontEnd -> ResNetBackbone(trainable, frozen_stages=1) -> FPNNeck(trainable) ->
SparseBEVTrainHead -> FusedAdamW with the reference's recipe -- three ways, interleaved in one process, and write one JSON line to
profiles/detector_step.json:

  (a) eager            ``detector.forward_train``, ``backward()``, ``FusedAdamW.step()``
  (b) head captured    what the tree could do before the backbone and the neck were capturable: front end / backbone / neck eager
                       around a ``CapturedHeadTrainStep`` whose feature tensors require grad, then the neck's and the backbone's backward
                       from the replay's feature gradients, then the optimizer
  (c) all captured     ``CapturedDetectorTrainStep`` with the optimizer inside: one graph replay

Shape: B = 1, 48 uint8 images of 3 x 256 x 704 (8 frames of 6 views), 40 boxes, capacity 40, 900 queries, 6 decoder layers.  Beside the
steps it times the ONE ``sbev_resnet_repack`` launch against the launches it replaces inside a step (``sbev_resnet_pack_weights`` +
``sbev_resnet_pack_weights_bwd`` on the same ResNet-50 tensors), with HIP events in the same run, and states the bytes both move.

    python tools/bench_detector_train.py [--steps 20] [--warmup 5] [--out profiles/detector_step.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch                                  # noqa: E402

DEV = 'cuda:0'
B, T, H, W, GTS, Q, LAYERS = 1, 8, 256, 704, 40, 900, 6
RECIPE = {'img_backbone': dict(lr_mult=0.1), 'sampling_offset': dict(lr_mult=0.1)}
COPY_RATE_TB_S = 6.29          # MI355X, measured float4 copy


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def make_detector():
    from sparsebev_amd import synthetic as S
    from sparsebev_amd.detector import SparseBEV
    head = dict(num_classes=10, in_channels=256, num_query=Q, code_size=10, code_weights=[2.0, 2.0] + [1.0] * 8,
                transformer=dict(type='SparseBEVTransformer', embed_dims=256, num_frames=T, num_points=4, num_layers=LAYERS, num_levels=4,
                                 num_classes=10, code_size=10, pc_range=S.PC_RANGE),
                bbox_coder=dict(type='NMSFreeCoder', post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_num=300, num_classes=10,
                                pc_range=S.PC_RANGE), assign_on='device', gt_capacity=GTS)
    det = SparseBEV(dict(depth=50, trainable=True, frozen_stages=1), dict(in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=4, trainable=True),
                    head, data_aug=dict(img_color_aug=True, img_norm_cfg=dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True),
                                        img_pad_cfg=dict(size_divisor=32)))
    det.pts_bbox_head.init_weights()
    S.randomize_zero_init(det.pts_bbox_head.transformer, std=0.02, seed=0)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        det.pts_bbox_head.init_query_bbox.weight[:, 2] = 0.5
        for _, bn in det.img_backbone.conv_bn_pairs():
            bn.running_var.copy_(0.5 + torch.rand(bn.running_var.shape, generator=g))
            bn.running_mean.copy_(0.1 * torch.randn(bn.running_mean.shape, generator=g))
        for s in range(4):
            for block in getattr(det.img_backbone, 'layer%d' % (s + 1)):
                block.bn3.weight.mul_(0.3)
    return det


def make_optimizer(det):
    from sparsebev_amd.optim import FusedAdamW
    return FusedAdamW(det.param_groups(2e-4, 0.01, RECIPE), max_grad_norm=35.0)


def bench_steps(steps, warmup):
    import bench_head_train as BH
    from sparsebev_amd import synthetic as S
    from sparsebev_amd.train_graph import CapturedDetectorTrainStep, CapturedHeadTrainStep
    base = make_detector()
    img = torch.randint(0, 256, (B, T * 6, 3, H, W), dtype=torch.uint8, device=DEV)
    boxes, labels = (list(t) for t in BH.make_gt(B, GTS, 1, 'cpu'))
    metas = S.make_img_metas(B, T, H, W)
    for m, bx, lb in zip(metas, boxes, labels):
        m['gt_bboxes_3d'], m['gt_labels_3d'] = bx, lb

    # (a) eager
    det_a = copy.deepcopy(base).to(DEV).train()
    opt_a = make_optimizer(det_a)
    params_a = [p for p in det_a.parameters() if p.requires_grad]

    def eager():
        for p in params_a:
            p.grad = None
        losses = det_a.forward_train(img, copy.deepcopy(metas), boxes, labels)
        sum(losses.values()).backward()
        opt_a.step()

    # (b) the head's step captured, everything around it eager
    det_b = copy.deepcopy(base).to(DEV).train()
    opt_b = make_optimizer(det_b)
    # the head's .grad tensors belong to the captured head step (static); only the backbone's and the neck's are autograd's to refill
    params_b = [p for n, p in det_b.named_parameters() if p.requires_grad and not n.startswith('pts_bbox_head.')]
    m0 = copy.deepcopy(metas)
    with torch.no_grad():
        shapes = [tuple(f.shape) for f in det_b.extract_feat(img, m0)]
    static = [torch.empty((s[0] * s[1], s[3], s[4], s[2]), device=DEV).permute(0, 3, 1, 2).view(s).detach().requires_grad_() for s in shapes]
    head_step = CapturedHeadTrainStep(det_b.pts_bbox_head, static, m0)

    def head_captured():
        for p in params_b:
            p.grad = None
        m = copy.deepcopy(metas)
        x = det_b.front(img, m)
        outs = det_b.img_neck(det_b.img_backbone(x), out_dtype=torch.float32)
        with torch.no_grad():
            for dst, o in zip(static, outs):
                dst.view(o.shape).copy_(o)
        head_step.replay(boxes, labels, m)
        torch.autograd.backward(outs, [f.grad.reshape(o.shape) for f, o in zip(static, outs)])
        opt_b.step()

    # (c) the whole step captured, the optimizer inside
    det_c = copy.deepcopy(base).to(DEV).train()
    opt_c = make_optimizer(det_c)
    whole = CapturedDetectorTrainStep(det_c, img, metas, optimizer=opt_c)

    def all_captured():
        whole.replay(boxes, labels, img_metas=metas)

    legs = (('a_eager', eager), ('b_head_captured', head_captured), ('c_all_captured', all_captured))
    times = {k: [] for k, _ in legs}
    for i in range(warmup + steps):
        for name, fn in legs:
            t = timed(fn)
            if i >= warmup:
                times[name].append(t)
    assert whole.captures == 1 and all(bool(torch.isfinite(v)) for v in whole.losses.values())
    med = {k: statistics.median(v) for k, v in times.items()}
    return dict(median_ms={k: round(v, 4) for k, v in med.items()}, min_ms={k: round(min(v), 4) for k, v in times.items()},
                max_ms={k: round(max(v), 4) for k, v in times.items()},
                c_over_b=round(med['c_all_captured'] / med['b_head_captured'], 4), c_over_a=round(med['c_all_captured'] / med['a_eager'], 4),
                trainable_parameters=sum(p.numel() for p in params_a))


def bench_repack(iters):
    """the one launch beside the launches it replaces in a step, on ResNet-50's tensors (fp32 weights, frozen_stages=1)"""
    from sparsebev_amd import resnet as R
    net = R.ResNetBackbone(depth=50, trainable=True, frozen_stages=1).to(DEV)
    layers = [(c.weight, b.weight, b.bias, b.running_mean, b.running_var) for c, b in net.conv_bn_pairs()]
    bp = net.backward_plan(1, 32, 32)
    order = sorted((l['pack_offset'], i) for i, l in enumerate(bp['layers']) if l['pack_offset'] >= 0)
    todo = [(layers[i - 1][0], layers[i - 1][1], layers[i - 1][4]) for _, i in order]
    p = R.repack_plan(50, [tuple(t.data_ptr() for t in l) for l in layers], torch.float32, first_trainable_stage=2)
    table = torch.tensor(p['table'], dtype=torch.int64).to(DEV)
    fwd, bwd = torch.empty(p['pack_bytes'], dtype=torch.uint8, device=DEV), torch.empty(p['pack_bwd_bytes'], dtype=torch.uint8, device=DEV)
    ref_fwd, ref_bwd = R.pack_layers(layers, net.eps)[0], R.pack_layers_bwd(todo, net.eps)[0]

    def old():
        R.pack_layers(layers, net.eps, ref_fwd)
        R.pack_layers_bwd(todo, net.eps, ref_bwd)

    def new():
        R.repack(table, fwd, bwd, net.eps)

    for _ in range(3):
        old()
        new()
    torch.cuda.synchronize()
    same = torch.equal(fwd, ref_fwd[:fwd.numel()]) and torch.equal(bwd, ref_bwd[:bwd.numel()])
    times = {'existing_pack_launches': [], 'one_repack_launch': []}
    for _ in range(iters):
        times['existing_pack_launches'].append(timed(old))
        times['one_repack_launch'].append(timed(new))
    weight_bytes = sum(l[0].numel() * 4 for l in layers)
    bwd_weight_bytes = sum(l[0].numel() * 4 for l in todo)
    moved_new = weight_bytes + p['pack_bytes'] + p['pack_bwd_bytes']
    moved_old = weight_bytes + bwd_weight_bytes + p['pack_bytes'] + p['pack_bwd_bytes']
    med = {k: statistics.median(v) for k, v in times.items()}
    return dict(launches_replaced=len(layers) + len(todo), bit_identical=same, median_us={k: round(v * 1e3, 2) for k, v in med.items()},
                min_us={k: round(min(v) * 1e3, 2) for k, v in times.items()}, weight_bytes=weight_bytes, forward_image_bytes=p['pack_bytes'],
                backward_image_bytes=p['pack_bwd_bytes'], bytes_moved={'one_repack_launch': moved_new, 'existing_pack_launches': moved_old},
                copy_rate_tb_s=COPY_RATE_TB_S, time_at_copy_rate_us=round(moved_new / (COPY_RATE_TB_S * 1e12) * 1e6, 2),
                share_of_copy_rate=round(moved_new / (COPY_RATE_TB_S * 1e12) / (med['one_repack_launch'] * 1e-3), 4),
                timing='HIP events around the host call(s): the existing entries include their launch overhead, which is what a step pays')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'detector_step.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_detector_train needs a GPU: nothing is measured without one')
    rec = {'tool': 'bench_detector_train', 'device': torch.cuda.get_device_name(0), 'hip': torch.version.hip, 'torch': torch.__version__,
           'shape': dict(B=B, frames=T, images=B * T * 6, image=[3, H, W], boxes=GTS, gt_capacity=GTS, queries=Q, decoder_layers=LAYERS, depth=50,
                         frozen_stages=1), 'recipe': 'FusedAdamW(lr 2e-4, weight_decay 0.01, img_backbone and sampling_offset lr_mult 0.1, clip 35)',
           'steps': a.steps, 'warmup': a.warmup, 'timing': 'HIP events around each step, the three legs interleaved in one run'}
    with torch.enable_grad():
        rec['repack'] = bench_repack(max(a.steps, 20))
        print(json.dumps({'repack': rec['repack']}), file=sys.stderr, flush=True)          # kept if the step legs fail
        rec['step'] = bench_steps(a.steps, a.warmup)
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
