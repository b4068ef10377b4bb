"""The whole detector's training step: the backbone and the neck inside a ``dense.step_images()`` scope under a graph capture,
``detector.SparseBEV`` and ``train_graph.CapturedDetectorTrainStep``.  Every comparison is of bits: a replay runs the launches of the
eager step on identical inputs (``ops.deterministic_feature_grad`` makes the sampler's feature gradient reproducible)."""
import copy

import numpy as np
import pytest
import torch

import head_train_cases as C
import test_gpu_head_train as T
from sparsebev_amd import dense, ops, optim, synthetic as S
from sparsebev_amd import head_train as HT
from sparsebev_amd.detector import SparseBEV
from sparsebev_amd.fpn import FPNNeck
from sparsebev_amd.image_front import FrontParams
from sparsebev_amd.resnet import ResNetBackbone

pytestmark = pytest.mark.gpu
DEV = T.DEV
F32 = torch.float32
B, TF, H, W, HP, WP = 1, 2, 64, 176, 64, 192          # 12 images of 3 x 64 x 176, padded to 64 x 192
N_IMG = B * TF * 6
CAP, GROUPS, Q = 5, 2, 49
DATA_AUG = dict(img_color_aug=True, img_norm_cfg=dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True),
                img_pad_cfg=dict(size_divisor=32))


@pytest.fixture(autouse=True)
def deterministic_feature_gradient():
    prev = ops.deterministic_feature_grad(True)
    yield
    ops.deterministic_feature_grad(prev)


def make_backbone(seed=3):
    torch.manual_seed(seed)
    net = ResNetBackbone(depth=50, stage_blocks=(1, 1, 1, 1), trainable=True, frozen_stages=1)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for _, bn in net.conv_bn_pairs():
            bn.weight.copy_(torch.rand(bn.weight.shape, generator=g) * 0.5 + 0.75)
            bn.bias.copy_(torch.randn(bn.bias.shape, generator=g) * 0.1)
            bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=g) * 0.1)
            bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=g) + 0.5)
    return net


def make_neck(seed=5):
    torch.manual_seed(seed)
    return FPNNeck([256, 512, 1024, 2048], 256, 4, trainable=True)


def make_detector(dropout=False):
    head = HT.SparseBEVTrainHead(
        num_classes=10, in_channels=256, num_query=Q, code_size=10, code_weights=C.CODE_WEIGHTS,
        transformer=dict(type='SparseBEVTransformer', embed_dims=256, num_frames=TF, num_points=4, num_layers=2, num_levels=4, num_classes=10,
                         code_size=10, pc_range=S.PC_RANGE),
        bbox_coder=dict(type='NMSFreeCoder', post_center_range=T.POST, max_num=30, score_threshold=None, num_classes=10, pc_range=S.PC_RANGE),
        assign_on='device', gt_capacity=CAP)
    params = S.make_params(61, embed_dims=256, num_frames=TF, num_points=4, num_levels=4)
    head.transformer.load_state_dict({'decoder.decoder_layer.' + k: v for k, v in params.items()}, strict=True)
    with torch.no_grad():
        head.init_query_bbox.weight[:, 2] = 0.5
        head.init_query_bbox.weight[:, 5] = 0.5
    head.dn_group_num = GROUPS
    if not dropout:
        layer = head.transformer.decoder.decoder_layer
        layer.self_attn.attn_drop, layer.ffn_drop = 0.0, 0.0
    det = SparseBEV(make_backbone(), make_neck(), head, data_aug=DATA_AUG)
    return det.to(DEV).train()


def batch(seed, counts, per_sample_cameras=False):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, TF * 6, 3, H, W), generator=g, dtype=torch.uint8).to(DEV)
    boxes, labels = C.make_gt(counts, 10, seed + 1)
    metas = (S.make_img_metas_per_sample if per_sample_cameras else S.make_img_metas)(B, TF, HP, WP)
    for m, b, l in zip(metas, boxes, labels):
        m['gt_bboxes_3d'], m['gt_labels_3d'] = b, l
    return img, metas, boxes, labels


def noise_of(seed):
    return C.make_noise(GROUPS, B * CAP, 10, seed)


def plain():
    return FrontParams(N_IMG)          # no colour transform, no mask


def eager_step(det, img, metas, boxes, labels, noise, front_params, optimizer=None):
    det.zero_grad(set_to_none=True)
    det.pts_bbox_head.dn_noise = tuple(t.to(DEV) for t in noise)
    with torch.enable_grad():
        losses = det.forward_train(img, copy.deepcopy(metas), boxes, labels, front_params=front_params)
        sum(losses.values()).backward()
    grads = {n: p.grad.clone() for n, p in det.named_parameters() if p.grad is not None}
    if optimizer is not None:
        optimizer.step()
    return {k: v.detach().clone() for k, v in losses.items()}, grads


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert torch.equal(got[k], want[k]), '%s: %s differs' % (what, k)


RECIPE = {'img_backbone': dict(lr_mult=0.1), 'sampling_offset': dict(lr_mult=0.1)}


# ---- 1. backbone and neck under a capture inside step_images() ----------------------------------------------------------------------

def test_backbone_and_neck_capture_inside_step_images():
    net, neck = make_backbone().to(DEV), make_neck().to(DEV)
    twin_net, twin_neck = copy.deepcopy(net), copy.deepcopy(neck)
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(N_IMG, 3, HP, WP, generator=g)).to(DEV)
    shapes = [(N_IMG, 256, 16, 48), (N_IMG, 256, 8, 24), (N_IMG, 256, 4, 12), (N_IMG, 256, 2, 6)]
    weights = [torch.randn(s, generator=g).to(DEV) * 2.0 ** -6 for s in shapes]
    leaves = lambda a, b: [p for p in list(a.parameters()) + list(b.parameters()) if p.requires_grad]

    def run(a, b):
        outs = b(a(x), out_dtype=F32)
        assert [tuple(o.shape) for o in outs] == shapes
        sum((o * w).sum() for o, w in zip(outs, weights)).backward()
        return [o.detach() for o in outs]

    def clear(a, b):
        for p in leaves(a, b):
            p.grad = None

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.enable_grad():
        for _ in range(2):          # the warm-up builds the repack table (outside the capture) and every workspace
            clear(net, neck)
            with dense.step_images():
                run(net, neck)
        clear(net, neck)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            with dense.step_images():
                outs = run(net, neck)
    torch.cuda.current_stream().wait_stream(side)
    assert all(holder.key is None for holder in (net._image, net._image_bwd, neck._image, neck._image_bwd))      # caches untouched
    grads = {id(p): p.grad for p in leaves(net, neck)}
    assert all(g is not None for g in grads.values())

    def compare(what):
        graph.replay()
        torch.cuda.synchronize()
        clear(twin_net, twin_neck)
        with torch.enable_grad():
            want = run(twin_net, twin_neck)
        for k, (a, b) in enumerate(zip(outs, want)):
            assert torch.equal(a, b) and float(b.abs().max()) > 0, '%s: output %d' % (what, k)
        for (name, p), q in zip(list(net.named_parameters()) + list(neck.named_parameters()), list(twin_net.parameters()) + list(twin_neck.parameters())):
            if p.requires_grad:
                assert p.grad is grads[id(p)] and torch.equal(p.grad, q.grad) and bool(torch.isfinite(q.grad).all()), '%s: %s' % (what, name)
        return [o.clone() for o in outs]

    first = compare('replay')
    # an in-place change of one stage-3 weight and one neck weight: the replay folds and packs the NEW weights
    with torch.no_grad():
        for a, b in ((net, neck), (twin_net, twin_neck)):
            a.layer3[0].conv2.weight.mul_(1.5)
            b.lateral_convs[1].conv.weight.mul_(-0.5)
    second = compare('replay on changed weights')
    assert not torch.equal(first[1], second[1]) and not torch.equal(first[3], second[3])
    # outside a scope the same capture still raises the existing messages
    for mod, arg, text in ((net, x, 'ResNetBackbone: a trainable forward under a graph capture'),
                           (neck, [o.detach() for o in twin_net(x)], 'FPNNeck: a trainable forward under a graph capture')):
        torch.cuda.synchronize()
        refused = torch.cuda.CUDAGraph()
        with torch.enable_grad(), pytest.raises(RuntimeError, match=text):
            with torch.cuda.graph(refused):
                mod(arg)
    # and under a capture inside a scope a backbone that never saw a warm-up step says so
    cold = make_backbone(seed=11).to(DEV)
    torch.cuda.synchronize()
    refused = torch.cuda.CUDAGraph()
    with torch.enable_grad(), pytest.raises(RuntimeError, match='run a warm-up step first'):
        with torch.cuda.graph(refused):
            with dense.step_images():
                cold(x)


# ---- 2. SparseBEV.forward_train, eager -----------------------------------------------------------------------------------------------

def test_forward_train_equals_the_modules_by_hand():
    det = make_detector()
    img, metas, boxes, labels = batch(21, (4,))
    noise = noise_of(700)
    losses, grads = eager_step(det, img, metas, boxes, labels, noise, plain())
    assert len(losses) == 8 and all(bool(torch.isfinite(v)) for v in losses.values())
    trainable = sorted(n for n, p in det.named_parameters() if p.requires_grad)
    assert sorted(grads) == trainable
    assert any(n.startswith('img_backbone.layer2.') for n in grads) and not any(n.startswith('img_backbone.layer1.') for n in grads)
    assert any(n.startswith('img_neck.') for n in grads) and 'pts_bbox_head.init_query_bbox.weight' in grads
    # the same modules called by hand in sequence
    det.zero_grad(set_to_none=True)
    m2 = copy.deepcopy(metas)
    with torch.enable_grad():
        x = det.front(img, m2, params=plain())
        assert tuple(x.shape) == (N_IMG, 3, HP, WP) and m2[0]['pad_shape'][0] == (HP, WP, 3)
        outs = det.img_neck(det.img_backbone(x), out_dtype=F32)
        feats = [o.view(B, TF * 6, 256, o.shape[2], o.shape[3]) for o in outs]
        for m, b, l in zip(m2, boxes, labels):
            m['gt_bboxes_3d'], m['gt_labels_3d'] = b, l
        det.pts_bbox_head.dn_noise = tuple(t.to(DEV) for t in noise)
        by_hand = det.pts_bbox_head.loss(boxes, labels, det.pts_bbox_head(feats, m2))
        sum(by_hand.values()).backward()
    assert_same(losses, {k: v.detach() for k, v in by_hand.items()}, 'loss')
    assert_same(grads, {n: p.grad for n, p in det.named_parameters() if p.grad is not None}, 'gradient')
    assert [tuple(f.shape) for f in det.extract_feat(img, copy.deepcopy(metas), plain())] == \
        [(B, TF * 6, 256, 16, 48), (B, TF * 6, 256, 8, 24), (B, TF * 6, 256, 4, 12), (B, TF * 6, 256, 2, 6)]
    # the reference's key prefixes, strict
    state = {}
    for prefix, mod in (('img_backbone.', det.img_backbone), ('img_neck.', det.img_neck), ('pts_bbox_head.', det.pts_bbox_head)):
        state.update({prefix + k: v.detach().clone() + (0.25 if v.is_floating_point() else 0) for k, v in mod.state_dict().items()})
    assert sorted(state) == sorted(det.state_dict())
    det.load_state_dict(state, strict=True)
    assert torch.equal(det.img_backbone.layer3[0].conv2.weight, state['img_backbone.layer3.0.conv2.weight'])
    # the reference's optimizer recipe in one call
    groups = det.param_groups(2e-4, 0.01, RECIPE)
    by_lr = {g['lr']: g['names'] for g in groups}
    assert sorted(by_lr) == [2e-4 * 0.1, 2e-4] and sorted(n for g in groups for n in g['names']) == trainable
    assert all(n.startswith('img_backbone.') or 'sampling_offset' in n for n in by_lr[2e-4 * 0.1])
    assert any('sampling_offset' in n for n in by_lr[2e-4 * 0.1]) and not any(n.startswith('img_backbone.') for n in by_lr[2e-4])
    with pytest.raises(ValueError, match='stop_prev_grad=1 is not built'):
        SparseBEV(det.img_backbone, det.img_neck, det.pts_bbox_head, data_aug=DATA_AUG, stop_prev_grad=1)


# ---- 3. the captured step against an eager twin --------------------------------------------------------------------------------------

def test_captured_detector_step_vs_eager_twin(monkeypatch):
    from sparsebev_amd.train_graph import CapturedDetectorTrainStep
    det = make_detector()
    twin = copy.deepcopy(det)                     # made before the first step
    a, b = batch(31, (5,)), batch(131, (0,), per_sample_cameras=True)
    static = a[0].clone()
    with torch.enable_grad():
        step = CapturedDetectorTrainStep(det, static, a[1])
    assert step.captures == 1
    assert sorted(step.grads) == sorted(n for n, p in det.named_parameters() if p.requires_grad)
    ptrs = {n: g.data_ptr() for n, g in step.grads.items()}
    seen = []
    for k, (img, metas, boxes, labels) in enumerate((a, b, a)):
        noise = noise_of(500 + (k % 2))
        losses = step.replay(boxes, labels, img=img, img_metas=metas, front_params=plain(), noise=noise)
        torch.cuda.synchronize()
        got = ({n: v.clone() for n, v in losses.items()}, {n: g.clone() for n, g in step.grads.items()})
        want = eager_step(twin, img, metas, boxes, labels, noise, plain())
        assert len(got[0]) == 8 and det.pts_bbox_head.plan_status.tolist() == [0]
        assert_same(got[0], want[0], 'loss, replay %d' % k)
        assert_same(got[1], want[1], 'gradient, replay %d' % k)
        assert all(bool(torch.isfinite(g).all()) for g in got[1].values())
        seen.append(got)
    assert_same(seen[2][0], seen[0][0], 'third replay vs first')
    assert_same(seen[2][1], seen[0][1], 'third replay vs first')
    assert any(not torch.equal(seen[1][0][k], seen[0][0][k]) for k in seen[0][0])
    assert float(seen[0][1]['img_backbone.layer2.0.conv1.weight'].abs().max()) > 0
    assert step.captures == 1 and {n: g.data_ptr() for n, g in step.grads.items()} == ptrs
    assert all(p.grad is step.grads[n] for n, p in det.named_parameters() if p.requires_grad)
    # refusals: an img of another shape; a moved backbone parameter; two ranks
    with pytest.raises(ValueError, match='img must be a torch.uint8 tensor of shape'):
        step.replay(a[2], a[3], img=a[0][:, :6])
    w = det.img_backbone.layer4[0].conv3.weight
    old = w.data
    w.data = w.data.clone()
    try:
        with pytest.raises(RuntimeError, match='another address'):
            step.replay(a[2], a[3])
    finally:
        w.data = old
    nw = det.img_neck.fpn_convs[2].conv.weight          # the neck's and the head's launches hold addresses as kernel arguments
    old = nw.data
    nw.data = nw.data.clone()
    try:
        with pytest.raises(RuntimeError, match='img_neck.fpn_convs.2.conv.weight'):
            step.replay(a[2], a[3])
    finally:
        nw.data = old
    step.replay(a[2], a[3], noise=False, front_params=plain())          # back at its address: accepted again
    torch.cuda.synchronize()
    import torch.distributed as dist
    with monkeypatch.context() as mp:
        mp.setattr(dist, 'is_initialized', lambda: True)
        mp.setattr(dist, 'get_world_size', lambda *a, **k: 2)
        with torch.enable_grad(), pytest.raises(RuntimeError, match='CapturedDetectorTrainStep: a process group of 2 ranks'):
            CapturedDetectorTrainStep(twin, static, a[1])


# ---- 4. with the optimizer inside the graph -----------------------------------------------------------------------------------------------

def test_captured_detector_step_with_the_recipes_optimizer():
    from sparsebev_amd.train_graph import CapturedDetectorTrainStep
    det = make_detector()
    twin = copy.deepcopy(det)
    a, b = batch(41, (3,)), batch(141, (5,))
    opt = optim.FusedAdamW(det.param_groups(2e-4, 0.01, RECIPE), max_grad_norm=35.0)
    twin_opt = optim.FusedAdamW(twin.param_groups(2e-4, 0.01, RECIPE), max_grad_norm=35.0)
    before = {n: p.detach().clone() for n, p in det.named_parameters()}
    with torch.enable_grad():
        step = CapturedDetectorTrainStep(det, a[0].clone(), a[1], optimizer=opt)
    assert_same({n: p.detach() for n, p in det.named_parameters()}, before, 'construction leaves the parameters alone')
    for k, (img, metas, boxes, labels) in enumerate((a, b)):
        noise = noise_of(600 + k)
        step.replay(boxes, labels, img=img, img_metas=metas, front_params=plain(), noise=noise)
        eager_step(twin, img, metas, boxes, labels, noise, plain(), optimizer=twin_opt)
    torch.cuda.synchronize()
    assert_same({n: p.detach() for n, p in det.named_parameters()}, {n: p.detach() for n, p in twin.named_parameters()}, 'parameters after two steps')
    moved = [n for n, p in det.named_parameters() if p.requires_grad and not torch.equal(p.detach(), before[n])]
    assert any(n.startswith('img_backbone.') for n in moved) and any(n.startswith('img_neck.') for n in moved)
    # the eager pack caches follow the graph's raw-pointer update (the _version bump after the replay)
    with torch.no_grad():
        got = det.extract_feat(a[0], copy.deepcopy(a[1]), plain())
        want = twin.extract_feat(a[0], copy.deepcopy(a[1]), plain())
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    # an optimizer that misses the backbone is refused by name
    with torch.enable_grad(), pytest.raises(ValueError, match='exactly the captured trainable parameters'):
        CapturedDetectorTrainStep(twin, a[0].clone(), a[1], optimizer=optim.FusedAdamW(twin.pts_bbox_head.parameters(), lr=1e-4))


# ---- 5. colour augmentation, GridMask and dropout inside the graph --------------------------------------------------------------------------

def test_captured_detector_step_front_params_and_dropout():
    from sparsebev_amd.train_graph import CapturedDetectorTrainStep
    det = make_detector(dropout=True)
    img, metas, boxes, labels = batch(51, (4,))
    with torch.enable_grad():
        step = CapturedDetectorTrainStep(det, img.clone(), metas, warmup=1)
    assert step.dropout and step.seed_dev is not None
    p1 = det.front.draw(N_IMG, HP, training=True, rng=np.random.RandomState(7))
    p2 = det.front.draw(N_IMG, HP, training=True, rng=np.random.RandomState(8))
    p1.mask[:], p2.mask[:] = (1, 16, 8, 3, 5), (1, 12, 6, 1, 2)          # GridMask applied in both, differently
    assert p1.flags.any() and p2.flags.any()
    runs = []
    for params, new_masks in ((p1, False), (p1, False), (p2, False), (p2, True)):
        losses = step.replay(boxes, labels, front_params=params, noise=False, new_masks=new_masks)
        torch.cuda.synchronize()
        runs.append(({k: v.clone() for k, v in losses.items()}, {n: g.clone() for n, g in step.grads.items()}))
    assert_same(runs[1][0], runs[0][0], 'loss, same front_params')
    assert_same(runs[1][1], runs[0][1], 'gradient, same front_params')
    assert any(not torch.equal(runs[2][0][k], runs[0][0][k]) for k in runs[0][0])          # other colours, another mask
    assert any(not torch.equal(runs[3][0][k], runs[2][0][k]) for k in runs[2][0])          # another dropout word
