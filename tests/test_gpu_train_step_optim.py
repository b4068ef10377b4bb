"""The captured train steps and an optimizer: replays after the weights moved (every derived weight image is derived inside the graph),
and FusedAdamW as the tail of the captured step (``optimizer=``).  Shapes: those of test_gpu_backward.py's captured test and of
test_gpu_head_capacity.py's."""
import copy
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT

gpu = pytest.mark.gpu


def _decoder_setup(seed, layers=3):
    import test_gpu_backward as TB
    from sparsebev_amd import synthetic as S
    B, Q, T = 1, 100, 2
    ih, iw, sizes = S.PYRAMIDS['tiny']
    model = TB.build(T, len(sizes), seed, layers).train()
    model.decoder.decoder_layer.self_attn.attn_drop = 0.0
    model.decoder.decoder_layer.ffn_drop = 0.0
    cot = [torch.randn(layers, B, Q, 10, generator=torch.Generator().manual_seed(5 + i)).to(TB.DEV) for i in range(2)]
    feats = [f.to(TB.DEV) for f in S.make_features(B, T, sizes, seed=1)]
    bbox, feat = [t.to(TB.DEV) for t in S.make_queries(B, Q, seed=2)]
    metas = S.make_img_metas(B, T, ih, iw)
    return model, cot, feats, bbox, feat, metas


def _eager_step(model, loss_fn, bbox, feat, feats, metas):
    for p in model.parameters():
        p.grad = None
    q = feat.clone().requires_grad_(True)
    cls, box = model(bbox, q, list(feats), None, copy.deepcopy(metas))
    loss = loss_fn(cls, box)
    loss.backward()
    return loss.detach(), cls.detach(), box.detach(), q.grad


@gpu
@torch.enable_grad()
def test_replay_after_a_plain_optimizer_step_sees_the_new_weights():
    """CapturedTrainStep WITHOUT optimizer=: replay, an in-place torch.optim.SGD step, replay again -- loss, outputs and every gradient
    of the second replay equal an eager step of a twin model that holds the updated weights (1e-6 / 1e-5 relative, the tolerances of
    test_gpu_backward.py's captured-against-eager test).  Before the derived weight images (W^T, the fp16 fragment images of the two
    mixing weights) were made inside the graph, the capture ran on warm caches and its GEMMs went on reading the images of the weights
    as they were at capture."""
    import test_gpu_backward as TB
    from sparsebev_amd.train_graph import CapturedTrainStep
    model, cot, feats, bbox, feat, metas = _decoder_setup(77)
    loss_fn = lambda cls, box: (cls * cot[0]).sum() + (box * cot[1]).sum()
    sq = feat.clone().requires_grad_(True)
    step = CapturedTrainStep(model, bbox, sq, feats, metas, loss_fn)
    first = [t.clone() for t in step.replay()]
    # the step size from the gradients: the element that moves most moves by 0.01 (the weights are of the order of 0.02 .. 1)
    lr = 0.01 / max(g.abs().max().item() for g in step.grads.values())
    sgd = torch.optim.SGD([p for p in model.decoder.parameters() if p.requires_grad], lr=lr)
    before = {n: p.detach().clone() for n, p in model.decoder.named_parameters()}
    sgd.step()
    moved = max(TB.rel(p, before[n]) for n, p in model.decoder.named_parameters())
    assert moved > 1e-3                                   # the weights really moved
    twin = copy.deepcopy(model)
    loss, cls, box = [t.clone() for t in step.replay()]
    grads = {n: g.clone() for n, g in step.grads.items()}
    gq = step.input_grads['query_feat'].clone()
    del step
    eloss, ecls, ebox, egq = _eager_step(twin, loss_fn, bbox, feat, feats, metas)
    print('second replay vs eager on the updated weights: loss %.2e cls %.2e box %.2e; first vs second replay loss %.2e'
          % (TB.rel(loss, eloss), TB.rel(cls, ecls), TB.rel(box, ebox), TB.rel(first[0], loss)))
    assert TB.rel(first[0], loss) > 1e-5                  # and the loss with them
    assert TB.rel(cls, ecls) < 1e-6 and TB.rel(box, ebox) < 1e-6 and TB.rel(loss, eloss) < 1e-6
    assert TB.rel(gq, egq) < 1e-5
    for n, p in twin.decoder.named_parameters():
        assert TB.rel(grads[n], p.grad) < 1e-5, n


@gpu
@torch.enable_grad()
def test_captured_train_step_with_the_optimizer_inside():
    """CapturedTrainStep(..., optimizer=FusedAdamW): construction (warm-up on the hold path, capture) leaves parameters, moments and
    counters bit-unchanged; three replays give the parameters of three times (eager step, opt.step()) on a twin to 1e-5 relative (the
    existing captured test's gradient tolerance), with the reference's recipe: lr 2e-4, weight decay 0.01, clip 35, loss scale 512."""
    import test_gpu_backward as TB
    from sparsebev_amd import optim
    from sparsebev_amd.train_graph import CapturedTrainStep
    model, cot, feats, bbox, feat, metas = _decoder_setup(78)
    twin = copy.deepcopy(model)
    loss_fn = lambda cls, box: 512.0 * ((cls * cot[0]).sum() + (box * cot[1]).sum())
    recipe = dict(lr=2e-4, weight_decay=0.01, max_grad_norm=35.0, loss_scale=512.0)
    keys = {'sampling_offset': dict(lr_mult=0.1)}
    opt = optim.FusedAdamW(optim.param_groups(model.decoder.named_parameters(), 2e-4, 0.01, keys), **recipe)
    topt = optim.FusedAdamW(optim.param_groups(twin.decoder.named_parameters(), 2e-4, 0.01, keys), **recipe)
    assert len(opt.param_groups) == 2
    params = dict(model.decoder.named_parameters())
    snap = lambda: ({n: p.detach().clone() for n, p in params.items()}, {n: opt.state[p]['exp_avg'].clone() for n, p in params.items()},
                    {n: opt.state[p]['exp_avg_sq'].clone() for n, p in params.items()})
    before = snap()
    sq = feat.clone().requires_grad_(True)
    step = CapturedTrainStep(model, bbox, sq, feats, metas, loss_fn, optimizer=opt)
    torch.cuda.synchronize()
    after = snap()
    for a, b in zip(before, after):
        assert all(torch.equal(a[n], b[n]) for n in a)
    assert int(opt.step_count.item()) == 0 and int(opt.skipped.item()) == 0 and not opt.hold
    versions = {n: p._version for n, p in params.items()}
    for k in range(3):
        loss = step.replay()[0].clone()
        g_used = {n: g.clone() for n, g in step.grads.items()}
        eloss = _eager_step(twin, loss_fn, bbox, feat, feats, metas)[0]
        assert TB.rel(loss, eloss) < 1e-6, k
        for n, p in twin.decoder.named_parameters():       # step.grads after a replay: the gradients the update consumed
            assert TB.rel(g_used[n], p.grad) < 1e-5, (k, n)
        topt.step()
        worst = max(TB.rel(params[n], p) for n, p in twin.decoder.named_parameters())
        print('replay %d: worst relative parameter difference captured vs eager %.2e' % (k, worst))
        for n, p in twin.decoder.named_parameters():
            assert TB.rel(params[n], p) < 1e-5, (k, n)
    assert int(opt.step_count.item()) == 3 and int(opt.skipped.item()) == 0 and int(topt.step_count.item()) == 3
    assert all(params[n]._version == versions[n] + 3 for n in params)
    assert max(TB.rel(params[n], before[0][n]) for n in params) > 1e-4          # they moved
    # an lr written into the group between replays reaches the graph
    for g in opt.param_groups + topt.param_groups:
        g['lr'] = 0.0
        g['weight_decay'] = 0.0
    frozen = {n: p.detach().clone() for n, p in params.items()}
    step.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(frozen[n], params[n]) for n in params) and int(opt.step_count.item()) == 4
    with pytest.raises(ValueError, match='exactly the captured'):
        CapturedTrainStep(twin, bbox, sq, feats, metas, loss_fn, optimizer=opt)
    with pytest.raises(TypeError, match='FusedAdamW'):
        CapturedTrainStep(twin, bbox, sq, feats, metas, loss_fn, optimizer=torch.optim.SGD(twin.parameters(), lr=0.1))


@gpu
def test_captured_head_step_with_the_optimizer_inside():
    """CapturedHeadTrainStep(head, feats, metas, optimizer=opt) at test_gpu_head_capacity.py's shape: three batches with different
    ground-truth counts, one capture; after each replay the parameters equal the twin's after (eager step, opt.step()) BIT FOR BIT
    (the existing captured head test asserts bit-equal gradients); the embeddings move; a batch above the capacity raises before
    anything is enqueued and leaves the parameters untouched."""
    import head_train_cases as C
    import test_gpu_head_capacity as HC
    from sparsebev_amd import optim
    from sparsebev_amd.train_graph import CapturedHeadTrainStep
    CAP, N = 5, 3
    state, feats_a, metas_a, boxes_a, labels_a = HC.setup((5, 3))
    _, feats_b, metas_b, boxes_b, labels_b = HC.setup((0, CAP), seed=162, per_sample_cameras=True)
    _, feats_c, metas_c, boxes_c, labels_c = HC.setup((2, 4), seed=262)
    head = HC.make(state, N, gt_capacity=CAP)
    twin = copy.deepcopy(head)
    recipe = dict(lr=2e-4, weight_decay=0.01, max_grad_norm=35.0)
    keys = {'sampling_offset': dict(lr_mult=0.1)}
    opt = optim.FusedAdamW(optim.param_groups(head.named_parameters(), 2e-4, 0.01, keys), **recipe)
    topt = optim.FusedAdamW(optim.param_groups(twin.named_parameters(), 2e-4, 0.01, keys), **recipe)
    params = {n: p for n, p in head.named_parameters() if p.requires_grad}
    before = {n: p.detach().clone() for n, p in params.items()}
    static = [f.clone() for f in feats_a]
    with torch.enable_grad():
        cap_step = CapturedHeadTrainStep(head, static, metas_a, optimizer=opt)
    torch.cuda.synchronize()
    assert all(torch.equal(before[n], params[n]) for n in params)
    assert all(not opt.state[p]['exp_avg'].any() and not opt.state[p]['exp_avg_sq'].any() for p in params.values())
    assert int(opt.step_count.item()) == 0 and int(opt.skipped.item()) == 0
    batches = [(feats_a, metas_a, boxes_a, labels_a), (feats_b, metas_b, boxes_b, labels_b), (feats_c, metas_c, boxes_c, labels_c)]
    for k, (feats, metas, boxes, labels) in enumerate(batches):
        noise = C.make_noise(N, 2 * CAP, 10, 500 + k)
        for dst, src in zip(static, feats):
            dst.copy_(src)
        losses = cap_step.replay(boxes, labels, metas, noise=noise)
        got_l = {n: v.clone() for n, v in losses.items()}
        want_l, _, _ = HC.step(twin, feats, metas, boxes, labels, noise)
        topt.step()
        torch.cuda.synchronize()
        HC.assert_same(got_l, want_l, 'loss, replay %d' % k)
        HC.assert_same({n: p.detach() for n, p in params.items()}, {n: p.detach() for n, p in twin.named_parameters() if p.requires_grad},
                       'parameters after replay %d' % k)
    assert cap_step.captures == 1 and int(opt.step_count.item()) == 3 and int(opt.skipped.item()) == 0
    assert not torch.equal(params['init_query_bbox.weight'], before['init_query_bbox.weight'])
    assert not torch.equal(params['label_enc.weight'], before['label_enc.weight'])
    now = {n: p.detach().clone() for n, p in params.items()}
    over_b, over_l = C.make_gt((6, 1), 10, 5)
    with pytest.raises(ValueError, match='capacity'):
        cap_step.replay(over_b, over_l)
    torch.cuda.synchronize()
    assert all(torch.equal(now[n], params[n]) for n in params) and int(opt.step_count.item()) == 3


def _rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    from sparsebev_amd.parallel import init_distributed
    from sparsebev_amd.train_graph import CapturedHeadTrainStep, CapturedTrainStep
    init_distributed(world, backend='gloo')
    seen = []
    for make in (lambda: CapturedTrainStep(None, None, None, [], [], None, optimizer=object()),
                 lambda: CapturedHeadTrainStep(None, [], [], optimizer=object())):
        try:
            with torch.enable_grad():
                make()
            seen.append('no error')
        except RuntimeError as e:
            seen.append(str(e))
    q.put((rank, seen))
    torch.distributed.destroy_process_group()


def test_two_ranks_with_an_optimizer_are_refused():
    """A process group of two ranks (gloo, on the CPU) together with optimizer=: both captured steps raise before they look at anything
    else -- DDP's gradient all-reduce is not in the graph."""
    port = 31500 + (os.getpid() % 2000)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    for rank, seen in res:
        assert len(seen) == 2 and all('optimizer= with a process group of 2 ranks' in s for s in seen), (rank, seen)
    assert 'CapturedTrainStep' in res[0][1][0] and 'CapturedHeadTrainStep' in res[0][1][1]
