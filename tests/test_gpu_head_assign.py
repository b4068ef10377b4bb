"""GPU tests of the device assignment solver (csrc/head_assign.hip, head_train.assign_device, SparseBEVTrainHead(assign_on='device')).
The yardstick is the host solver's table (sbev_head_assign on a host copy of the same costs), itself pinned against brute force, scipy
and the reference's recording by test_head_train_host.py / test_gpu_head_train.py: equality is torch.equal on the int32 tables."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import head_train_cases as C
import test_gpu_head_train as T
from conftest import load_golden
from sparsebev_amd import _lib, synthetic as S
from sparsebev_amd import head_train as HT

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64
SENTINELS = {torch.int32: -12345, torch.uint8: 0xA5}


def guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), SENTINELS[dtype], device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def host_table(cost, counts):
    """sbev_head_assign on the host copy: the yardstick."""
    cost = np.ascontiguousarray(cost.cpu().numpy(), dtype=np.float32)
    L, B, Q, Gmax = cost.shape
    counts = np.asarray(counts, dtype=np.int32)
    table = np.full((L, B, Q), 7, dtype=np.int32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    _lib.check(_lib.load().sbev_head_assign(vp(cost), vp(counts), L, B, Q, Gmax, vp(table)), 'sbev_head_assign')
    return torch.from_numpy(table)


def device_table(cost, counts, with_status=True, offsets=None):
    """sbev_head_assign_device with sentinel words around assign, status and the workspace -> (table, status) on the host."""
    lib = _lib.load()
    cost = cost.to(DEV).contiguous()
    L, B, Q, Gmax = cost.shape
    off = torch.from_numpy(offsets_of(counts) if offsets is None else np.asarray(offsets, dtype=np.int32)).to(DEV)
    nws = lib.sbev_head_assign_device_workspace(L, B, Q, Gmax)
    assert nws >= 0
    bufs = [guarded(L * B * Q, torch.int32), guarded(L * B, torch.int32), guarded(nws, torch.uint8)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lib.sbev_head_assign_device(p(cost), p(off), L, B, Q, Gmax, p(bufs[0][1]), p(bufs[1][1]) if with_status else None, p(bufs[2][1]),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(st, 'sbev_head_assign_device')
    torch.cuda.synchronize()
    for buf, view in bufs:
        s = SENTINELS[buf.dtype]
        assert bool((buf[:GUARD] == s).all()) and bool((buf[GUARD + view.numel():] == s).all()), 'a word outside an output was written'
    table, status = bufs[0][1].cpu().view(L, B, Q), bufs[1][1].cpu()
    assert not bool((table == SENTINELS[torch.int32]).any())
    if not with_status:
        assert bool((status == SENTINELS[torch.int32]).all())
    return table, status


def make_cost(kind, L, B, Q, Gmax, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'normal':
        return torch.randn(L, B, Q, Gmax, generator=g)
    if kind == 'integer':
        return torch.randint(0, 3, (L, B, Q, Gmax), generator=g).float()
    assert kind == 'ties'                     # one all-100 column (a gt with a NaN velocity), every third query row a copy of row 0
    cost = torch.randn(L, B, Q, Gmax, generator=g)
    cost[..., 0] = 100.0
    cost[:, :, 3::3, :] = cost[:, :, 0:1, :]
    return cost


def check_equal(cost, counts):
    want = host_table(cost, counts)
    got, status = device_table(cost, counts)
    assert got.dtype == torch.int32 and torch.equal(got, want)
    assert bool((status == 0).all())
    return got


@pytest.mark.parametrize('Q', range(1, 7))
def test_every_small_shape_with_ties(Q):
    L, counts, Gmax = 2, list(range(7)), 6
    cost = make_cost('integer', L, len(counts), Q, Gmax, 500 + Q)
    table = check_equal(cost, counts)
    for l in range(L):
        for b, n in enumerate(counts):
            rows = torch.nonzero(table[l, b] >= 0).reshape(-1)
            total = float(cost[l, b].double()[rows, table[l, b][rows].long()].sum())
            assert len(rows) == min(Q, n) and total == C.brute_force_total(cost[l, b, :, :n].numpy()), (l, b)      # exact on these integers


@pytest.mark.parametrize('kind', ['normal', 'integer', 'ties'])
@pytest.mark.parametrize('Q', [63, 64, 65, 255, 256, 257, 900])
def test_lane_and_wave_boundaries(Q, kind):
    counts = (5, 0, 1, 37)
    check_equal(make_cost(kind, 2, len(counts), Q, max(counts), 600 + Q), counts)


def test_more_boxes_than_queries():
    boxes, labels, cls, box = T.cost_case((40, 3), 36, 2, 77)
    gt = HT.GroundTruth(boxes, labels, DEV)
    cost = HT.match_cost(cls.to(DEV), box.to(DEV), gt, torch.tensor(C.CODE_WEIGHTS, device=DEV)).cpu()
    for cost, counts in ((cost, (40, 3)), (make_cost('normal', 2, 2, 5, 300, 78), (300, 7))):
        table = check_equal(cost, counts)
        Q = cost.shape[2]
        for l in range(cost.shape[0]):
            for b, n in enumerate(counts):
                used = table[l, b][table[l, b] >= 0]
                assert used.numel() == min(Q, n) and used.unique().numel() == used.numel() and int(used.max()) < n


def test_workspace_path():
    lib = _lib.load()
    Gmax = 3
    lo, hi = 1, 0x7fff                        # the plan is monotone in Q: bisect for the smallest Q whose state leaves LDS
    assert lib.sbev_head_assign_device_plan(lo, Gmax) == 0 and lib.sbev_head_assign_device_plan(hi, Gmax) == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if lib.sbev_head_assign_device_plan(mid, Gmax) == 1 else (mid, hi)
    assert lib.sbev_head_assign_device_plan(hi, Gmax) == 1 and lib.sbev_head_assign_device_plan(hi - 1, Gmax) == 0
    assert lib.sbev_head_assign_device_workspace(1, 2, hi, Gmax) >= 2 * (29 * hi + 13 * Gmax)
    for Q in (hi, hi - 1):
        for kind in ('normal', 'integer'):
            check_equal(make_cost(kind, 1, 2, Q, Gmax, 700 + Q), (3, 0))


def test_status():
    counts = (4, 4, 4)
    cost = torch.zeros(1, 3, 36, 6)
    cost[..., :4] = make_cost('normal', 1, 3, 36, 4, 800)
    clean = cost.clone()
    cost[0, 1, 17, 2] = float('nan')
    cost[0, 2, 5, 4] = float('inf')           # a padding column (g >= count): not read
    want = host_table(clean, counts)
    got, status = device_table(cost, counts)
    assert status.tolist() == [0, 1, 0]
    assert bool((got[0, 1] == -1).all()) and torch.equal(got[0, 0], want[0, 0]) and torch.equal(got[0, 2], want[0, 2])
    for bad in (float('inf'), float('-inf')):
        c2 = clean.clone()
        c2[0, 0, 35, 3] = bad
        got, status = device_table(c2, counts)
        assert status.tolist() == [1, 0, 0] and bool((got[0, 0] == -1).all()) and torch.equal(got[0, 1:], want[0, 1:])
    got, _ = device_table(cost, counts, with_status=False)      # a null status pointer
    assert bool((got[0, 1] == -1).all()) and torch.equal(got[0, 0], want[0, 0]) and torch.equal(got[0, 2], want[0, 2])
    # counts the host never sees: one above Gmax and a negative one are clamped, flagged, and read nothing out of bounds
    got, status = device_table(clean, counts, offsets=[0, 9, 5, 9])
    assert status.tolist() == [1, 1, 0] and bool((got[0, :2] == -1).all()) and torch.equal(got[0, 2], want[0, 2])
    # Gmax == 0: the launch fills the table
    got, status = device_table(torch.zeros(2, 2, 5, 0), (0, 0))
    assert bool((got == -1).all()) and bool((status == 0).all())


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_reference_recording(tag):
    c = C.fixture_case(load_golden('g15_head_train'), tag)
    pad = c['pad']
    head = T.make_head(assign_on='device').to(DEV)
    gt = HT.GroundTruth(c['boxes'], c['labels'], DEV)
    cd, bd = c['cls'].to(DEV), c['box'].to(DEV)
    a = head.assign(cd[:, :, pad:], bd[:, :, pad:], gt)                  # case a: the NaN-velocity tie column
    assert a.dtype == torch.int32 and a.is_cuda and torch.equal(a.cpu().long(), c['assign'].long())
    assert head.assign_status.shape == (a.shape[0] * a.shape[1],) and bool((head.assign_status == 0).all())
    host = T.make_head().to(DEV)
    assert torch.equal(a, host.assign(cd[:, :, pad:], bd[:, :, pad:], gt))


def test_inside_a_captured_graph():
    L, B, Q, Gmax = 2, 2, 36, 8
    _lib.load()
    cw = torch.tensor(C.CODE_WEIGHTS, device=DEV)
    gt = HT.GroundTruth([torch.ones(Gmax, 9)] * B, [torch.zeros(Gmax, dtype=torch.long)] * B, DEV)      # capacity B * Gmax, single = Gmax
    assert gt.single == Gmax and gt.boxes.shape == (B * Gmax, 9)
    cls, box = torch.zeros(L, B, Q, 10, device=DEV), torch.zeros(L, B, Q, 10, device=DEV)
    status = torch.zeros(L * B, dtype=torch.int32, device=DEV)

    def run():
        cost = HT.match_cost(cls, box, gt, cw)
        return cost, HT.assign_device(cost, gt, status)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):          # a synchronisation or a host read in here would raise
        cost, table = run()
    for k, counts in enumerate([(8, 0), (3, 5), (1, 8)]):
        boxes, labels, c, b = T.cost_case(counts, Q, L, 900 + k)
        G = sum(counts)
        cls.copy_(c.to(DEV)), box.copy_(b.to(DEV))
        gt.boxes[:G].copy_(torch.cat(boxes).to(DEV)), gt.labels[:G].copy_(torch.cat(labels).to(DEV).int())
        gt.offsets.copy_(torch.from_numpy(offsets_of(counts)).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        eager = HT.match_cost(cls, box, HT.GroundTruth(boxes, labels, DEV), cw)
        assert torch.equal(cost[..., :max(counts)], eager) and float(cost[..., max(counts):].abs().max() if max(counts) < Gmax else 0.0) == 0.0
        assert torch.equal(table.cpu(), host_table(cost, counts)) and bool((status == 0).all()), counts
        assert int((table >= 0).sum()) == L * sum(min(Q, n) for n in counts)


def end_to_end_setup():
    """test_gpu_head_train.py::test_train_head_end_to_end's set-up: (state dict source head, feats, metas, boxes, labels, noise)."""
    Tn, B = 2, 2
    ih, iw, sizes = S.PYRAMIDS['tiny']
    head = T.make_head()
    params = S.make_params(61, embed_dims=256, num_frames=Tn, num_points=4, num_levels=4)
    head.transformer.load_state_dict({'decoder.decoder_layer.' + k: v for k, v in params.items()}, strict=True)
    with torch.no_grad():
        head.init_query_bbox.weight[:, 2] = 0.5
        head.init_query_bbox.weight[:, 5] = 0.5
    feats = [f.to(DEV) for f in S.make_features(B, Tn, sizes, seed=62)]
    boxes, labels = C.make_gt((5, 3), 10, 63)
    metas = S.make_img_metas(B, Tn, ih, iw)
    for m, b, l in zip(metas, boxes, labels):
        m['gt_bboxes_3d'], m['gt_labels_3d'] = b, l
    noise = C.make_noise(head.dn_group_num, 8, 10, 64)
    return head, feats, metas, boxes, labels, noise


def twin(src, noise, assign_on):
    head = T.make_head(assign_on=assign_on)
    head.load_state_dict(src.state_dict(), strict=True)
    layer = head.transformer.decoder.decoder_layer
    layer.self_attn.attn_drop, layer.ffn_drop = 0.0, 0.0               # dropout off: the loss is a function of the inputs alone
    head.draw_noise = lambda G, device: tuple(t.to(device) for t in noise)      # the same recorded noise for every head
    return head.to(DEV).train()


def step(head, feats, metas, boxes, labels):
    head.zero_grad()
    with torch.enable_grad():
        outs = head(feats, copy.deepcopy(metas))
        losses = head.loss(boxes, labels, outs)
        sum(losses.values()).backward()
    return {k: v.detach().clone() for k, v in losses.items()}, {n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None}


def test_loss_dict_host_vs_device():
    src, feats, metas, boxes, labels, noise = end_to_end_setup()
    host, dev = twin(src, noise, 'host'), twin(src, noise, 'device')
    assert list(host.state_dict()) == list(dev.state_dict())
    l_host, g_host = step(host, feats, metas, boxes, labels)
    l_ctrl, g_ctrl = step(host, feats, metas, boxes, labels)            # the control: the host path against itself
    l_dev, g_dev = step(dev, feats, metas, boxes, labels)
    assert bool((dev.assign_status == 0).all()) and host.assign_status is None
    assert sorted(l_dev) == sorted(l_host) and len(l_dev) == 8
    for k in l_host:
        assert torch.equal(l_dev[k], l_host[k]) and torch.equal(l_ctrl[k], l_host[k]), k
    assert sorted(g_dev) == sorted(g_host)
    loose = []
    for n in g_host:
        if torch.equal(g_ctrl[n], g_host[n]):
            assert torch.equal(g_dev[n], g_host[n]), n
        else:                                   # an atomics-ordered sum upstream: the host path does not repeat itself here either
            loose.append(n)
            spread = (g_ctrl[n] - g_host[n]).abs().max().item()
            assert (g_dev[n] - g_host[n]).abs().max().item() <= 4 * spread, n
    print('parameter gradients: %d bit-equal, %d that the host path itself does not repeat bit for bit' % (len(g_host) - len(loose), len(loose)))


def test_no_synchronisation_in_loss():
    src, feats, metas, boxes, labels, noise = end_to_end_setup()
    host, dev = twin(src, noise, 'host'), twin(src, noise, 'device')
    preds = []
    for head in (host, dev):
        with torch.no_grad():
            preds.append(head(feats, copy.deepcopy(metas)))
        head.loss(boxes, labels, preds[-1])      # allocations, staging buffers and the library's one-time set-up happen here
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            host.loss(boxes, labels, preds[0])
            control_raised = False
        except RuntimeError:
            control_raised = True
        if control_raised:
            dev.loss(boxes, labels, preds[1])    # raises if anything in it synchronises
    finally:
        torch.cuda.set_sync_debug_mode('default')
    if not control_raised:
        pytest.skip("torch's sync debug mode does not flag the host path's stream synchronisation on this build; "
                    'test_inside_a_captured_graph carries the claim')
