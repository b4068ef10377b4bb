"""GPU tests of the training head at a fixed ground-truth capacity: the plan launch (csrc/head_train.hip::capacity_plan_kernel),
``head_train.GroundTruthSlab``, ``SparseBEVTrainHead(gt_capacity=...)`` and ``train_graph.CapturedHeadTrainStep``.

The capacity path is the dynamic path with ``single`` forced to the capacity, so its references are the dynamic path itself (bit for
bit), the fp64 restatement of tests/head_train_cases.py and the reference's recording (fixture G15)."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import head_train_cases as C
import test_gpu_head_train as T
from conftest import load_golden
from sparsebev_amd import _lib, synthetic as S
from sparsebev_amd import head_train as HT

pytestmark = pytest.mark.gpu
DEV = T.DEV
PLAN_BLOCK = 256            # threads of capacity_plan_kernel's workgroup: one thread per element of the flat [B, N * capacity] codes
I_SENTINEL = -7777777


# ---- helpers ----------------------------------------------------------------------------------------------------------------

def guarded_i32(n):
    """test_gpu_head_train.guarded() for an int32 output (its sentinel is not an integer)"""
    buf = torch.full((n + 2 * T.GUARD,), I_SENTINEL, device=DEV, dtype=torch.int32)
    return buf, buf[T.GUARD:T.GUARD + n]


def untouched(buf, n, sentinel):
    return bool((buf[:T.GUARD] == sentinel).all()) and bool((buf[T.GUARD + n:] == sentinel).all())


host_plan = C.host_plan


def force_single(monkeypatch, single):
    """the dynamic path with every ``GroundTruth.single`` forced to ``single`` (legal for its kernels while single <= G) -- patched here,
    not in the product"""
    init = HT.GroundTruth.__init__

    def forced(self, *a, **kw):
        init(self, *a, **kw)
        self.single = single

    monkeypatch.setattr(HT.GroundTruth, '__init__', forced)


def raw_plan(offsets, B, Q, cap, N, bg):
    """sbev_head_capacity_plan with sentinel words around its three outputs; checks them, returns (codes, avg, status)."""
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    n = B * N * cap
    (cb, codes), (ab, avg), (sb, status) = guarded_i32(n), T.guarded(4), guarded_i32(1)
    off = torch.as_tensor(offsets, dtype=torch.int32).to(DEV)
    st = lib.sbev_head_capacity_plan(p(off), B, Q, cap, N, float(bg), p(codes), p(avg), p(status), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(st, 'sbev_head_capacity_plan')
    torch.cuda.synchronize()
    assert untouched(cb, n, I_SENTINEL) and untouched(ab, 4, T.SENTINEL) and untouched(sb, 1, I_SENTINEL), 'a word outside an output was written'
    return codes.clone().view(B, N * cap).cpu(), avg.clone().view(2, 2).cpu(), int(status.item())


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def scatter_noise(noise, counts, cap, N):
    """noise of the dynamic layout (row r * G + gi, G = sum(counts)) in the capacity layout (row r * B * cap + gi); the rest zero"""
    G, Gc = sum(counts), len(counts) * cap
    out = []
    for t in noise:
        t = torch.as_tensor(t)
        big = torch.zeros((N * Gc,) + tuple(t.shape[1:]), dtype=t.dtype)
        if G:
            big.view((N, Gc) + tuple(t.shape[1:]))[:, :G] = t.reshape((N, G) + tuple(t.shape[1:]))
        out.append(big)
    return tuple(out)


def setup(counts=(5, 3), seed=62, per_sample_cameras=False):
    """test_gpu_head_train.py::test_train_head_end_to_end's set-up: (state dict, feats, metas with the gt, boxes, labels)"""
    Tn, B = 2, len(counts)
    ih, iw, sizes = S.PYRAMIDS['tiny']
    head = T.make_head()
    params = S.make_params(61, embed_dims=256, num_frames=Tn, num_points=4, num_levels=4)
    head.transformer.load_state_dict({'decoder.decoder_layer.' + k: v for k, v in params.items()}, strict=True)
    with torch.no_grad():
        head.init_query_bbox.weight[:, 2] = 0.5
        head.init_query_bbox.weight[:, 5] = 0.5
    feats = [f.to(DEV) for f in S.make_features(B, Tn, sizes, seed=seed)]
    boxes, labels = C.make_gt(counts, 10, seed + 1)
    metas = (S.make_img_metas_per_sample if per_sample_cameras else S.make_img_metas)(B, Tn, ih, iw)
    for m, b, l in zip(metas, boxes, labels):
        m['gt_bboxes_3d'], m['gt_labels_3d'] = b, l
    return head.state_dict(), feats, metas, boxes, labels


def make(state, groups=3, dropout=False, **kw):
    head = T.make_head(assign_on='device', **kw)
    head.load_state_dict(state, strict=True)
    head.dn_group_num = groups
    if not dropout:
        layer = head.transformer.decoder.decoder_layer
        layer.self_attn.attn_drop, layer.ffn_drop = 0.0, 0.0           # dropout off: the loss is a function of the inputs alone
    return head.to(DEV).train()


def step(head, feats, metas, boxes, labels, noise):
    head.zero_grad()
    head.dn_noise = tuple(t.to(DEV) for t in noise)
    with torch.enable_grad():
        outs = head(feats, copy.deepcopy(metas))
        losses = head.loss(boxes, labels, outs)
        sum(losses.values()).backward()
    return ({k: v.detach().clone() for k, v in losses.items()}, {n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None},
            outs)


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert torch.equal(got[k], want[k]), (what, k, (got[k].double() - want[k].double()).abs().max().item())


# ---- 1. the plan launch -----------------------------------------------------------------------------------------------------

PLAN_CASES = [
    ((0,), 36, 4, 2, 0.0),
    ((0, 5, 2), 36, 5, 3, 0.0),                 # counts (0, cap, 2)
    ((0, 5, 2), 36, 5, 3, 0.1),
    ((5,), 3, 5, 2, 0.0),                       # Q = 3 < count 5: min(c, Q)
    ((5,), 3, 5, 2, 0.1),
    ((1,), 36, 1, 1, 0.1),                      # N * capacity = 1
    ((200,), 36, 255, 1, 0.0),                  # PLAN_BLOCK - 1, PLAN_BLOCK, PLAN_BLOCK + 1
    ((128,), 36, 128, 2, 0.1),
    ((257,), 36, 257, 1, 0.0),
    ((340,), 900, 341, 3, 0.1),                 # 4 * PLAN_BLOCK - 1, 4 * PLAN_BLOCK, 4 * PLAN_BLOCK + 1
    ((3,), 900, 512, 2, 0.0),
    ((205,), 900, 205, 5, 0.1),
    ((43, 0, 17), 36, 43, 2, 0.1),              # B * N * capacity = 258: samples share a workgroup, the last one is partial
]


@pytest.mark.parametrize('counts,Q,cap,N,bg', PLAN_CASES, ids=['c%s_q%d_cap%d_n%d_bg%g' % ('-'.join(map(str, c[0])), c[1], c[2], c[3], c[4]) for c in PLAN_CASES])
def test_plan_vs_host_restatement(counts, Q, cap, N, bg):
    B = len(counts)
    codes, avg, status = raw_plan(offsets_of(counts), B, Q, cap, N, bg)
    want_codes, want_avg = host_plan(counts, Q, cap, N, bg)
    assert status == 0
    assert torch.equal(codes, want_codes)
    assert torch.equal(avg, want_avg), (avg.tolist(), want_avg.tolist())
    # the wrapper hands out the same three tensors
    c2, a2, s2 = HT.capacity_plan(torch.from_numpy(offsets_of(counts)).to(DEV), B, Q, cap, N, bg)
    assert torch.equal(c2.cpu(), want_codes) and torch.equal(a2.cpu(), want_avg) and s2.tolist() == [0]
    assert c2.shape == (B, N * cap) and a2.shape == (2, 2) and c2.dtype == torch.int32 and a2.dtype == torch.float32


def test_plan_flags_and_clamps_bad_offsets():
    B, Q, cap, N = 2, 36, 4, 2
    # one count = cap + 2: flagged, and everything written is what the clamped counts (4, 1) give; the guards are checked in raw_plan
    codes, avg, status = raw_plan([0, cap + 2, cap + 3], B, Q, cap, N, 0.1)
    want_codes, want_avg = host_plan((cap, 1), Q, cap, N, 0.1)
    assert status == HT.PLAN_COUNT_ABOVE_CAPACITY
    assert torch.equal(codes, want_codes) and torch.equal(avg, want_avg)
    # offsets that go down: the negative count reads as 0
    codes, avg, status = raw_plan([0, 3, 1], B, Q, cap, N, 0.0)
    want_codes, want_avg = host_plan((3, 0), Q, cap, N, 0.0)
    assert status == HT.PLAN_OFFSETS_NOT_MONOTONE
    assert torch.equal(codes, want_codes) and torch.equal(avg, want_avg)
    # a total above B * capacity
    codes, avg, status = raw_plan([0, 4, 9], B, Q, cap, N, 0.0)
    assert status == HT.PLAN_COUNT_ABOVE_CAPACITY | HT.PLAN_TOTAL_ABOVE_CAPACITY
    assert torch.equal(codes, host_plan((4, 4), Q, cap, N, 0.0)[0])
    # offsets that do not start at 0
    assert raw_plan([1, 2, 3], B, Q, cap, N, 0.0)[2] == HT.PLAN_OFFSETS_NOT_MONOTONE
    # capacity 0 and B = 0: the factors and the status are still written
    codes, avg, status = raw_plan([0, 0, 0], B, Q, 0, N, 0.1)
    assert status == 0 and codes.numel() == 0 and torch.equal(avg, host_plan((0, 0), Q, 0, N, 0.1)[1])
    codes, avg, status = raw_plan([0], 0, Q, cap, N, 0.1)
    assert status == 0 and codes.numel() == 0 and float(avg.abs().max()) == 0.0


# ---- 2. capacity == the batch's maximum is the dynamic path ---------------------------------------------------------------------

def test_capacity_at_batch_maximum_is_the_dynamic_path():
    counts, N = (5, 3), 3
    state, feats, metas, boxes, labels = setup(counts)
    dyn, cap = make(state, N), make(state, N, gt_capacity=5)
    noise = C.make_noise(N, sum(counts), 10, 64)
    l_dyn, g_dyn, o_dyn = step(dyn, feats, metas, boxes, labels, noise)
    l_cap, g_cap, o_cap = step(cap, feats, metas, boxes, labels, scatter_noise(noise, counts, 5, N))
    assert len(l_dyn) == 8 and o_cap['dn_mask_dict']['pad_size'] == 5 * N == o_dyn['dn_mask_dict']['pad_size']
    assert cap.plan_status.tolist() == [0] and bool((cap.assign_status == 0).all())
    assert_same(l_cap, l_dyn, 'loss')
    assert_same(g_cap, g_dyn, 'gradient')
    assert float(g_cap['init_query_bbox.weight'].abs().max()) > 0 and float(g_cap['label_enc.weight'].abs().max()) > 0


# ---- 3. capacity above the maximum -------------------------------------------------------------------------------------------

def test_capacity_above_the_batch_maximum(monkeypatch):
    counts, N, CAP = (5, 3), 3, 7
    state, feats, metas, boxes, labels = setup(counts)
    cap = make(state, N, gt_capacity=CAP)
    noise = C.make_noise(N, sum(counts), 10, 64)
    l_cap, g_cap, outs = step(cap, feats, metas, boxes, labels, scatter_noise(noise, counts, CAP, N))
    md = outs['dn_mask_dict']
    assert md['pad_size'] == CAP * N and outs['all_cls_scores'].shape == (2, 2, 36, 10) and cap.plan_status.tolist() == [0]
    # (a) the restatement on the head's own outputs.  C.loss_dict lays the dn rows out at single = max(counts): hand it rows k < 5 of
    # every group (the rows k = 5, 6 it does not see are filler rows of both samples, code -2)
    rows = torch.cat([torch.arange(5) + CAP * r for r in range(N)])
    dn_cls, dn_box = [t.detach().cpu().double()[:, :, rows] for t in md['output_known_lbs_bboxes']]
    ref = C.loss_dict(outs['all_cls_scores'].detach().cpu().double(), outs['all_bbox_preds'].detach().cpu().double(), dn_cls, dn_box,
                      boxes, labels, torch.tensor(C.CODE_WEIGHTS, dtype=torch.float64), N)
    assert sorted(ref) == sorted(l_cap)
    for k, v in ref.items():
        print('capacity %d %-16s restatement %.6f  rel err %.2e' % (CAP, k, v.item(), abs(l_cap[k].item() - v.item()) / abs(v.item())))
        assert abs(l_cap[k].item() - v.item()) < T.FUNC_TOL * abs(v.item()), (k, l_cap[k].item(), v.item())
    # (b) the dynamic path with gt.single forced to the capacity (legal for its kernels: 7 <= G = 8)
    force_single(monkeypatch, CAP)
    dyn = make(state, N)
    l_dyn, g_dyn, o_dyn = step(dyn, feats, metas, boxes, labels, noise)
    assert o_dyn['dn_mask_dict']['pad_size'] == CAP * N
    assert_same(l_cap, l_dyn, 'loss')
    assert_same(g_cap, g_dyn, 'gradient')


# ---- 3b. loss() handed other objects than the forward ---------------------------------------------------------------------------

def forward_on(head, feats, metas, noise):
    head.dn_noise = tuple(t.to(DEV) for t in noise)
    with torch.enable_grad():
        return head(feats, metas)


def dn_keys(losses):
    return {k: v for k, v in losses.items() if k.endswith('_dn')}


def test_other_objects_in_loss_dynamic_path():
    """The matching pair reads loss()'s arguments, the dn pair keeps the forward's ground truth (md['gt']): codes, factors, boxes, labels."""
    N = 3
    state, feats, metas, boxes_a, labels_a = setup((5, 3))
    boxes_b, labels_b = C.make_gt((4, 3), 10, 99)
    head = make(state, N)
    metas = copy.deepcopy(metas)
    own_a = [m['gt_bboxes_3d'] for m in metas], [m['gt_labels_3d'] for m in metas]       # the very objects the forward reads
    outs = forward_on(head, feats, metas, C.make_noise(N, 8, 10, 64))
    plain = {k: v for k, v in outs.items() if k != 'dn_mask_dict'}
    assert outs['dn_mask_dict']['gt'].same_as(*own_a) and not outs['dn_mask_dict']['gt'].same_as(boxes_a, labels_a)
    with torch.enable_grad():
        l_own, l_a = head.loss(*own_a, outs), head.loss(boxes_a, labels_a, outs)         # one source; an equal upload next to it
        l_b, l_b_plain = head.loss(boxes_b, labels_b, outs), head.loss(boxes_b, labels_b, plain)
    assert len(l_b) == 8 and len(l_b_plain) == 4 and not dn_keys(l_b_plain) and head.plan_status is None
    assert_same(l_own, l_a, 'the same objects vs copies of them')
    assert_same({k: v for k, v in l_b.items() if k not in dn_keys(l_b)}, l_b_plain, 'matching pair: the arguments')
    assert_same(dn_keys(l_b), dn_keys(l_a), "dn pair: the forward's")
    assert all(not torch.equal(l_b[k], l_a[k]) for k in l_b_plain)


def test_other_objects_in_loss_capacity_path(monkeypatch):
    """One slab, refreshed in place: both pairs read loss()'s arguments."""
    N, CAP = 3, 7
    state, feats, metas, boxes_a, labels_a = setup((5, 3))
    boxes_b, labels_b = C.make_gt((4, 3), 10, 99)
    cap = make(state, N, gt_capacity=CAP)
    outs = forward_on(cap, feats, copy.deepcopy(metas), scatter_noise(C.make_noise(N, 8, 10, 64), (5, 3), CAP, N))
    slab = outs['dn_mask_dict']['gt']
    with torch.enable_grad():
        l_a = cap.loss(boxes_a, labels_a, outs)
        l_b = cap.loss(boxes_b, labels_b, outs)
    assert slab is cap.gt_slab(2, DEV) and slab.same_as(boxes_b, labels_b) and slab.counts == [4, 3] and cap.plan_status.tolist() == [0]

    def no_update(*a, **kw):
        raise AssertionError('the slab holds these objects: no second update')

    with monkeypatch.context() as mp, torch.enable_grad():
        mp.setattr(slab, 'update', no_update)
        assert_same(cap.loss(boxes_b, labels_b, outs), l_b, 'a second loss() on the same objects')
    assert all(not torch.equal(l_b[k], l_a[k]) for k in l_b)
    # the same predictions through the dynamic path, its md['gt'] built from B at single = CAP (7 <= G = 7)
    force_single(monkeypatch, CAP)
    md = dict(outs['dn_mask_dict'], gt=HT.GroundTruth(boxes_b, labels_b, DEV))
    assert md['gt'].single == CAP and md['pad_size'] == CAP * N
    with torch.enable_grad():
        l_dyn = make(state, N).loss(boxes_b, labels_b, dict(outs, dn_mask_dict=md))
    assert_same(dn_keys(l_b), dn_keys(l_dyn), 'dn pair at capacity: the arguments')
    assert_same(l_b, l_dyn, 'both pairs')


def test_dn_backward_at_capacity_vs_restatement():
    """Both gradients of sbev_head_dn_prepare_bwd at capacity against autograd through the fp64 restatement, with the words of
    noised_label that the forward does not write (rows behind offsets[B]) set to a real class id and a gradient on every filler row."""
    B, N, NC, counts, CAP, Q, D, seed = 3, 2, 10, (5, 0, 3), 7, 25, 20, 71
    G, Gc = sum(counts), B * CAP
    boxes, labels = C.make_gt(counts, NC, seed)
    init_w, label_w = C.make_embeddings(Q, NC, D, seed + 1)
    noise = C.make_noise(N, G, NC, seed + 2)
    slab = HT.GroundTruthSlab(B, CAP, DEV).update(boxes, labels)
    iw, lw = init_w.to(DEV).requires_grad_(True), label_w.to(DEV).requires_grad_(True)
    big = [t.to(DEV) for t in scatter_noise(noise, counts, CAP, N)]
    g = torch.Generator().manual_seed(seed + 3)
    Tq = CAP * N + Q
    gb, gf = torch.randn(B, Tq, 10, generator=g), torch.randn(B, Tq, D, generator=g)
    with torch.enable_grad():
        qb, qf, mask, noised = HT.dn_prepare(iw, lw, slab, big[0], big[1], big[2].int(), B, N, NC, C.PC_RANGE)
        got = torch.autograd.grad([qb, qf], [iw, lw], [gb.to(DEV), gf.to(DEV)])
    # forward at capacity = the restatement with its rows moved: row r * 5 + k of the restatement is row r * CAP + k here
    ref32 = C.dn_prepare(init_w, label_w, boxes, labels, noise, N, NC)
    single = max(counts)
    rows = torch.cat([torch.arange(single) + CAP * r for r in range(N)] + [torch.arange(Q) + CAP * N])
    filler = torch.ones(Tq, dtype=torch.bool)
    filler[rows] = False
    assert float(qb[:, filler].abs().max()) == 0.0 and float(qf[:, filler].abs().max()) == 0.0
    valid = (torch.arange(N)[:, None] * Gc + torch.arange(G)[None, :]).reshape(-1)
    T.check_dn_forward((qb[:, rows], qf[:, rows], mask[rows][:, rows], noised[valid.to(DEV)]), ref32, 'capacity')
    assert mask.shape == (Tq, Tq) and torch.equal(mask.cpu(), C.dn_prepare(init_w, label_w, [torch.ones(CAP, 9)], [torch.zeros(CAP)],
                                                                           C.make_noise(N, CAP, NC, 1), N, NC)['attn_mask'])
    # backward, fp64 autograd through the restatement with the upstream gradient of the rows it has
    i64, l64 = init_w.double().requires_grad_(True), label_w.double().requires_grad_(True)
    with torch.enable_grad():
        r64 = C.dn_prepare(i64, l64, boxes, labels, (noise[0].double(), noise[1], noise[2]), N, NC)
        ((r64['query_bbox'] * gb[:, rows].double()).sum() + (r64['query_feat'] * gf[:, rows].double()).sum()).backward()
    e_init, e_lab = T.rel(got[0], i64.grad), T.rel(got[1], l64.grad)
    print('dn backward at capacity: rel err init %.2e label_enc %.2e' % (e_init, e_lab))
    assert e_init < T.FUNC_TOL and e_lab < T.FUNC_TOL
    # the raw launch with the unwritten label words set to class 3: the same gradients, bit for bit
    lib, p = _lib.load(), (lambda t: ctypes.c_void_p(t.data_ptr()))
    poisoned = noised.clone()
    unwritten = torch.ones(N * Gc, dtype=torch.bool)
    unwritten[valid] = False
    poisoned[unwritten.to(DEV)] = 3
    (ib, g_init), (lb, g_label) = T.guarded(Q * 10), T.guarded((NC + 1) * (D - 1))
    gbd, gfd = gb.to(DEV).contiguous(), gf.to(DEV).contiguous()
    st = lib.sbev_head_dn_prepare_bwd(p(gbd), p(gfd), p(poisoned), p(slab.offsets), B, Q, D, NC, Gc, N, CAP, p(g_init), p(g_label),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(st, 'sbev_head_dn_prepare_bwd')
    torch.cuda.synchronize()
    assert untouched(ib, Q * 10, T.SENTINEL) and untouched(lb, (NC + 1) * (D - 1), T.SENTINEL)
    assert torch.equal(g_init.view(Q, 10), got[0]) and torch.equal(g_label.view(NC + 1, D - 1), got[1])
    assert T.rel(g_label.view(NC + 1, D - 1), l64.grad) < T.FUNC_TOL


# ---- 4. the reference's recording -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', C.FIXTURE_CASES)
def test_reference_recording_at_recorded_capacity(tag):
    c = C.fixture_case(load_golden('g15_head_train'), tag)
    N, NC, pad, counts = c['N'], c['NC'], c['pad'], c['counts']
    cap, B = pad // N, len(counts)
    assert cap == max(counts)
    head = T.make_head(assign_on='device', gt_capacity=cap)
    head.dn_group_num = N
    head = head.to(DEV).train()
    label_enc = nn.Embedding(NC + 1, c['label_w'].shape[1]).to(DEV)
    with torch.no_grad():
        label_enc.weight.copy_(c['label_w'])
    metas = [{'gt_bboxes_3d': b, 'gt_labels_3d': l} for b, l in zip(c['boxes'], c['labels'])]
    noise = scatter_noise((c['u_box'], c['u_lab'], c['new_lab']), counts, cap, N)
    qb, qf, mask, md = head.prepare_for_dn_input(B, c['init_w'].to(DEV), label_enc, metas, noise=noise)
    assert md['pad_size'] == pad and mask.dtype == torch.bool and md['gt'] is head.gt_slab(B, DEV)
    # the dn queries within check_dn_forward's bounds of the recording
    slab = md['gt']
    out = HT.dn_prepare(c['init_w'].to(DEV), c['label_w'].to(DEV), slab, *[t.to(DEV) for t in noise[:2]], noise[2].to(DEV).int(), B, N, NC, C.PC_RANGE)
    G = sum(counts)
    valid = (torch.arange(N)[:, None] * (B * cap) + torch.arange(G)[None, :]).reshape(-1).to(DEV)
    ref = dict(query_bbox=c['query_bbox'], query_feat=c['query_feat'], attn_mask=c['attn_mask'],
               noised_labels=C.dn_prepare(c['init_w'], c['label_w'], c['boxes'], c['labels'], (c['u_box'], c['u_lab'], c['new_lab']), N, NC)['noised_labels'])
    T.check_dn_forward((out[0], out[1], out[2], out[3][valid]), ref, tag)
    assert torch.equal(T.bits(qb), T.bits(out[0])) and torch.equal(T.bits(qf), T.bits(out[1])) and torch.equal(mask, out[2])
    # the loss dict on the recorded decoder outputs
    cls, box = c['cls'].to(DEV), c['box'].to(DEV)
    preds = {'all_cls_scores': cls[:, :, pad:], 'all_bbox_preds': box[:, :, pad:], 'enc_cls_scores': None, 'enc_bbox_preds': None}
    if pad:
        md['output_known_lbs_bboxes'] = (cls[:, :, :pad], box[:, :, :pad])
        preds['dn_mask_dict'] = md
    losses = head.loss(c['boxes'], c['labels'], preds)
    assert sorted(losses) == [str(k) for k in c['loss_keys']] and head.plan_status.tolist() == [0]
    for k, v in zip(c['loss_keys'], c['loss_values']):
        got = losses[str(k)]
        print('capacity loss dict %s %-16s reference %.6f  |diff| %.2e' % (tag, k, v.item(), abs(got.item() - v.item())))
        assert got.dim() == 0 and abs(got.item() - v.item()) <= 1e-4, (str(k), got.item(), v.item())


# ---- 5. update() at fixed addresses -------------------------------------------------------------------------------------------

def test_slab_update_in_place_and_empty_batch():
    state, feats, metas, boxes, labels = setup((5, 3))
    slab = HT.GroundTruthSlab(2, 5, DEV)
    assert (slab.single, slab.G, slab.B) == (5, 10, 2) and slab.boxes.shape == (10, 9) and slab.labels.shape == (10,) and slab.offsets.shape == (3,)
    assert slab.boxes.dtype == torch.float32 and slab.labels.dtype == torch.int32 and slab.offsets.dtype == torch.int32
    ptrs = (slab.boxes.data_ptr(), slab.labels.data_ptr(), slab.offsets.data_ptr())

    class Box:                                   # a duck-typed box object: gravity_center + tensor[:, 3:]
        def __init__(self, t):
            self.tensor = t.clone()
            self.tensor[:, 2] -= 7.0
            self.gravity_center = t[:, :3]

    for bl, ll in ((boxes, labels), ([Box(b) for b in boxes[::-1]], labels[::-1]), ([torch.zeros(0, 9)] * 2, [torch.zeros(0)] * 2), (boxes, labels)):
        slab.update(bl, ll)
        plain = [b if torch.is_tensor(b) else torch.cat([b.gravity_center, b.tensor[:, 3:]], dim=1) for b in bl]
        n = sum(b.shape[0] for b in plain)
        assert (slab.boxes.data_ptr(), slab.labels.data_ptr(), slab.offsets.data_ptr()) == ptrs
        assert slab.counts == [b.shape[0] for b in plain] and slab.offsets.tolist() == slab.offsets_host.tolist() == offsets_of(slab.counts).tolist()
        assert torch.equal(slab.boxes[:n].cpu(), torch.cat(plain)) and torch.equal(slab.labels[:n].cpu().long(), torch.cat(ll).long())
        assert float(slab.boxes[n:].abs().max()) == 0.0 and slab.same_as(bl, ll) and not slab.same_as([torch.zeros(1, 9)] * 2, ll)
    # above the capacity: ValueError, nothing enqueued, nothing changed
    before = slab.buffer.clone()
    over_b, over_l = C.make_gt((6, 1), 10, 5)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')     # (a copy to the host would raise here; a launch would change the buffer)
    try:
        with pytest.raises(ValueError, match='capacity'):
            slab.update(over_b, over_l)
        with pytest.raises(ValueError):
            slab.update(boxes[:1], labels[:1])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(slab.buffer, before) and slab.counts == [5, 3] and slab.same_as(boxes, labels)
    head = make(state, 3, gt_capacity=5)
    for m, b, l in zip(metas, over_b, over_l):
        m['gt_bboxes_3d'], m['gt_labels_3d'] = b, l
    with pytest.raises(ValueError, match='capacity'):
        head(feats, metas)
    # an all-empty batch: the dn keys stay, at 0.0, and the backward is finite
    for m in metas:
        m['gt_bboxes_3d'], m['gt_labels_3d'] = torch.zeros(0, 9), torch.zeros(0, dtype=torch.long)
    with torch.enable_grad():
        outs = head(feats, metas)
        assert outs['dn_mask_dict']['pad_size'] == 15 and outs['all_cls_scores'].shape == (2, 2, 36, 10)
        l0 = head.loss([m['gt_bboxes_3d'] for m in metas], [m['gt_labels_3d'] for m in metas], outs)
        sum(l0.values()).backward()
    assert sorted(l0) == sorted(['loss_cls', 'loss_bbox', 'd0.loss_cls', 'd0.loss_bbox', 'loss_cls_dn', 'loss_bbox_dn', 'd0.loss_cls_dn', 'd0.loss_bbox_dn'])
    assert all(l0[k].item() == 0.0 for k in l0 if k.endswith('_dn')) and l0['loss_bbox'].item() == 0.0 and l0['loss_cls'].item() > 0
    assert head.plan_status.tolist() == [0]
    for name, p in head.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name


# ---- 6. the captured step -------------------------------------------------------------------------------------------------------

def test_captured_head_step_vs_eager(monkeypatch):
    from sparsebev_amd.train_graph import CapturedHeadTrainStep
    CAP, N = 5, 3
    state, feats_a, metas_a, boxes_a, labels_a = setup((5, 3))
    _, feats_b, metas_b, boxes_b, labels_b = setup((0, CAP), seed=162, per_sample_cameras=True)
    head = make(state, N, gt_capacity=CAP)
    twin = copy.deepcopy(head)                   # made before the first step
    static = [f.clone() for f in feats_a]
    with torch.enable_grad():
        cap_step = CapturedHeadTrainStep(head, static, metas_a)
    assert cap_step.captures == 1
    assert sorted(cap_step.grads) == sorted(n for n, p in head.named_parameters() if p.requires_grad)
    assert 'init_query_bbox.weight' in cap_step.grads and 'label_enc.weight' in cap_step.grads
    ptrs = {n: g.data_ptr() for n, g in cap_step.grads.items()}
    seen = []
    for k, (feats, metas, boxes, labels) in enumerate([(feats_a, metas_a, boxes_a, labels_a), (feats_b, metas_b, boxes_b, labels_b),
                                                       (feats_a, metas_a, boxes_a, labels_a)]):
        noise = C.make_noise(N, 2 * CAP, 10, 500 + (k % 2))            # at capacity; the third step draws the first one's again
        for dst, src in zip(static, feats):
            dst.copy_(src)
        losses = cap_step.replay(boxes, labels, metas, noise=noise)
        torch.cuda.synchronize()
        got_l, got_g = {n: v.clone() for n, v in losses.items()}, {n: g.clone() for n, g in cap_step.grads.items()}
        want_l, want_g, _ = step(twin, feats, metas, boxes, labels, noise)
        assert len(got_l) == 8 and head.plan_status.tolist() == [0] and bool((head.assign_status == 0).all())
        assert_same(got_l, want_l, 'loss, replay %d' % k)
        assert_same(got_g, want_g, 'gradient, replay %d' % k)
        seen.append((got_l, got_g))
    assert_same(seen[2][0], seen[0][0], 'third replay vs first')
    assert_same(seen[2][1], seen[0][1], 'third replay vs first')
    assert any(not torch.equal(seen[1][0][k], seen[0][0][k]) for k in seen[0][0])
    assert all(seen[1][0][k].item() > 0 for k in seen[1][0])            # counts (0, cap): the dn losses are sample 1's
    assert cap_step.captures == 1 and {n: g.data_ptr() for n, g in cap_step.grads.items()} == ptrs
    assert all(p.grad is cap_step.grads[n] for n, p in head.named_parameters() if p.requires_grad)
    # a batch above the capacity is refused before anything is enqueued
    over_b, over_l = C.make_gt((6, 1), 10, 5)
    with pytest.raises(ValueError, match='capacity'):
        cap_step.replay(over_b, over_l)
    # the feature-gradient mode of the capture is the only one replayed
    from sparsebev_amd import ops
    if not torch.are_deterministic_algorithms_enabled():
        prev = ops.deterministic_feature_grad(not cap_step.det_feat_grad)
        try:
            with pytest.raises(RuntimeError, match='deterministic feature gradient'):
                cap_step.replay(boxes_a, labels_a)
        finally:
            ops.deterministic_feature_grad(prev)
    # refusals at construction: a second rank, a head without a capacity, the host solver with a capacity
    import torch.distributed as dist
    with monkeypatch.context() as mp:
        mp.setattr(dist, 'is_initialized', lambda: True)
        mp.setattr(dist, 'get_world_size', lambda *a, **k: 2)
        with torch.enable_grad(), pytest.raises(RuntimeError, match='2 ranks'):
            CapturedHeadTrainStep(twin, static, metas_a)
    with torch.enable_grad(), pytest.raises(ValueError, match='gt_capacity'):
        CapturedHeadTrainStep(make(state, N), static, metas_a)
    with pytest.raises(ValueError, match="assign_on='device'"):
        T.make_head(assign_on='host', gt_capacity=CAP)


def test_captured_head_step_dropout_word():
    from sparsebev_amd.train_graph import CapturedHeadTrainStep
    CAP, N = 5, 2
    state, feats, metas, boxes, labels = setup((5, 3))
    head = make(state, N, dropout=True, gt_capacity=CAP)
    with torch.enable_grad():
        cap_step = CapturedHeadTrainStep(head, [f.clone() for f in feats], metas, warmup=1)
    assert cap_step.dropout and cap_step.seed_dev is not None and cap_step.captures == 1
    runs = []
    for new_masks in (False, False, True):
        losses = cap_step.replay(boxes, labels, metas, new_masks=new_masks, noise=False)
        torch.cuda.synchronize()
        runs.append(({k: v.clone() for k, v in losses.items()}, {n: g.clone() for n, g in cap_step.grads.items()}))
    assert_same(runs[1][0], runs[0][0], 'loss, same dropout word')
    assert_same(runs[1][1], runs[0][1], 'gradient, same dropout word')
    assert any(not torch.equal(runs[2][0][k], runs[0][0][k]) for k in runs[0][0])     # a new word: other masks


def test_split_k_workspace_belongs_to_the_capture():
    """dense._ws hands a capture a workspace from the capture's own pool: the shared one is replaced when a larger call comes along
    (two captured steps of different capacity in one process), and a graph must not be left pointing at it."""
    from sparsebev_amd import dense
    dev = torch.device(DEV)
    shared = dense._ws(4096, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        inside = dense._ws(4096, dev)
        inside.zero_()
    assert inside.numel() * 4 >= 4096 and inside.data_ptr() != shared.data_ptr()
    assert dense._ws(4096, dev) is shared
