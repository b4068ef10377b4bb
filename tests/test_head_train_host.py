"""CPU-side checks of the training head: the library's host linear-sum-assignment solver, the fixture G15 against the
independent restatement (tests/head_train_cases.py), and the class contract of SparseBEVTrainHead."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import head_train_cases as C
from conftest import load_golden
from sparsebev_amd import _lib, synthetic as S
from sparsebev_amd import head_train as HT

POST = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]


def total(cost, col):
    return float(sum(np.float64(cost[i, c]) for i, c in enumerate(col) if c >= 0))


def check_valid(cost, col):
    n, m = cost.shape
    used = [c for c in col if c >= 0]
    assert len(used) == min(n, m) and len(set(used)) == len(used) and all(0 <= c < m for c in used)


# ---- host solver ------------------------------------------------------------------------------------------------------------

def test_solver_vs_brute_force_all_small_shapes():
    """All shapes with rows, cols <= 6, continuous and small-integer (tie-rich) costs: a valid matching of min(n, m) pairs whose total
    equals the enumerated minimum (on ties the pairs may differ, the total may not)."""
    rng = np.random.default_rng(5)
    for n, m in itertools.product(range(1, 7), repeat=2):
        for kind in ('continuous', 'integer'):
            cost = (rng.standard_normal((n, m)) * 3 if kind == 'continuous' else rng.integers(0, 4, (n, m))).astype(np.float32)
            col = HT.lsa_solve(cost)
            check_valid(cost, col)
            assert abs(total(cost, col) - C.brute_force_total(cost)) <= 1e-9 * max(1.0, abs(C.brute_force_total(cost))), (n, m, kind)
            ref = C.solve(cost)                                         # the restatement's own solver agrees on the total as well
            assert abs(total(cost, ref) - total(cost, col)) <= 1e-9 * max(1.0, abs(total(cost, col)))


@pytest.mark.parametrize('n,m', [(36, 5), (900, 40), (36, 40), (1, 1), (7, 0), (0, 7)])
def test_solver_vs_scipy(n, m):
    so = pytest.importorskip('scipy.optimize')
    rng = np.random.default_rng(n * 100 + m)
    cost = (rng.standard_normal((n, m)) * 2).astype(np.float32)
    col = HT.lsa_solve(cost)
    assert col.shape == (n,) and col.dtype == np.int32
    if n == 0 or m == 0:
        assert (col == -1).all()
        return
    check_valid(cost, col)
    rr, cc = so.linear_sum_assignment(cost.astype(np.float64))
    ref = float(cost.astype(np.float64)[rr, cc].sum())
    assert abs(total(cost, col) - ref) <= 1e-9 * max(1.0, abs(ref))
    # a cost column of all 100s (a gt with a NaN velocity, hungarian_assigner_3d.py:74)
    if m > 1:
        cost[:, m // 2] = 100.0
        col = HT.lsa_solve(cost)
        check_valid(cost, col)
        rr, cc = so.linear_sum_assignment(cost.astype(np.float64))
        ref = float(cost.astype(np.float64)[rr, cc].sum())
        assert abs(total(cost, col) - ref) <= 1e-9 * max(1.0, abs(ref))


def test_solver_status_and_leading_dimension():
    lib = _lib.load()
    cost = np.arange(12, dtype=np.float32).reshape(3, 4)
    out = np.zeros(3, dtype=np.int32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert lib.sbev_lsa_solve(vp(cost), 4, 3, 4, vp(out)) == 0
    assert lib.sbev_lsa_solve(vp(cost), 3, 3, 4, vp(out)) == -1 and b'leading dimension' in lib.sbev_last_error()
    bad = cost.copy()
    bad[1, 2] = np.nan
    assert lib.sbev_lsa_solve(vp(bad), 4, 3, 4, vp(out)) == -1 and b'not finite' in lib.sbev_last_error()
    bad[1, 2] = np.inf
    assert lib.sbev_lsa_solve(vp(bad), 4, 3, 4, vp(out)) == -1
    with pytest.raises(_lib.SbevError):
        HT.lsa_solve(bad)
    # a leading dimension above n_cols: the columns behind n_cols are not read (they hold NaN here)
    wide = np.full((3, 6), np.nan, dtype=np.float32)
    wide[:, :4] = cost
    assert np.array_equal(HT.lsa_solve(wide[:, :4]), HT.lsa_solve(cost))
    # the step's table: per layer and sample, -1 = background
    c = np.zeros((2, 2, 3, 2), dtype=np.float32)
    c[..., 0] = [3, 1, 2]
    c[..., 1] = [1, 5, 5]
    counts = np.array([2, 0], dtype=np.int32)
    table = np.full((2, 2, 3), 7, dtype=np.int32)
    assert lib.sbev_head_assign(vp(c), vp(counts), 2, 2, 3, 2, vp(table)) == 0
    assert table[:, 0].tolist() == [[1, 0, -1]] * 2 and (table[:, 1] == -1).all()
    counts[1] = 3
    assert lib.sbev_head_assign(vp(c), vp(counts), 2, 2, 3, 2, vp(table)) == -1 and b'gt_counts[1]' in lib.sbev_last_error()


# ---- fixture sanity -------------------------------------------------------------------------------------------------------

def close(got, ref, tol=1e-6):
    """|got - ref| <= 1e-6 * max(1, |ref|).  Up to magnitude 1 (normalised xyz, sin, cos, the indicator) that is the absolute 1e-6 asked
    for.  Above 1 it has to be relative: the recording is fp32, so a value v carries a rounding of up to 2^-24 * |v| of its own --
    1.2e-5 at the largest recorded loss (196.5), 3e-6 at a 50 m centre -- which no fp64 restatement can come closer to."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    ok = ~torch.isnan(ref)
    return bool(((got[ok] - ref[ok]).abs() <= tol * ref[ok].abs().clamp_min(1.0)).all())


@pytest.mark.parametrize('tag', C.FIXTURE_CASES)
def test_restatement_reproduces_the_fixture(tag):
    """fp64 restatement vs the reference's fp32 recording: integers equal, floats within 1e-6 of max(1, |ref|)."""
    c = C.fixture_case(load_golden('g15_head_train'), tag)
    r = C.dn_prepare(c['init_w'].double(), c['label_w'].double(), c['boxes'], c['labels'], (c['u_box'].double(), c['u_lab'], c['new_lab']),
                     c['N'], c['NC'])
    assert r['pad_size'] == c['pad']
    for k in ('known_indice', 'batch_idx', 'map_known_indice', 'known_labels'):
        assert torch.equal(r[k], c[k].long()), k
    assert torch.equal(r['attn_mask'], c['attn_mask'])
    assert close(r['query_bbox'], c['query_bbox']) and close(r['query_feat'], c['query_feat']) and close(r['known_bboxs'], c['known_bboxs'])
    pad, cw = c['pad'], torch.tensor(C.CODE_WEIGHTS, dtype=torch.float64)
    cls, box = c['cls'].double(), c['box'].double()
    a = C.assign(cls[:, :, pad:], box[:, :, pad:], c['boxes'], c['labels'], cw)
    assert torch.equal(a, c['assign'].long())
    if pad:
        codes = C.dn_codes(c['counts'], c['N'])
        sel = (codes >= 0)
        # prepare_for_dn_loss's gather [L, num_tgt, *] in known-query order (group-major) = the rows the codes select, sample-major
        got = [cls[:, b, :pad][:, sel[b]] for b in range(len(c['counts']))]                      # per sample [L, N * g_b, NC]
        order = torch.cat([torch.nonzero(c['batch_idx'].long().repeat(c['N']) == b).reshape(-1) for b in range(len(c['counts']))])
        assert torch.equal(torch.cat(got, dim=1).float(), c['dn_gather_cls'][:, order])
        assert int(c['num_tgt']) == c['N'] * sum(c['counts'])
    d = C.loss_dict(cls[:, :, pad:], box[:, :, pad:], cls[:, :, :pad] if pad else None, box[:, :, :pad] if pad else None,
                    c['boxes'], c['labels'], cw, c['N'])
    assert sorted(d) == [str(k) for k in c['loss_keys']]
    assert close(torch.stack([d[str(k)] for k in c['loss_keys']]), c['loss_values'])
    if tag == 'a':
        assert float(c['margin']) >= 1e-3 and torch.isnan(c['gt_boxes']).any()
    if tag == 'c':
        assert not any(k.endswith('_dn') for k in d)


# ---- class contract -------------------------------------------------------------------------------------------------------

def make_head(cls=None, **kw):
    cls = cls or HT.SparseBEVTrainHead
    return cls(num_classes=10, in_channels=256, num_query=36, code_size=10, code_weights=C.CODE_WEIGHTS,
               transformer=dict(type='SparseBEVTransformer', embed_dims=256, num_frames=2, num_points=4, num_layers=2, num_levels=4,
                                num_classes=10, code_size=10, pc_range=S.PC_RANGE),
               bbox_coder=dict(type='NMSFreeCoder', post_center_range=POST, max_num=30, score_threshold=None, num_classes=10,
                               pc_range=S.PC_RANGE), **kw)


CONFIG = dict(loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=2.0),
              loss_bbox=dict(type='L1Loss', loss_weight=0.25), loss_iou=dict(type='GIoULoss', loss_weight=0.0), sync_cls_avg_factor=True,
              train_cfg=dict(pts=dict(assigner=dict(type='HungarianAssigner3D', cls_cost=dict(type='FocalLossCost', weight=2.0),
                                                    reg_cost=dict(type='BBox3DL1Cost', weight=0.25), iou_cost=dict(type='IoUCost', weight=0.0)))))


def test_train_head_class_contract():
    import sparsebev_amd
    from sparsebev_amd.head import SparseBEVHead
    assert sparsebev_amd.SparseBEVTrainHead is HT.SparseBEVTrainHead and issubclass(HT.SparseBEVTrainHead, SparseBEVHead)
    head, base = make_head(**CONFIG), make_head(SparseBEVHead)
    assert len(head.state_dict()) == 51 and set(head.state_dict()) == set(base.state_dict())
    head.load_state_dict(base.state_dict(), strict=True)
    base.load_state_dict(head.state_dict(), strict=True)
    assert (head.loss_cls_weight, head.focal_gamma, head.focal_alpha, head.loss_bbox_weight) == (2.0, 2.0, 0.25, 0.25)
    assert (head.cls_cost_weight, head.reg_cost_weight, head.bg_cls_weight) == (2.0, 0.25, 0.0)
    assert (head.dn_weight, head.dn_bbox_noise_scale, head.dn_label_noise_scale, head.dn_group_num) == (1.0, 0.5, 0.5, 10)
    plain = make_head()                                                 # the defaults are the config's values
    assert (plain.loss_cls_weight, plain.loss_bbox_weight, plain.cls_cost_weight, plain.reg_cost_weight) == (2.0, 0.25, 2.0, 0.25)
    # CPU tensors: no fallback
    boxes, labels = C.make_gt((2,), 10, 3)
    metas = [dict(m, gt_bboxes_3d=boxes[0], gt_labels_3d=labels[0]) for m in S.make_img_metas(1, 2, 64, 176)]
    with pytest.raises(RuntimeError, match='no CPU path'):
        head.train()(S.make_features(1, 2, S.PYRAMIDS['tiny'][2]), metas)
    with pytest.raises(RuntimeError, match='no CPU path'):
        preds = {'all_cls_scores': torch.zeros(2, 1, 36, 10), 'all_bbox_preds': torch.zeros(2, 1, 36, 10)}
        head.loss(boxes, labels, preds)
    with pytest.raises(ValueError):
        HT.GroundTruth([torch.zeros(2, 7)], [torch.zeros(2)], 'cpu')
    # a copy or a pickle of the module carries no staging state of the assigner
    import copy
    import pickle
    assert copy.deepcopy(head)._assigner is not head._assigner and pickle.loads(pickle.dumps(head._assigner))._cost is None


@pytest.mark.parametrize('kw', [
    dict(loss_cls=dict(type='CrossEntropyLoss')), dict(loss_cls=dict(type='FocalLoss', use_sigmoid=False)),
    dict(loss_bbox=dict(type='SmoothL1Loss')), dict(loss_iou=dict(type='GIoULoss', loss_weight=2.0)), dict(loss_iou=dict(type='IoULoss', loss_weight=0.0)),
    dict(train_cfg=dict(assigner=dict(type='HungarianAssigner3D', cls_cost=dict(type='ClassificationCost', weight=1.0)))),
    dict(train_cfg=dict(assigner=dict(type='HungarianAssigner3D', reg_cost=dict(type='BBoxL1Cost', weight=1.0)))),
    dict(train_cfg=dict(pts=dict(assigner=dict(type='HungarianAssigner3D', iou_cost=dict(type='IoUCost', weight=1.0))))),
    dict(train_cfg=dict(assigner=dict(type='MaxIoUAssigner'))),
])
def test_train_head_refuses_unsupported_losses_and_costs(kw):
    with pytest.raises(ValueError):
        make_head(**kw)
