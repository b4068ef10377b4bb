"""The box decode (csrc/head.hip, sbev_nms_free_decode) at every instantiation and edge its dispatch can reach: the four bitonic sort
widths with and without padding keys, max_num up to the limit of 1024 with kept boxes in every one of the 16 waves, the 'v0.17.1' box
layout, non-finite and signed-zero logits, and the strict / non-strict edges of the two masks.

The reference is torch on the CPU, written out from models/bbox/coders/nms_free_coder.py:49-79 (tests/head_cases.py); the logits are a
seeded permutation of an evenly spaced grid, so that every score is distinct and torch.topk's order is the only right one
(tests/test_head_edges_host.py asserts that on the CPU).  Tolerances are those of tests/test_gpu_head.py: labels, box index, count and
the copied columns exact; scores 1e-6; exp columns 1e-6 relative; atan2 1e-6; bottom-centre z 2e-5."""
import ctypes
import math

import numpy as np
import pytest
import torch

import head_cases as HC
from oracle import sparsebev_oracle as O
from sparsebev_amd import _lib, synthetic as S
from sparsebev_amd import head as H
from sparsebev_amd.utils import VERSION

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POST = HC.POST


def decode(cls, box, NC, max_num, thr, bottom=False):
    """The padded device outputs on the CPU: boxes [B, max_num, 9], scores, labels, count."""
    return [t.cpu() for t in H.nms_free_decode(cls.to(DEV), box.to(DEV), NC, max_num, thr, POST, bottom)]


def check_sample(out, i, ref, what=''):
    """Sample i of the padded outputs against (boxes, scores, labels, bbox_index) of the CPU reference."""
    boxes, scores, labels, count = out
    rb, rs, rl, ri = ref
    k = int(count[i])
    assert k == rb.shape[0], (what, k, rb.shape[0])
    assert not boxes[i, k:].any() and not scores[i, k:].any() and not labels[i, k:].any(), what      # rows past the count are zero
    if k == 0:
        return
    got = boxes[i, :k]
    assert torch.equal(labels[i, :k].long(), rl), what
    assert torch.equal(got[:, 7].long(), ri), what                                       # vx carries the query index
    assert torch.equal(got[:, [0, 1, 2, 7, 8]], rb[:, [0, 1, 2, 7, 8]]), what            # copied columns: bit-identical
    assert (scores[i, :k] - rs).abs().max() < 1e-6, what
    assert ((got[:, 3:6] - rb[:, 3:6]).abs() / rb[:, 3:6]).max() < 1e-6, what            # exp
    assert (got[:, 6] - rb[:, 6]).abs().max() < 1e-6, what                               # atan2


@pytest.mark.parametrize('Q,NC', HC.SORT_SHAPES, ids=['n%d-sort%d' % (q * c, HC.sort_width(q * c)) for q, c in HC.SORT_SHAPES])
def test_decode_every_sort_width_vs_torch_topk(Q, NC):
    """n = Q * num_classes at, one below and one above each padded width: no padding key, one, and the next kernel."""
    n, B = Q * NC, 2
    cls = torch.stack([HC.distinct_logits(Q, NC, 1000 * b + Q + NC) for b in range(B)])
    box = torch.stack([HC.random_boxes(Q, 77 * b + Q) for b in range(B)])
    max_num = min(n, 777)
    for thr in (None, 0.9):
        out = decode(cls, box, NC, max_num, thr)
        for b in range(B):
            ref = HC.ref_decode_single(cls[b], box[b], NC, max_num, thr)
            check_sample(out, b, ref, 'n=%d sample %d thr=%s' % (n, b, thr))
        print('sort width %d: n = %d = %d x %d, max_num %d, thr %s: kept %s' % (HC.sort_width(n), n, Q, NC, max_num, thr, out[3].tolist()))
    assert n == 1 or 0 < int(out[3][0]) < max_num                                        # the masks decided something


def test_decode_refuses_what_does_not_fit_and_launches_nothing():
    """n = 16385 and max_num = 1025 are refused with the library's own messages, the output buffers untouched."""
    lim = (ctypes.c_double * 6)(*POST)
    for Q, NC, max_num, msg in ((3277, 5, 100, r'Q \* num_classes = 16385 > 16384'), (2048, 8, 1025, r'max_num 1025 > 1024')):
        cls = HC.distinct_logits(Q, NC, 1)[None].to(DEV)
        box = HC.random_boxes(Q, 2)[None].to(DEV)
        with pytest.raises(RuntimeError, match=msg):
            H.nms_free_decode(cls, box, NC, max_num, None, POST)
        outs = [torch.full((1, max_num, 9), 7.0, device=DEV), torch.full((1, max_num), 7.0, device=DEV),
                torch.full((1, max_num), 7, device=DEV, dtype=torch.int32), torch.full((1,), 7, device=DEV, dtype=torch.int32)]
        st = _lib.load().sbev_nms_free_decode(H._p(cls), H._p(box), 1, Q, NC, max_num, 0.0, 0, lim, 0, *[H._p(t) for t in outs], H._stream())
        torch.cuda.synchronize()
        assert st != 0 and all(bool((t == 7).all()) for t in outs)


@pytest.mark.parametrize('max_num', HC.MAX_NUMS, ids=['max_num%d' % m for m in HC.MAX_NUMS])
@pytest.mark.parametrize('Q,NC', HC.COMPACT_SHAPES, ids=['n%d-sort%d' % (q * c, HC.sort_width(q * c)) for q, c in HC.COMPACT_SHAPES])
def test_decode_max_num_and_compaction_by_rank(Q, NC, max_num):
    """The ballot + prefix-sum compaction over all 16 waves: the centre-range mask is decided through cx so that exactly the named RANKS
    survive -- all, none, every third, only the last, only ranks >= 960 (the last wave).  Sample 1 carries the next pattern and other
    logits: its rows must not depend on sample 0's count."""
    shots = [HC.distinct_query_logits(Q, NC, 31 * b + Q + max_num) for b in range(2)]
    cls = torch.stack([s[0] for s in shots])
    for i, pattern in enumerate(HC.PATTERNS):
        pats = [pattern, HC.PATTERNS[(i + 1) % len(HC.PATTERNS)]]
        box = torch.stack([HC.boxes_for_pattern(Q, shots[b][1], pats[b], max_num, 5 + b) for b in range(2)])
        out = decode(cls, box, NC, max_num, None)
        for b in range(2):
            want = [r for r in range(max_num) if HC.keep_rank(pats[b], r, max_num)]
            assert int(out[3][b]) == len(want), (pats, b)
            assert out[0][b, :len(want), 7].long().tolist() == shots[b][1][want].tolist(), (pats, b)      # the kept ranks, in rank order
            check_sample(out, b, HC.ref_decode_single(cls[b], box[b], NC, max_num, None), 'max_num=%d %s sample %d' % (max_num, pats[b], b))
        if pattern == 'none':
            assert int(out[3][0]) == 0 and not out[0][0].any() and not out[1][0].any() and not out[2][0].any()
    # the same through a score threshold that cuts inside the top-k: kept = a prefix of the ranks
    box = torch.stack([HC.boxes_for_pattern(Q, shots[b][1], 'all', max_num, 5 + b) for b in range(2)])
    top = cls[0].sigmoid().view(-1).topk(max_num).values.double()
    half = max_num // 2                                                # halfway between two ranks' scores: 15 ulps from either
    thr = float((top[half - 1] + top[half]) / 2) if half else 0.999
    out = decode(cls, box, NC, max_num, thr)
    assert int(out[3][0]) == half
    for b in range(2):
        check_sample(out, b, HC.ref_decode_single(cls[b], box[b], NC, max_num, thr), 'thr sample %d' % b)


def test_get_bboxes_old_box_convention_v0_17_1():
    """bottom == 2 in the kernel: SparseBEVHead.get_bboxes under VERSION.name = 'v0.17.1' (models/sparsebev_head.py:472-476: w / l swapped,
    yaw = -yaw - pi / 2) against the oracle under the same switch, and against the same inputs under 'v1.0.0'."""
    Q, NC, B, max_num = 100, 7, 2, 60
    head = H.SparseBEVHead(num_classes=NC, in_channels=256, num_query=Q, code_size=10,
                           transformer=dict(type='SparseBEVTransformer', embed_dims=256, num_frames=2, num_points=4, num_layers=1,
                                            num_levels=4, num_classes=NC, code_size=10, pc_range=S.PC_RANGE),
                           bbox_coder=dict(type='NMSFreeCoder', post_center_range=POST, max_num=max_num, score_threshold=0.3,
                                           num_classes=NC, pc_range=S.PC_RANGE))
    cls = torch.stack([HC.distinct_logits(Q, NC, 40 + b) for b in range(B)])
    box = torch.stack([HC.random_boxes(Q, 50 + b) for b in range(B)])
    preds = {'all_cls_scores': cls[None].to(DEV), 'all_bbox_preds': box[None].to(DEV)}
    try:
        VERSION.name = O.VERSION_NAME = 'v0.17.1'
        old = [[t.cpu() for t in r] for r in head.get_bboxes(preds)]
        also = head.bbox_coder._decode(preds, True)
        ref = O.get_bboxes(O.nms_free_decode(cls[None], box[None], NC, max_num, 0.3, POST))
        VERSION.name = O.VERSION_NAME = 'v1.0.0'
        new = [[t.cpu() for t in r] for r in head.get_bboxes(preds)]
        ref_new = O.get_bboxes(O.nms_free_decode(cls[None], box[None], NC, max_num, 0.3, POST))
    finally:
        VERSION.name = O.VERSION_NAME = 'v1.0.0'
    for b in range(B):
        (ob, os_, ol), (nb, ns, nl), (rb, rs, rl), (qb, _, _) = old[b], new[b], ref[b], ref_new[b]
        assert 0 < ob.shape[0] < max_num and torch.equal(ol, rl) and torch.equal(nl, rl) and ol.dtype == torch.long
        assert torch.equal(also[b]['bboxes'].cpu(), ob)                                 # _decode(..., True) is the same launch
        assert (os_ - rs).abs().max() < 1e-6 and torch.equal(os_, ns)
        assert torch.equal(ob[:, 3], nb[:, 4]) and torch.equal(ob[:, 4], nb[:, 3])      # the swap moves bits
        assert not torch.equal(ob[:, 3], nb[:, 3])
        assert ((ob[:, 3:6] - rb[:, 3:6]).abs() / rb[:, 3:6]).max() < 1e-6
        assert (ob[:, 6] - rb[:, 6]).abs().max() < 1e-6                                  # yaw = -atan2 - pi / 2
        assert (ob[:, 6] - (-nb[:, 6] - math.pi / 2)).abs().max() < 1e-6
        assert (ob[:, 6] - nb[:, 6]).abs().max() > 1e-3                                  # ... which is another angle
        assert (ob[:, 2] - rb[:, 2]).abs().max() < 2e-5 and torch.equal(ob[:, 2], nb[:, 2])          # bottom-centre z: both layouts
        assert torch.equal(ob[:, [0, 1, 7, 8]], rb[:, [0, 1, 7, 8]])
        assert (nb - qb).abs().max() < 2e-5
    print("box convention 'v0.17.1' (bottom == 2) and 'v1.0.0' ran: kept %s of %d" % ([r[0].shape[0] for r in old], max_num))


def special_row():
    """[8, 4] logits: the grid (no value is 0, none repeats) with the special values planted.  Returns (logits, the required order)."""
    cls = HC.distinct_logits(8, 4, 3)
    flat = cls.view(-1)
    flat[[25, 2, 20]] = HC.f32_bits(HC.NAN_SET, HC.NAN_SET, HC.NAN_CLEAR)
    assert flat[[2, 25]].view(torch.int32).tolist() == [-0x400000, -0x400000] and flat[20:21].view(torch.int32).item() == 0x7fc00000
    flat[9], flat[30] = float('inf'), -float('inf')
    flat[3], flat[5], flat[16] = -0.0, 0.0, -0.0                      # one logit, one score (0.5): flat index decides
    assert flat[[3, 16]].view(torch.int32).tolist() == [-2 ** 31] * 2
    flat[14], flat[11] = 2.5, 2.5                                     # equal reals: flat index decides
    real = [i for i in range(32) if i not in (2, 20, 25)]
    order = [2, 20, 25] + sorted(real, key=lambda i: (-float(flat[i]), i))            # -(-0.0) == -(0.0) in Python: a tie
    assert order[3] == 9 and order[-1] == 30 and order.index(11) + 1 == order.index(14)
    assert [i for i in order if i in (3, 5, 16)] == [3, 5, 16] and order.index(16) == order.index(3) + 2
    return cls, order


def test_decode_special_logits_nan_of_either_sign_first():
    """+inf, -inf, +0, -0, a sign-clear and two sign-set NaNs and a repeated real in one row.  Required: every NaN before +inf, NaNs among
    themselves by flat index, then the reals in descending order, equal logits (-0 == +0 included) by flat index.  A NaN cx is dropped
    by the range mask, a NaN score by a threshold.  (Before the fix in desc_key a sign-set NaN, 0xffc00000 -- what inf - inf gives --
    sorted LAST, and -0 behind every +0.)"""
    NC = 4
    cls, order = special_row()
    box = HC.random_boxes(8, 4, spread=10.0)
    plain = HC.distinct_logits(8, 4, 8)
    both = torch.stack([cls, plain])
    boxes = torch.stack([box, HC.random_boxes(8, 9, spread=10.0)])
    out = decode(both, boxes, NC, 32, None)
    assert int(out[3][0]) == 32
    got = (out[0][0, :, 7].long() * NC + out[2][0].long()).tolist()
    assert got[:3] == [2, 20, 25], got                                # NaNs first, by flat index, whatever their sign bit
    assert got == order, got
    want_s = cls.view(-1)[order].sigmoid()
    assert torch.isnan(out[1][0, :3]).all() and (out[1][0, 3:] - want_s[3:]).abs().max() < 1e-6
    assert out[1][0, 3].item() == 1.0 and out[1][0, 31].item() == 0.0                   # +inf, -inf
    assert [out[1][0, order.index(i)].item() for i in (3, 5, 16)] == [0.5] * 3          # a logit of +-0: exactly 0.5
    # the oracle (NaN-first since this change) agrees, and sample 1 (no special value) with torch.topk
    d = O.nms_free_decode_single(cls, box, NC, 32, None, POST)
    assert (d['bboxes'][:, 7].long() * NC + d['labels']).tolist() == got
    check_sample(out, 1, HC.ref_decode_single(plain, boxes[1], NC, 32, None))
    # max_num below n: the NaNs take the first places
    out = decode(both, boxes, NC, 5, None)
    assert (out[0][0, :, 7].long() * NC + out[2][0].long()).tolist() == order[:5]
    # a NaN cx is dropped by the range mask (every comparison with it is false)
    nbox = boxes.clone()
    nbox[0, 6, 0] = float('nan')
    out = decode(both, nbox, NC, 32, None)
    keep = [i for i in order if i // NC != 6]
    assert int(out[3][0]) == 28 and (out[0][0, :28, 7].long() * NC + out[2][0, :28].long()).tolist() == keep
    assert not torch.isnan(out[0][0]).any() and not out[0][0, 28:].any()
    # a NaN score is dropped by a threshold; 0.5 is strict (the three zeros go), the float below 0.5 keeps them
    out = decode(both, boxes, NC, 32, 0.5)
    keep = [i for i in order[3:] if float(cls.view(-1)[i]) > 0]
    assert (out[0][0, :int(out[3][0]), 7].long() * NC + out[2][0, :int(out[3][0])].long()).tolist() == keep and len(keep) > 3
    assert not torch.isnan(out[1][0]).any()
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    out = decode(both, boxes, NC, 32, below)
    assert (out[0][0, :int(out[3][0]), 7].long() * NC + out[2][0, :int(out[3][0])].long()).tolist() == keep + [3, 5, 16]
    check_sample(out, 1, HC.ref_decode_single(plain, boxes[1], NC, 32, below))


def test_decode_mask_edges_are_the_reference_comparisons():
    """>= / <= on the centre range, strict > on the score: a centre exactly on float32(+-61.2) (or +-10 in z) is kept, the next float outside is
    dropped; a score of exactly 0.5 is dropped at threshold 0.5 and kept at the float below."""
    f = np.float32
    hi, lo, zhi, zlo = f(61.2), f(-61.2), f(10.0), f(-10.0)
    cx = [hi, np.nextafter(hi, f(np.inf)), lo, np.nextafter(lo, f(-np.inf)), 0, 0, 0, 0, 0, 0, 0, 0]
    cy = [0, 0, 0, 0, hi, np.nextafter(hi, f(np.inf)), lo, np.nextafter(lo, f(-np.inf)), 0, 0, 0, 0]
    cz = [0, 0, 0, 0, 0, 0, 0, 0, zhi, np.nextafter(zhi, f(np.inf)), zlo, np.nextafter(zlo, f(-np.inf))]
    Q, NC = 12, 3
    box = HC.random_boxes(Q, 1, spread=10.0)
    box[:, 0], box[:, 1], box[:, 4] = torch.tensor(np.array(cx, f)), torch.tensor(np.array(cy, f)), torch.tensor(np.array(cz, f))
    cls = HC.distinct_logits(Q, NC, 2)[None]
    out = decode(cls, box[None], NC, Q * NC, None)
    ref = HC.ref_decode_single(cls[0], box, NC, Q * NC, None)
    check_sample(out, 0, ref)
    assert sorted(set(out[0][0, :int(out[3][0]), 7].long().tolist())) == [0, 2, 4, 6, 8, 10] and int(out[3][0]) == 18
    # the score edge, every class of query 0 at logit 0
    cls = HC.distinct_logits(Q, NC, 2)
    cls[0] = 0.0
    box = HC.random_boxes(Q, 1, spread=10.0)
    n_above = int((cls > 0).sum())
    for thr, kept in ((0.5, n_above), (float(np.nextafter(f(0.5), f(0))), n_above + NC)):
        out = decode(cls[None], box[None], NC, Q * NC, thr)
        assert int(out[3][0]) == kept, (thr, int(out[3][0]))
        # (three equal scores: torch.topk may order them otherwise, the oracle's order is score desc, flat index asc)
        d = O.nms_free_decode_single(cls, box, NC, Q * NC, thr, POST)
        assert torch.equal(out[2][0, :kept].long(), d['labels']) and torch.equal(out[0][0, :kept, 7], d['bboxes'][:, 7])
        assert (out[1][0, :kept] - d['scores']).abs().max() < 1e-6
