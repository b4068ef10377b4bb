"""CPU half of the box-decode edge tests: the conditions tests/test_gpu_head_edges.py rests on (pairwise distinct fp32 scores, ranks
that map to queries one to one) and the oracle's NaN-first top-k order against torch.topk."""
import pytest
import torch

import head_cases as HC
from oracle import sparsebev_oracle as O


@pytest.mark.parametrize('Q,NC', HC.SORT_SHAPES + HC.COMPACT_SHAPES)
def test_grid_logits_give_pairwise_distinct_fp32_scores(Q, NC):
    for seed in (0, 1):
        cls = HC.distinct_logits(Q, NC, 1000 * seed + Q + NC)
        assert HC.scores_distinct(cls)
        cls, _ = HC.distinct_query_logits(Q, NC, 1000 * seed + Q + NC)
        assert HC.scores_distinct(cls)
    s = HC.grid_logits(Q * NC).sigmoid()
    if s.numel() > 1:
        print('n = %d: smallest fp32 score gap %.2e' % (s.numel(), (s[1:] - s[:-1]).min().item()))
        assert (s[1:] - s[:-1]).min().item() > 4 * 6e-8            # several ulps, not one: the device's expf may differ by one


@pytest.mark.parametrize('Q,NC', HC.COMPACT_SHAPES)
def test_rank_patterns_keep_exactly_the_named_ranks(Q, NC):
    cls, rank_query = HC.distinct_query_logits(Q, NC, Q + NC)
    _, idx = cls.sigmoid().view(-1).topk(1024)
    assert torch.equal(torch.div(idx, NC, rounding_mode='trunc'), rank_query[:1024])
    for max_num in HC.MAX_NUMS:
        for pattern in HC.PATTERNS:
            box = HC.boxes_for_pattern(Q, rank_query, pattern, max_num, 7)
            _, _, _, bidx = HC.ref_decode_single(cls, box, NC, max_num, None)
            want = [r for r in range(max_num) if HC.keep_rank(pattern, r, max_num)]
            assert bidx.tolist() == rank_query[want].tolist(), (max_num, pattern)


@pytest.mark.parametrize('Q,NC', [(89, 23), (1024, 4), (241, 17), (2048, 8)])       # both of the oracle's sort paths (n <= 4096, n > 4096)
def test_oracle_topk_order_vs_torch_topk_with_nans(Q, NC):
    cls = HC.distinct_logits(Q, NC, 5 + Q)
    box = HC.random_boxes(Q, 6 + Q, spread=10.0)                       # every centre in range: the order is all that decides
    max_num = min(300, Q * NC)
    rb, rs, rl, ri = HC.ref_decode_single(cls, box, NC, max_num, None)
    d = O.nms_free_decode_single(cls, box, NC, max_num, None, HC.POST)
    assert torch.equal(d['labels'], rl) and torch.equal(d['scores'], rs) and torch.equal(d['bboxes'], rb)
    # NaNs of both sign bits: torch.topk ranks every NaN first (among themselves in no stated order), then the reals as before
    bad, pos = HC.plant_nans(cls, 9 + Q)
    bits = bad.reshape(-1)[pos].view(torch.int32)
    assert (bits < 0).any() and (bits > 0).any() and torch.isnan(bad.reshape(-1)[pos]).all()
    m = pos.numel()
    _, idx = bad.sigmoid().view(-1).topk(max_num)
    assert sorted(idx[:m].tolist()) == pos.tolist()
    d = O.nms_free_decode_single(bad, box, NC, max_num, None, HC.POST)
    got = d['bboxes'][:, 7].long() * NC + d['labels']                 # vx names the query
    assert got[:m].tolist() == pos.tolist()                            # NaNs first, by flat index
    assert torch.equal(got[m:], idx[m:])
    assert torch.isnan(d['scores'][:m]).all() and not torch.isnan(d['scores'][m:]).any()
    # with a threshold a NaN score is dropped (NaN > thr is false)
    d = O.nms_free_decode_single(bad, box, NC, max_num, 0.5, HC.POST)
    assert not torch.isnan(d['scores']).any() and d['scores'].numel() > 0


def test_oracle_orders_signed_zeros_and_infinities():
    """-0 and +0 are one logit (one score, 0.5): flat index decides, in both sort paths."""
    for Q, NC in ((4, 3), (2100, 2)):
        cls = torch.full((Q, NC), -3.0)
        flat = cls.view(-1)
        flat[1], flat[3], flat[5], flat[7], flat[8], flat[9] = -0.0, 0.0, float('inf'), 0.0, -float('inf'), 2.0
        flat[[2, 6]] = HC.f32_bits(HC.NAN_SET, HC.NAN_CLEAR)
        box = HC.random_boxes(Q, 3, spread=10.0)
        d = O.nms_free_decode_single(cls, box, NC, 8, None, HC.POST)
        got = d['bboxes'][:, 7].long() * NC + d['labels']
        assert got.tolist() == [2, 6, 5, 9, 1, 3, 7, 0]
