"""Inputs and the CPU reference of the box-decode edge tests (tests/test_gpu_head_edges.py on the device,
tests/test_head_edges_host.py for the conditions that can be checked without one).

The reference is torch on the CPU, written out from the reference coder (models/bbox/coders/nms_free_coder.py:49-79):
sigmoid, ``view(-1).topk(max_num)``, ``% num_classes``, ``div(..., rounding_mode='trunc')``, denormalize_bbox, the two
masks, boolean indexing.  ``topk`` is only well defined for pairwise distinct scores, so the logits are a seeded
permutation of an evenly spaced grid on [-6, 6]: at 16384 values the smallest fp32 score gap is about 1.8e-6 (the grid
step 7.3e-4 times sigmoid'(6) = 2.5e-3) against an ulp of 6e-8 below 1."""
import numpy as np
import torch

POST = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]

# (Q, num_classes) per n = Q * num_classes, and the bitonic sort width n pads to (csrc/head.hip: 2048, 4096, 8192, 16384)
SORT_SHAPES = [(1, 1), (89, 23), (256, 8), (683, 3), (315, 13), (1024, 4), (241, 17), (8191, 1), (128, 64), (2731, 3), (381, 43), (2048, 8)]
SORT_NS = [1, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384]
assert [q * c for q, c in SORT_SHAPES] == SORT_NS

# max_num / compaction cases: one n per sort width, Q >= 1024 so that the first 1024 ranks can sit in distinct queries
COMPACT_SHAPES = [(1024, 2), (1365, 3), (1170, 7), (1489, 11)]          # n = 2048 (no padding key), 4095, 8190, 16379
MAX_NUMS = [1, 63, 64, 65, 1023, 1024]
PATTERNS = ['all', 'none', 'third', 'last', 'tail']                    # which RANKS pass the centre-range mask


def sort_width(n):
    return next(w for w in (2048, 4096, 8192, 16384) if n <= w)


def grid_logits(n, descending=False):
    v = torch.linspace(-6.0, 6.0, n, dtype=torch.float64).float()
    return v.flip(0) if descending else v


def distinct_logits(Q, NC, seed):
    """[Q, NC] logits: a seeded permutation of the grid."""
    g = torch.Generator().manual_seed(seed)
    n = Q * NC
    return grid_logits(n)[torch.randperm(n, generator=g)].reshape(Q, NC)


def distinct_query_logits(Q, NC, seed):
    """A seeded permutation of the grid whose Q largest values sit in Q different queries (one class each, drawn at random):
    rank r < Q of the top-k is query ``rank_query[r]``, so a centre-range decision per QUERY is a decision per RANK.
    Returns (logits [Q, NC], rank_query [Q])."""
    g = torch.Generator().manual_seed(seed)
    n = Q * NC
    vals = grid_logits(n, descending=True)
    rank_query = torch.randperm(Q, generator=g)
    top = rank_query * NC + torch.randint(0, NC, (Q,), generator=g)
    flat = torch.empty(n)
    flat[top] = vals[:Q]
    rest = torch.ones(n, dtype=torch.bool)
    rest[top] = False
    rest = rest.nonzero()[:, 0]
    flat[rest[torch.randperm(rest.numel(), generator=g)]] = vals[Q:]
    return flat.reshape(Q, NC), rank_query


def scores_distinct(logits):
    """The condition torch.topk needs: the fp32 sigmoid values are pairwise distinct."""
    s = logits.sigmoid().reshape(-1)
    return torch.unique(s).numel() == s.numel()


def random_boxes(Q, seed, spread=45.0):
    """[Q, 10] head-format boxes (cx, cy, w, l, cz, h, sin, cos, vx, vy): centres of which ~17 % fall outside +-61.2 m per axis with the
    default spread (with spread <= 10 every centre is inside, cz included), log sizes, an unnormalised (sin, cos) pair; vx carries the
    query index (a copied column: it names the gathered box)."""
    g = torch.Generator().manual_seed(seed)
    box = torch.randn(Q, 10, generator=g)
    box[:, 0:2] *= spread
    box[:, 2:4] *= 0.5
    box[:, 4] *= 3.0
    box[:, 5] *= 0.5
    box[:, 8] = torch.arange(Q).float()
    if spread <= 10.0:                    # "every centre inside": cz (3 sigma = 9 m) as well
        box[:, 4].clamp_(-9.5, 9.5)
    return box


def keep_rank(pattern, r, max_num):
    return {'all': True, 'none': False, 'third': r % 3 == 0, 'last': r == max_num - 1, 'tail': r >= 960}[pattern]


def boxes_for_pattern(Q, rank_query, pattern, max_num, seed):
    """Boxes whose centre-range mask, decided through cx alone, keeps exactly the ranks ``keep_rank`` names."""
    box = random_boxes(Q, seed, spread=10.0)                          # every centre well inside the range ...
    out = torch.tensor([not keep_rank(pattern, r, max_num) for r in range(max_num)])
    box[rank_query[:max_num][out], 0] = 70.0 + torch.arange(int(out.sum())).float()      # ... but the dropped ranks' cx
    return box


def denormalize(nb):
    """models/bbox/utils.py:26-47."""
    rot = torch.atan2(nb[..., 6:7], nb[..., 7:8])
    return torch.cat([nb[..., 0:2], nb[..., 4:5], nb[..., 2:4].exp(), nb[..., 5:6].exp(), rot, nb[..., 8:10]], dim=-1)


def ref_decode_single(cls, box, num_classes, max_num, score_threshold, post=POST):
    """nms_free_coder.py:49-79 on the CPU.  Returns boxes [k, 9], scores [k], labels [k], bbox_index [k] (all after the masks)."""
    s = cls.sigmoid()
    scores, indexs = s.view(-1).topk(max_num)
    labels = indexs % num_classes
    bbox_index = torch.div(indexs, num_classes, rounding_mode='trunc')
    boxes = denormalize(box[bbox_index])
    limit = torch.tensor(post)
    mask = (boxes[..., :3] >= limit[:3]).all(1)
    mask &= (boxes[..., :3] <= limit[3:]).all(1)
    if score_threshold:
        mask &= scores > score_threshold
    return boxes[mask], scores[mask], labels[mask], bbox_index[mask]


def f32_bits(*words):
    """fp32 values from their bit patterns (the two NaNs of the special-logit test cannot be written as literals)."""
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


NAN_CLEAR, NAN_SET = 0x7fc00000, 0xffc00000       # float('nan'); what inf - inf and 0 / 0 give on an x86 host


def plant_nans(logits, seed, count=6):
    """A copy of ``logits`` with ``count`` NaNs of alternating sign bit at seeded flat positions.  Returns (logits, positions)."""
    g = torch.Generator().manual_seed(seed)
    flat = logits.clone().reshape(-1)
    count = min(count, flat.numel())
    pos = torch.randperm(flat.numel(), generator=g)[:count]
    flat[pos] = f32_bits(*[NAN_SET if i % 2 == 0 else NAN_CLEAR for i in range(count)])
    return flat.reshape(logits.shape), pos.sort().values
