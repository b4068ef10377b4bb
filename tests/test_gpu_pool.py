"""The keyed frame pool (cache.FramePool, sbev_msmv_fwd_pool, sbev_sample_mix_pool, sbev_decoder_config.slot_table) against the paths it
must equal BIT for bit: the dense pyramid holding the same frames, and the by-value ring where the ring can express the step.  Every
comparison is torch.equal between two of this library's own paths; shapes are the smallest that reach every branch.  No test feeds an
out-of-range table: the kernels' clamp is for C callers and is checked by reading csrc/msmv_common.hpp::msmv_pool_slot."""
import copy

import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

from sparsebev_amd import _lib, ops, synthetic as S  # noqa: E402
from sparsebev_amd.cache import FrameFeatureCache, FramePool  # noqa: E402
from sparsebev_amd.transformer import SparseBEVTransformer  # noqa: E402

DEV = 'cuda:0'
PREFIX = 'decoder.decoder_layer.'
G, C, N = 4, 64, 6
# per-sample tables over 5 slots, T = 3: sample 0 a permutation, sample 1 another one with a duplicate (logical frames 0 and 2 share slot 1)
TABLES = {3: [[3, 0, 4], [1, 2, 1]], 4: [[3, 0, 4, 2], [1, 2, 1, 0]], 8: [[3, 0, 4, 2, 1, 3, 0, 4], [1, 2, 1, 0, 0, 4, 3, 2]]}


def slots_and_dense(B, T, n_slots, pyr, dtype, table, seed):
    """distinct random frames in every slot [B*n_slots*6, H, W, G*C], the device table, and the dense pyramid [B*T*6, H, W, G*C] built
    from them with torch indexing"""
    sizes = S.PYRAMIDS[pyr][2]
    g = torch.Generator(device=DEV).manual_seed(seed)
    levels = [torch.randn(B * n_slots * N, h, w, G * C, generator=g, device=DEV).to(dtype) for h, w in sizes]
    tab = torch.tensor(table, device=DEV, dtype=torch.int32)
    idx = tab.long()
    dense = [f.reshape(B, n_slots, N, h, w, G * C)[torch.arange(B, device=DEV)[:, None], idx].reshape(B * T * N, h, w, G * C).contiguous()
             for f, (h, w) in zip(levels, sizes)]
    return levels, tab, dense, g


def points(B, T, Q, P, L, g):
    loc = torch.rand(B * T * G, Q, P, 3, generator=g, device=DEV) * 1.3 - 0.15          # incl. a border band and outside points
    loc[..., 2] = torch.randint(0, 6, (B * T * G, Q, P), generator=g, device=DEV).float() / 5
    w = torch.softmax(torch.randn(B * T * G, Q, P, L, generator=g, device=DEV), -1)
    return loc, w


@pytest.mark.parametrize('pyr,dtype,P,n_slots,table', [
    ('tiny', torch.float32, 4, 5, TABLES[3]), ('tiny', torch.bfloat16, 4, 5, TABLES[3]), ('tiny', torch.float16, 4, 5, TABLES[3]),
    ('tiny5', torch.float32, 4, 5, TABLES[3]), ('tiny5', torch.bfloat16, 4, 5, TABLES[3]), ('tiny', torch.float32, 8, 5, TABLES[3]),
    ('tiny5', torch.float16, 8, 5, TABLES[3]),
    ('tiny', torch.float32, 4, 2, [[1, 0, 1], [0, 0, 1]]),                              # fewer slots than frames
])
@pytest.mark.parametrize('layout', [ops.OUT_MIX, ops.OUT_REF])
def test_pool_sampler_equals_dense(pyr, dtype, P, n_slots, table, layout):
    B, T, Q = 2, 3, 9                                                                    # Q odd; 216 items on 54 workgroups, one item per wave
    L = len(S.PYRAMIDS[pyr][2])
    levels, tab, dense, g = slots_and_dense(B, T, n_slots, pyr, dtype, table, seed=11 + P + n_slots)
    loc, w = points(B, T, Q, P, L, g)
    want = ops.msmv_sampling_nhwc(dense, B, T, G, loc, w, out_layout=layout)
    got = ops.msmv_sampling_pool(levels, B, T, G, tab, n_slots, loc, w, out_layout=layout)
    assert torch.equal(got, want) and got.abs().max() > 0
    prev = _lib.load().sbev_msmv_buffer_taps(0)                                          # the 64-bit global-load instantiations
    try:
        assert torch.equal(ops.msmv_sampling_pool(levels, B, T, G, tab, n_slots, loc, w, out_layout=layout), want)
    finally:
        _lib.load().sbev_msmv_buffer_taps(prev)


def test_pool_sampler_pipelined_items():
    """enough items for the two-items-per-wave launch (B' * Q >= 8192; the shapes above take one item per wave) with Q odd: every other
    wave's two items belong to different sample batches -- other frames, other slots: the table is read per item"""
    B, T, Q, P, n_slots = 2, 3, 343, 4, 5
    levels, tab, dense, g = slots_and_dense(B, T, n_slots, 'tiny', torch.float32, TABLES[3], seed=5)
    loc, w = points(B, T, Q, P, 4, g)
    assert B * T * G * Q >= 8192 and (B * T * G * Q) % 2 == 0 and Q % 2 == 1
    assert torch.equal(ops.msmv_sampling_pool(levels, B, T, G, tab, n_slots, loc, w), ops.msmv_sampling_nhwc(dense, B, T, G, loc, w))
    # the table's CONTENTS are read at run time: refresh it in place, same launch arguments, other frames
    tab.copy_(torch.tensor([[0, 0, 2], [4, 3, 4]], device=DEV, dtype=torch.int32))
    dense2 = [f.reshape(B, n_slots, N, *f.shape[1:])[torch.arange(B, device=DEV)[:, None], tab.long()].reshape(B * T * N, *f.shape[1:]).contiguous() for f in levels]
    assert torch.equal(ops.msmv_sampling_pool(levels, B, T, G, tab, n_slots, loc, w), ops.msmv_sampling_nhwc(dense2, B, T, G, loc, w))


@pytest.mark.parametrize('pyr,dtype,T,P', [('tiny', torch.float32, 3, 4), ('tiny5', torch.bfloat16, 3, 4), ('tiny', torch.float16, 3, 8),
                                           ('tiny', torch.float32, 4, 4), ('tiny5', torch.float32, 8, 4), ('tiny', torch.bfloat16, 8, 8)])
def test_pool_fused_equals_dense_and_ring(pyr, dtype, T, P):
    """B = 2, Q = 20, T = 3 is the smallest fused shape of tests/test_gpu_fused.py (12 in-points: the padded instantiation); T = 4 is the
    tuned whole-row-tile instantiation, T = 8 gives every wave a second unit (the slot requested one unit ahead)."""
    B, Q, n_slots = 2, 20, 5
    L = len(S.PYRAMIDS[pyr][2])
    levels, tab, dense, g = slots_and_dense(B, T, n_slots, pyr, dtype, TABLES[T], seed=31 + T + P)
    loc, w = points(B, T, Q, P, L, g)
    params = torch.randn(B, Q, G * (C * C + 128 * T * P), generator=g, device=DEV) * 0.3
    want = ops.sample_mix(dense, B, T, G, loc, w, params, 128)
    got = ops.sample_mix(levels, B, T, G, loc, w, params, 128, slot_table=tab, n_slots=n_slots)
    assert torch.equal(got, want) and got.abs().max() > 0
    # pair output and a launch order: the same launch, other epilogue / other block -> item map
    og = torch.Generator().manual_seed(3)
    order = torch.cat([torch.randperm(Q, generator=og) + b * Q for b in range(B)]).to(torch.int32).to(DEV)      # each sample's rows stay together
    assert torch.equal(ops.sample_mix(levels, B, T, G, loc, w, params, 128, slot_table=tab, n_slots=n_slots, up_log2=3, order=order),
                       ops.sample_mix(dense, B, T, G, loc, w, params, 128, up_log2=3, order=order))
    # all samples share one duplicate-free table: what the by-value ring expresses
    shared = TABLES[T][0][:T] if len(set(TABLES[T][0])) == T else [3, 0, 4, 2, 1][:T]
    if len(set(shared)) == T:
        tab.copy_(torch.tensor([shared] * B, device=DEV, dtype=torch.int32))
        assert torch.equal(ops.sample_mix(levels, B, T, G, loc, w, params, 128, slot_table=tab, n_slots=n_slots),
                           ops.sample_mix(levels, B, T, G, loc, w, params, 128, frame_slots=shared, n_slots=n_slots))
        assert torch.equal(ops.msmv_sampling_pool(levels, B, T, G, tab, n_slots, loc, w), ops.msmv_sampling_ring(levels, B, T, G, shared, n_slots, loc, w))
    with pytest.raises(RuntimeError, match='not both'):
        ops.sample_mix(levels, B, T, G, loc, w, params, 128, slot_table=tab, frame_slots=[0] * T, n_slots=n_slots)


# ---- the decoder step ------------------------------------------------------------------------------------------------------------

def build(T, L, seed, num_layers=2, graph=False):
    params = S.make_params(seed, embed_dims=256, num_frames=T, num_points=4, num_levels=L)
    m = SparseBEVTransformer(256, num_frames=T, num_points=4, num_layers=num_layers, num_levels=L, num_classes=10, code_size=10, pc_range=S.PC_RANGE)
    m.load_state_dict({PREFIX + k: v for k, v in params.items()}, strict=True)
    m = m.to(DEV).eval()
    m.decoder.static_graph = graph
    return m


class Frames:
    """key -> one sample's frame (list over levels of [6, C, H, W] NCHW), generated once and kept"""

    def __init__(self, pyr, seed):
        self.sizes = S.PYRAMIDS[pyr][2]
        self.g = torch.Generator(device=DEV).manual_seed(seed)
        self.frames = {}

    def __getitem__(self, key):
        if key not in self.frames:
            self.frames[key] = [torch.randn(N, G * C, h, w, generator=self.g, device=DEV) for h, w in self.sizes]
        return self.frames[key]

    def dense(self, keys):
        """the reference's layout for a step: list over levels of [B, T*6, C, H, W]"""
        return [torch.stack([torch.cat([self[k][l] for k in row], 0) for row in keys], 0) for l in range(len(self.sizes))]


def feed(pool, frames, keys):
    for b, k in pool.missing(keys):
        pool.put(b, k, frames[k])
    return pool.pyramid(keys)


def test_decoder_on_pool_equals_dense_eager():
    B, Q, T = 2, 49, 4
    ih, iw, sizes = S.PYRAMIDS['tiny']
    m = build(T, len(sizes), 7)
    frames = Frames('tiny', 70)
    bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=8)]
    metas = S.make_img_metas(B, T, ih, iw)
    keys = [['a3', 'a2', 'a1', 'a0'], ['b1', 'b0', 'b1', 'b2']]                       # per-sample tables, one duplicate
    pool = FramePool(T, n_slots=5)
    pyr = feed(pool, frames, keys)
    assert not hasattr(pyr, 'frame_slots') and pyr.slot_table.dtype == torch.int32 and tuple(pyr.slot_table.shape) == (B, T)
    assert (pyr.B, pyr.T, pyr.n_slots, pyr.GC, len(pyr.levels)) == (B, T, 5, G * C, len(sizes))
    got = m(bbox, feat, pyr, None, copy.deepcopy(metas))
    want = m(bbox, feat, frames.dense(keys), None, copy.deepcopy(metas))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # the two-launch path of the step (stand-alone sampler through the table) and the layer-by-layer path agree with it as they do for a dense pyramid
    from sparsebev_amd import runtime
    runtime.fuse_sample_mix(False)
    try:
        got2 = m(bbox, feat, pyr, None, copy.deepcopy(metas))
    finally:
        runtime.fuse_sample_mix(True)
    assert torch.equal(got2[0], want[0]) and torch.equal(got2[1], want[1])
    # eval() with grad enabled (a caller that forgot no_grad): the inference runtime with a warning, as for the ring
    with torch.enable_grad(), pytest.warns(UserWarning, match='inference'):
        got3 = m(bbox, feat.clone().requires_grad_(True), pyr, None, copy.deepcopy(metas))
    assert torch.equal(got3[0], want[0]) and not got3[0].requires_grad
    # training refuses the pool as it refuses the ring
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match='inference cache'):
            m.train()(bbox, feat.clone().requires_grad_(True), pyr, None, copy.deepcopy(metas))
    m.eval()


def test_one_graph_for_every_phase_and_scene_change():
    """n_slots = 12 is above StepGraphs.MAX (8): the by-value ring would evict its own graphs lap after lap; the pool captures once"""
    B, Q, T, n_slots, steps = 1, 49, 4, 12, 30
    ih, iw, sizes = S.PYRAMIDS['tiny']
    g, e = build(T, len(sizes), 9, graph=True), build(T, len(sizes), 9)
    from sparsebev_amd.runtime import CapturedStep, StepGraphs
    assert n_slots > StepGraphs.MAX
    frames = Frames('tiny', 90)
    bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=10)]
    metas = S.make_img_metas(B, T, ih, iw)
    pool = FramePool(T, n_slots=n_slots)
    scene, first, ptr = 0, 0, None
    for i in range(steps):
        if i == 17:
            scene, first = 1, i                      # scene change: T unseen keys over the next steps, the window padded by duplicates
        keys = [[(scene, max(i - t, first)) for t in range(T)]]
        n_missing = len(pool.missing(keys))
        assert n_missing == 1                        # a new key each step (the first step's padded window included)
        pyr = feed(pool, frames, keys)
        ptr = ptr or pyr.slot_table.data_ptr()
        assert pyr.slot_table.data_ptr() == ptr and pool.slot_table.data_ptr() == ptr
        got = g(bbox, feat, pyr, None, metas)
        want = e(bbox, feat, frames.dense(keys), None, metas)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), i
    sg = g.decoder._runtime.step_graphs
    graphs = [v for v in sg.entries.values() if isinstance(v, CapturedStep)]
    print('pool stream: %d steps, captures %d, graph launches %d, replays of the one graph %s' % (steps, sg.captures, sg.replays, [v.replays for v in graphs]))
    # step 0 is the shape's first sighting (eager), step 1 captures and launches, every later step replays that one graph: the entry's
    # 'replays' counts launches after the capturing call's own (steps - 2), StepGraphs.replays every launch (steps - 1, as in test_gpu_stepgraph.py)
    assert sg.captures == 1 and len(graphs) == 1 and graphs[0].replays == steps - 2 and sg.replays == steps - 1, (sg.captures, sg.replays)


def test_sequential_keys_equal_the_ring():
    B, Q, T = 1, 49, 4
    ih, iw, sizes = S.PYRAMIDS['tiny']
    m = build(T, len(sizes), 12)
    frames = Frames('tiny', 120)
    bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=13)]
    metas = S.make_img_metas(B, T, ih, iw)
    ring, pool = FrameFeatureCache(T, n_slots=T + 1), FramePool(T, n_slots=T + 1)
    for k in range(T - 1):
        ring.push([f[None] for f in frames[k]])
    for i in range(T - 1, 3 * T - 1):                # 2 T steps
        ring.push([f[None] for f in frames[i]])
        keys = [[i - t for t in range(T)]]
        a = m(bbox, feat, ring.pyramid(), None, metas)
        b = m(bbox, feat, feed(pool, frames, keys), None, metas)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), i


def test_two_streams_are_independent():
    Q, T, steps = 49, 4, 7
    ih, iw, sizes = S.PYRAMIDS['tiny']
    m = build(T, len(sizes), 14, graph=True)
    frames = Frames('tiny', 140)
    bbox, feat = [t.to(DEV) for t in S.make_queries(2, Q, seed=15)]
    metas = S.make_img_metas(2, T, ih, iw)

    def window(b, i):                                # sample 1 changes scene at step 3, sample 0 streams on
        scene, first = (1, 3) if b == 1 and i >= 3 else (0, 0)
        return [('s%d' % b, scene, max(i - t, first)) for t in range(T)]

    both = FramePool(T, n_slots=6)
    single = [FramePool(T, n_slots=6), FramePool(T, n_slots=6)]
    for i in range(steps):
        keys = [window(0, i), window(1, i)]
        got = m(bbox, feat, feed(both, frames, keys), None, metas)
        for b in range(2):
            one = m(bbox[b:b + 1].contiguous(), feat[b:b + 1].contiguous(), feed(single[b], frames, [keys[b]]), None, metas[b:b + 1])
            assert torch.equal(got[0][:, b], one[0][:, 0]) and torch.equal(got[1][:, b], one[1][:, 0]), (i, b)
    both.drop(1)
    assert [b for b, _ in both.missing([window(0, steps - 1), window(1, steps - 1)])] == [1] * T


def test_head_on_pool_equals_dense():
    from sparsebev_amd.head import SparseBEVHead
    B, T = 2, 4
    ih, iw, sizes = S.PYRAMIDS['tiny']
    torch.manual_seed(0)
    head = SparseBEVHead(num_classes=10, in_channels=256, num_query=64, code_size=10,
                         transformer=dict(type='SparseBEVTransformer', embed_dims=256, num_frames=T, num_points=4, num_layers=2, num_levels=len(sizes),
                                          num_classes=10, code_size=10, pc_range=S.PC_RANGE),
                         bbox_coder=dict(type='NMSFreeCoder', post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_num=30,
                                         score_threshold=None, num_classes=10, pc_range=S.PC_RANGE)).to(DEV).eval()
    frames = Frames('tiny', 160)
    metas = S.make_img_metas(B, T, ih, iw)
    keys = [['a3', 'a2', 'a1', 'a0'], ['b0', 'b0', 'b1', 'b1']]
    pool = FramePool(T, n_slots=4)
    out_p = head(feed(pool, frames, keys), metas)
    out_d = head(frames.dense(keys), metas)
    res_p, res_d = head.get_bboxes(out_p, metas), head.get_bboxes(out_d, metas)
    assert torch.equal(out_p['all_cls_scores'], out_d['all_cls_scores']) and torch.equal(out_p['all_bbox_preds'], out_d['all_bbox_preds'])
    assert len(res_p) == len(res_d) == B and sum(r[0].shape[0] for r in res_p) > 0
    for (bb, ss, ll), (rb, rs, rl) in zip(res_p, res_d):
        assert torch.equal(bb, rb) and torch.equal(ss, rs) and torch.equal(ll, rl)
