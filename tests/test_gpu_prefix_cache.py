"""Prefix cache (csrc/decoder.hip: sbev_decoder_forward_cached, runtime.PrefixCache): layer 0's position encoder + in-projection, self
attention and parameter generator read the queries and the weights only; a step whose queries repeat bit for bit skips the three
launches and reads what the step that stored them left in the cache.  The reference for every comparison is the SAME model with the
cache forced off (runtime.prefix_cache(False): the force word, same launches, same captures); outputs are compared as int32 views.
Shapes: `tiny` pyramid, T = 2, 2 layers; Q = 36, B = 1 (one 32-row fragment + 4, a 4-row chain tail) and Q = 49, B = 2 (98 rows: the
sample boundary falls inside a 32-query attention block); the watch launch's second pass and leftover words at Q = 289, B = 1.  Every
case runs on the eager runtime and on replayed steps."""
import copy

import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

from sparsebev_amd import runtime, synthetic as S  # noqa: E402
from sparsebev_amd.transformer import SparseBEVTransformer  # noqa: E402

DEV = 'cuda:0'
PREFIX = 'decoder.decoder_layer.'
T, LAYERS = 2, 2
SHAPES = [(1, 36), (2, 49)]
NAN_BITS = 0x7fc00000


def bits(pair):
    return tuple(t.contiguous().view(torch.int32).clone() for t in pair)


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


class Rig:
    """A model and one set of inputs; ``call`` returns the outputs' bits, ``ref`` the same call with the cache forced off."""

    def __init__(self, B, Q, graph, seed=11):
        self.B, self.Q, self.graph = B, Q, graph
        self.ih, self.iw, self.sizes = S.PYRAMIDS['tiny']
        params = S.make_params(seed, embed_dims=256, num_frames=T, num_points=4, num_levels=len(self.sizes))
        m = SparseBEVTransformer(256, num_frames=T, num_points=4, num_layers=LAYERS, num_levels=len(self.sizes), pc_range=S.PC_RANGE)
        m.load_state_dict({PREFIX + k: v for k, v in params.items()}, strict=True)
        self.model = m.to(DEV).eval()
        self.model.decoder.static_graph = graph
        self.bbox, self.feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=12)]
        self.feats = [f.to(DEV) for f in S.make_features(B, T, self.sizes, seed=13)]
        self.metas = S.make_img_metas(B, T, self.ih, self.iw)
        runtime.prefix_cache(True)

    @property
    def rt(self):
        return self.model.decoder._runtime

    def call(self, bbox=None, feat=None, feats=None, metas=None, mask=None):
        out = self.model(self.bbox if bbox is None else bbox, self.feat if feat is None else feat,
                         list(self.feats if feats is None else feats), mask, copy.deepcopy(self.metas if metas is None else metas))
        return bits(out)

    def ref(self, **kw):
        runtime.prefix_cache(False)
        try:
            return self.call(**kw)
        finally:
            runtime.prefix_cache(True)

    def settle(self, **kw):
        """calls until this kind of call runs the way the rig is meant to: a replay (first sighting, capture, replay) or the eager step"""
        for _ in range(3 if self.graph else 1):
            out = self.call(**kw)
        return out

    def caches(self):
        steps = [e.prefix for e in self.rt.step_graphs.entries.values() if isinstance(e, runtime.CapturedStep)]
        return [c for c in ([self.rt._prefix] + steps) if c is not None]

    def live_cache(self):
        """the cache the rig's kind of call uses"""
        if not self.graph:
            return self.rt._prefix
        steps = [e.prefix for e in self.rt.step_graphs.entries.values() if isinstance(e, runtime.CapturedStep) and e.prefix is not None]
        assert len(steps) == 1
        return steps[0]

    def counters(self):
        return self.rt.prefix_counters()

    def delta(self, before):
        h, m = self.counters()
        return h - before[0], m - before[1]


@pytest.fixture(params=[False, True], ids=['eager', 'replay'])
def graph(request):
    return request.param


@pytest.fixture(autouse=True)
def _cache_on_again():
    yield
    runtime.prefix_cache(True)


@pytest.mark.parametrize('B,Q', SHAPES)
def test_four_identical_calls_from_a_poisoned_cache(B, Q, graph):
    r = Rig(B, Q, graph)
    want = r.ref()
    r.settle()
    c = r.live_cache()
    assert c is not None, 'the step takes no prefix cache'
    c.buf.view(torch.int32).fill_(NAN_BITS)          # whatever a hit read before a miss stored it would surface
    c.reset()                                        # header zero (and the force word as the switch stands: off)
    outs = [r.call() for _ in range(4)]
    assert all(same(o, want) for o in outs)
    assert c.counters() == (3, 1)
    if graph:
        assert r.rt.step_graphs.captures == 1


@pytest.mark.parametrize('B,Q', SHAPES)
def test_cloned_queries_hit_and_changed_queries_miss(B, Q, graph):
    r = Rig(B, Q, graph)
    want = r.ref()
    r.settle()
    n0 = r.counters()
    assert same(r.call(bbox=r.bbox.clone(), feat=r.feat.clone()), want)
    assert r.delta(n0) == (1, 0), 'same values in new tensors'
    for which in ('bbox_first', 'feat_last'):
        for in_place in (True, False):
            bbox, feat = (r.bbox, r.feat) if in_place else (r.bbox.clone(), r.feat.clone())
            t = bbox if which == 'bbox_first' else feat
            flat = t.view(-1)
            i = 0 if which == 'bbox_first' else flat.numel() - 1
            flat[i] = flat[i] + 0.25
            n0 = r.counters()
            got = r.call(bbox=bbox, feat=feat)
            assert r.delta(n0) == (0, 1), (which, in_place)
            want = r.ref(bbox=bbox, feat=feat)
            assert same(got, want), (which, in_place)
            n0 = r.counters()
            assert same(r.call(bbox=bbox.clone(), feat=feat.clone()), want)
            assert r.delta(n0) == (1, 0), (which, in_place, 'the call after a miss')
            r.bbox, r.feat = bbox, feat


@pytest.mark.parametrize('B,Q', SHAPES)
def test_new_frame_same_queries_hits(B, Q, graph):
    r = Rig(B, Q, graph)
    r.settle()
    feats2 = [f.to(DEV) for f in S.make_features(B, T, r.sizes, seed=99)]
    metas2 = S.make_img_metas(B, T, r.ih, r.iw, frame_dt=0.4)
    want = r.ref(feats=feats2, metas=metas2)
    r.call()                                         # (back on the first frame: the cache holds these queries either way)
    n0 = r.counters()
    got = r.call(feats=feats2, metas=metas2)
    assert r.delta(n0) == (1, 0)
    assert same(got, want) and not same(got, r.ref())


@pytest.mark.parametrize('B,Q', SHAPES[:1])
@pytest.mark.parametrize('name', ['position_encoder.3.weight', 'self_attn.attention.attn.in_proj_weight', 'mixing.parameter_generator.weight'])
def test_weight_changed_in_place(B, Q, graph, name):
    """one weight of each skipped launch: no stale x0 / att0 / params0"""
    r = Rig(B, Q, graph)
    before = r.settle()
    p = dict(r.model.named_parameters())[PREFIX + name]
    p.mul_(1.5)
    outs = [r.call() for _ in range(3)]              # replay rig: eager, capture, replay -- all on the new weights
    want = r.ref()
    assert all(same(o, want) for o in outs) and not same(want, before)


@pytest.mark.parametrize('B,Q', SHAPES)
def test_masked_call_between_two_without(B, Q, graph):
    r = Rig(B, Q, graph)
    want = r.settle()
    mask = (torch.rand(Q, Q, device=DEV) < 0.2).to(torch.uint8)
    mask.fill_diagonal_(0)
    n0 = r.counters()
    masked = [r.call(mask=mask) for _ in range(3 if graph else 1)]
    assert r.delta(n0) == (0, 0), 'a masked step touched a cache'
    want_masked = r.ref(mask=mask)
    assert all(same(o, want_masked) for o in masked) and not same(want_masked, want)
    n0 = r.counters()
    assert same(r.call(), want) and same(r.ref(), want)
    assert r.delta(n0) == (1, 1)


@pytest.mark.parametrize('B,Q', SHAPES)
def test_off_and_on_without_a_new_capture(B, Q):
    r = Rig(B, Q, True)
    want = r.settle()
    assert r.rt.step_graphs.captures == 1
    c = r.live_cache()
    n0 = c.counters()
    assert runtime.prefix_cache(False) is True
    off = [r.call() for _ in range(2)]
    assert (c.counters()[0] - n0[0], c.counters()[1] - n0[1]) == (0, 2)
    assert runtime.prefix_cache(True) is False
    on = [r.call() for _ in range(2)]
    assert (c.counters()[0] - n0[0], c.counters()[1] - n0[1]) == (2, 2)
    assert all(same(o, want) for o in off + on)
    assert r.rt.step_graphs.captures == 1


@pytest.mark.parametrize('B,Q', SHAPES)
def test_two_captured_steps_on_one_workspace(B, Q):
    """an NCHW list (staged) and a channels-last list (read in place) of the same shapes: one workspace, two caches"""
    r = Rig(B, Q, True)
    nhwc = [f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3) for f in r.feats]
    bbox2, feat2 = [t.to(DEV) for t in S.make_queries(B, Q, seed=77)]
    kinds = [dict(), dict(bbox=bbox2, feat=feat2, feats=nhwc)]
    for kw in kinds:
        r.settle(**kw)
    steps = [e for e in r.rt.step_graphs.entries.values() if isinstance(e, runtime.CapturedStep)]
    assert len(steps) == 2 and steps[0].ws_key == steps[1].ws_key and len(r.rt._graph_ws) == 1
    assert steps[0].prefix is not None and steps[1].prefix is not None and steps[0].prefix is not steps[1].prefix
    want = [r.ref(**kw) for kw in kinds]
    assert not same(want[0], want[1])
    n0 = r.counters()
    for _ in range(3):
        for kw, w in zip(kinds, want):
            assert same(r.call(**kw), w)
    assert r.delta(n0)[0] >= 4, 'the alternating steps never hit'
    assert r.rt.step_graphs.captures == 2


@pytest.mark.parametrize('B,Q', SHAPES[:1])
def test_gemm_modes_on_the_eager_runtime(B, Q):
    r = Rig(B, Q, False)
    for mode in ('f16x3', 'f16x4', 'f16x3'):
        r.model.decoder.gemm_mode = mode
        want = r.ref()
        n0 = r.counters()
        outs = [r.call() for _ in range(2)]
        assert all(same(o, want) for o in outs), mode
        assert r.delta(n0)[0] >= 1, mode
    r.model.decoder.gemm_mode = 'f32'
    r.call()
    r.call()
    assert r.rt._prefix is None, 'the exact GEMM mode takes no cache'


@pytest.mark.parametrize('B,Q', SHAPES)
def test_queries_with_a_nan_repeat_bit_for_bit(B, Q, graph):
    r = Rig(B, Q, graph)
    r.feat[0, Q // 2, 5] = float('nan')
    r.bbox[B - 1, Q - 1, 9] = float('nan')
    want = r.ref()
    r.settle()
    n0 = r.counters()
    assert same(r.call(), want) and same(r.call(bbox=r.bbox.clone(), feat=r.feat.clone()), want)
    assert r.delta(n0) == (2, 0)


def test_one_bit_changes_where_the_watch_launch_loops_and_in_its_leftover_words(graph):
    """B = 1, Q = 289 (17 x 17): the watch launch compares 16 bytes per thread with 64 workgroups of 256 threads, so query_feat -- 289 * 256
    words = 18 496 chunks -- takes a second pass from chunk 16 384 on (word 65 536), every workgroup sees data, and query_bbox -- an odd
    number of rows of 10 words -- leaves words 2888 and 2889 behind its last chunk.  One word at a time changes by its lowest mantissa
    bit, or from +0.0 to -0.0 (equal as floats, another bit pattern): each must count as exactly one miss, give the outputs of the same
    call with the cache off, and be followed by a hit on clones of the changed queries."""
    B, Q = 1, 289
    r = Rig(B, Q, graph)
    n_bbox, n_feat = B * Q * 10, B * Q * 256
    assert n_bbox % 4 == 2 and n_feat // 4 > 64 * 256
    zero_feat, zero_bbox = 70000, n_bbox - 1                        # a second-pass word and the last leftover word start as +0.0
    r.feat.view(-1)[zero_feat] = 0.0
    r.bbox.view(-1)[zero_bbox] = 0.0
    want = r.ref()
    r.settle()
    n0 = r.counters()
    assert same(r.call(bbox=r.bbox.clone(), feat=r.feat.clone()), want)
    assert r.delta(n0) == (1, 0)
    LOW, SIGN = 1, -0x80000000
    flips = [('bbox', 0, LOW), ('bbox', n_bbox - 2, LOW), ('bbox', zero_bbox, SIGN),
             ('feat', 65535, LOW), ('feat', 65536, LOW), ('feat', 63 * 256 * 4, LOW), ('feat', n_feat - 1, LOW), ('feat', zero_feat, SIGN)]
    for which, word, bit in flips:
        bbox, feat = r.bbox.clone(), r.feat.clone()
        t = (bbox if which == 'bbox' else feat).view(-1).view(torch.int32)
        before = int(t[word])
        t[word] = t[word] ^ bit
        assert int(t[word]) != before and (bit == LOW or (before == 0 and float((bbox if which == 'bbox' else feat).view(-1)[word]) == 0.0))
        n0 = r.counters()
        got = r.call(bbox=bbox, feat=feat)
        assert r.delta(n0) == (0, 1), (which, word, 'a changed word went unnoticed' if r.delta(n0)[1] == 0 else 'more than one miss')
        assert same(got, r.ref(bbox=bbox, feat=feat)), (which, word)
        n0 = r.counters()
        assert same(r.call(bbox=bbox.clone(), feat=feat.clone()), got), (which, word)
        assert r.delta(n0) == (1, 0), (which, word, 'the call after a miss')
        r.bbox, r.feat = bbox, feat
