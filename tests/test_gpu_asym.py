"""The decoder on inputs that share nothing between the samples of a batch: a camera pose and a frame spacing per sample
(synthetic.make_img_metas_per_sample), a pc_range whose x and y extents differ and that is not centred (synthetic.PC_RANGE_ASYM), and
class counts other than the 10 box columns (synthetic.CLASS_COUNTS).  With the default inputs of every other decoder-level test
lidar2img, time_diff and the velocity divisor are the same for every sample, num_classes == code_size and x / y can be swapped unseen:
a kernel that drops the sample index from one of those reads, or swaps the two widths, passes them all.

Reference recording: fixture G14 (tests/golden/make_golden.py::main_asym: the reference's SparseBEVTransformer.forward, B = 3, Q = 36,
T = 2, 7 classes); elsewhere the oracle in fp64 on the CUDA kernel's sampling semantics.  Bounds: 1e-4, the project's parity bound,
unless a test says otherwise.  Every assertion message names the worst sample and tensor.  Camera hits of G14's layer-0 sample points per
sample (none / one camera / two or more): 2.2 / 93.2 / 4.6 %, 1.6 / 91.7 / 6.8 %, 1.6 / 93.3 / 5.0 %."""
import copy
import functools

import numpy as np
import pytest
import torch

from conftest import op_by_op_runtime
from oracle import sparsebev_oracle as O
from sparsebev_amd import synthetic as S
from sparsebev_amd.transformer import SparseBEVTransformer, FeaturePyramid, DecoderContext
from test_oracle_golden import g14_inputs, forced_layer_inputs

gpu = pytest.mark.gpu
TOL = 1e-4
DEV = 'cuda:0'
PREFIX = 'decoder.decoder_layer.'
KERNEL = O.msmv_sampling_kernel_semantics


# ---- helpers ---------------------------------------------------------------------------------------------------------------------

def per_sample(got, ref):
    """max |got - ref| per sample of [B, Q, X] or [layers, B, Q, X] tensors"""
    d = (got.detach().cpu().double() - ref.detach().cpu().double()).abs()
    d = torch.nan_to_num(d, nan=float('inf'))
    return d.amax(dim=(0, 2, 3) if d.dim() == 4 else (1, 2))


def assert_close(what, pairs, tol):
    """pairs: (tensor name, got, ref); prints every figure, then asserts with the worst sample and tensor named"""
    worst = (-1.0, None, None, None)
    for name, got, ref in pairs:
        assert tuple(got.shape) == tuple(ref.shape), '%s %s: shape %s, expected %s' % (what, name, tuple(got.shape), tuple(ref.shape))
        e = per_sample(got, ref)
        print('%s %-5s max |error| per sample %s (bound %.0e)' % (what, name, ' '.join('%.2e' % v for v in e.tolist()), tol))
        if float(e.max()) > worst[0]:
            worst = (float(e.max()), name, int(e.argmax()), e.tolist())
    assert worst[0] < tol, '%s: worst is sample %d of %s, %.3e >= %.0e (per sample %s)' % (what, worst[2], worst[1], worst[0], tol, worst[3])
    return worst[0]


def assert_same(what, got, ref):
    """(cls, box) bit for bit; the message names the samples that differ"""
    for name, a, b in (('cls', got[0], ref[0]), ('box', got[1], ref[1])):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        if not torch.equal(a, b):
            e = per_sample(a, b)
            raise AssertionError('%s: %s differs in samples %s (max |difference| per sample %s)'
                                 % (what, name, [i for i, v in enumerate(e.tolist()) if v > 0] or 'none by value (bits only)', e.tolist()))


def model_of(params, T, L, num_classes, pc_range, num_layers, graph=False, P=4):
    m = SparseBEVTransformer(256, num_frames=T, num_points=P, num_layers=num_layers, num_levels=L, num_classes=num_classes,
                             code_size=10, pc_range=pc_range)
    missing = m.load_state_dict({PREFIX + k: v for k, v in params.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    m = m.to(DEV).eval()
    m.decoder.static_graph = graph
    return m


def fp64_oracle(params, bbox, feat, feats, metas, pc_range, num_layers=1, sampler=KERNEL):
    return O.decoder({k: v.double() for k, v in params.items()}, bbox.double(), feat.double(), [f.double() for f in feats], metas,
                     pc_range, num_layers=num_layers, sampler=sampler)


def swap_xy(pc):
    return [pc[1], pc[0], pc[2], pc[4], pc[3], pc[5]]


@functools.lru_cache(maxsize=None)
def g14():
    return g14_inputs()


@functools.lru_cache(maxsize=None)
def g14_oracle():
    """the fp32 oracle's (cls, box) on the G14 inputs, kernel sampling semantics, 2 layers -- computed once, never written to"""
    g, params, feats, metas, pc, nc = g14()
    return O.decoder(params, g['query_bbox'], g['query_feat'], feats, metas, pc, num_layers=2, sampler=KERNEL)[:2]


def on_device(g, feats):
    return g['query_bbox'].to(DEV), g['query_feat'].to(DEV), [f.to(DEV) for f in feats]


# ---- CPU: the fixtures do their job ------------------------------------------------------------------------------------------------

def test_helper_gives_every_sample_its_own_pose_spacing_and_jitter():
    ih, iw, _ = S.PYRAMIDS['tiny']
    B, T = 4, 3
    metas, shared = S.make_img_metas_per_sample(B, T, ih, iw), S.make_img_metas(B, T, ih, iw)
    l2i = np.asarray([m['lidar2img'] for m in metas])
    assert l2i.shape == (B, T * 6, 4, 4) and l2i.dtype == np.float64
    assert np.array_equal(l2i[0], np.asarray(shared[0]['lidar2img']))                       # sample 0: identity pose
    for b in range(1, B):
        for i in range(T * 6):
            assert np.allclose(l2i[b, i], np.asarray(shared[b]['lidar2img'][i]) @ S.ego_pose(b), rtol=0, atol=1e-9)
            assert np.abs(l2i[b, i] - l2i[b - 1, i]).max() > 0.1
    td = O.time_diff_from_metas(metas, B)
    assert float((td[1:, 1:] - td[:-1, 1:]).abs().min()) >= 0.1                            # the velocity divisor td[:, 1] and every later frame
    ts = np.array([m['img_timestamp'] for m in metas]).reshape(B, T, 6)
    mean = (ts[:, 0] - np.floor(ts[:, 0])).mean(-1)                                         # frame 0: the jitter alone, < 0.03 s
    assert len({round(float(v), 6) for v in mean}) == B, mean                               # the per-camera jitter's mean changes with b
    pc = S.PC_RANGE_ASYM
    assert pc[3] - pc[0] != pc[4] - pc[1] and all(pc[i] != -pc[i + 3] for i in range(2)) and len(pc) == 6
    assert S.CLASS_COUNTS == (1, 7, 23, 64) and 10 not in S.CLASS_COUNTS


def test_g14_inputs_separate_a_wrong_sample_index_from_the_bound_by_two_orders():
    """With G14's inputs the oracle's cls AND box of every sample b >= 1 move by more than 100 x 1e-4 when (a) its lidar2img is replaced by
    sample 0's, (b) its timestamps are replaced by sample 0's, (c) the x and y ends of pc_range are swapped (measured: (a) 0.56 / 0.20,
    (b) 0.061 / 0.13, (c) 0.47 / 0.14 at the least moved sample; sample 0 itself stays bit-identical under (a) and (b))."""
    g, params, feats, metas, pc, nc = g14()
    B = len(metas)
    base = g14_oracle()

    def run(metas, pc):
        return O.decoder(params, g['query_bbox'], g['query_feat'], feats, metas, pc, num_layers=2, sampler=KERNEL)[:2]
    m_l2i, m_ts = copy.deepcopy(metas), copy.deepcopy(metas)
    for b in range(1, B):
        m_l2i[b]['lidar2img'] = copy.deepcopy(metas[0]['lidar2img'])
        m_ts[b]['img_timestamp'] = list(metas[0]['img_timestamp'])
    for what, out, own in (('lidar2img of sample 0', run(m_l2i, pc), True), ('timestamps of sample 0', run(m_ts, pc), True),
                           ('pc_range x <-> y', run(metas, swap_xy(pc)), False)):
        for name, a, r in (('cls', out[0], base[0]), ('box', out[1], base[1])):
            e = per_sample(a, r).tolist()
            print('%-24s %s moves per sample by %s' % (what, name, ' '.join('%.3f' % v for v in e)))
            assert min(e[1:]) > 100 * TOL, '%s: %s of sample %d moves by %.2e only' % (what, name, 1 + int(np.argmin(e[1:])), min(e[1:]))
            assert not own or e[0] == 0.0


def test_g14_inputs_fp32_oracle_equals_fp64_oracle_to_1e5():
    """The condition for keeping G14's seeds: no sample point within fp32 reach of an image border or the depth threshold, so that the
    parity bound is not spent on a flipped camera choice (measured worst 2.8e-6 cls, 7.7e-7 box over both layers, free-running)."""
    g, params, feats, metas, pc, nc = g14()
    for sampler in (O.msmv_sampling_gridsample, KERNEL):
        a = O.decoder(params, g['query_bbox'], g['query_feat'], feats, metas, pc, num_layers=2, sampler=sampler)
        d = fp64_oracle(params, g['query_bbox'], g['query_feat'], feats, metas, pc, num_layers=2, sampler=sampler)
        assert_close('fp32 vs fp64 oracle (%s)' % sampler.__name__[14:], [('cls', a[0], d[0]), ('box', a[1], d[1])], 1e-5)


# ---- G14 on the device -------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('how', ['default', 'op_by_op'])
def test_g14_decoder_teacher_forced_and_free_running(how):
    """Layer 0 free-running through the public forward and both layers teacher-forced from the recording, at 1e-4, on the default runtime
    (row chains, pair-mode tail, fused gather + mixing, on-demand relayout) and with one launch per op; the default runtime against the
    op-by-op one on layer 0 to 2e-5 (tests/test_gpu_chain.py's bound); the layer-by-layer Python path's query_feat too.  Measured worst
    9.5e-7 cls, 3.9e-7 box, 2.4e-6 feat against the recording; 7.2e-7 chains against op by op."""
    import contextlib
    g, params, feats, metas, pc, nc = g14()
    B, Q, T, L = [int(v) for v in g['cfg']]
    qb, qf, fd = on_device(g, feats)
    ctxm = op_by_op_runtime if how == 'op_by_op' else contextlib.nullcontext
    model = model_of(params, T, L, nc, pc, 2)
    one = model_of(params, T, L, nc, pc, 1)
    with ctxm():
        metas_in = copy.deepcopy(metas)
        cls, box = model(qb, qf, list(fd), None, metas_in)
        assert 'time_diff' not in metas_in[0] and not torch.is_tensor(metas_in[0]['lidar2img'])      # inputs not mutated
        per_layer = model.decoder._runtime.launches_per_layer(B, Q)
        assert per_layer == 6 if how == 'default' else per_layer >= 17, per_layer          # row chains: 6 launches a layer
        assert cls.shape == (2, B, Q, nc) and box.shape == (2, B, Q, 10)
        assert_close('G14 %s free-running layer 0' % how, [('cls', cls[0], g['out_cls'][0]), ('box', box[0], g['out_bbox'][0])], TOL)
        for i, (b_in, f_in) in enumerate(forced_layer_inputs(g)):
            c, bb = one(b_in.to(DEV), f_in.to(DEV), list(fd), None, copy.deepcopy(metas))
            assert_close('G14 %s teacher-forced layer %d' % (how, i), [('cls', c[0], g['out_cls'][i]), ('box', bb[0], g['out_bbox'][i])], TOL)
    if how == 'default':
        with op_by_op_runtime():
            cls_o, box_o = model_of(params, T, L, nc, pc, 2)(qb, qf, list(fd), None, copy.deepcopy(metas))
        assert_close('G14 row chains vs op by op, layer 0', [('cls', cls[0], cls_o[0]), ('box', box[0], box_o[0])], 2e-5)
    else:
        layer = model.decoder.decoder_layer
        pyr, ctx = FeaturePyramid(fd), DecoderContext(metas, B, torch.device(DEV))
        for i, (b_in, f_in) in enumerate(forced_layer_inputs(g)):
            x, c, bb = layer(b_in.to(DEV), f_in.to(DEV), pyr, None, ctx)
            assert_close('G14 layer by layer, teacher-forced layer %d' % i,
                         [('feat', x, g['out_feat'][i]), ('cls', c, g['out_cls'][i]), ('box', bb, g['out_bbox'][i])], TOL)


# ---- every row-block size with a sample boundary inside a block -------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('Q,pyr', [(36, 'tiny'), (361, 'tiny'), (729, 'tiny5')])
def test_sample_boundary_inside_a_row_block_vs_fp64_oracle(Q, pyr):
    """B = 3: 108 rows (4 rows per workgroup, pairs of 8: 36 mod 8 = 4), 1083 rows (8 per workgroup: 361 mod 8 = 1), 2187 rows (16 per
    workgroup: 729 mod 16 = 9) -- the smallest square query counts that reach each row-chain instantiation with the sample boundary off a
    block edge.  One layer, T = 2, 7 classes, per-sample metas, asymmetric range, against the fp64 oracle at 1e-4 (measured worst cls / box:
    8.4e-7 / 4.1e-7, 8.4e-6 / 1.7e-6, 8.4e-6 / 1.6e-6)."""
    B, T, nc, pc = 3, 2, 7, S.PC_RANGE_ASYM
    ih, iw, sizes = S.PYRAMIDS[pyr]
    L = len(sizes)
    params = S.make_params(300 + Q, embed_dims=256, num_frames=T, num_points=4, num_levels=L, num_classes=nc)
    bbox, feat = S.make_queries(B, Q, seed=301 + Q)
    feats = S.make_features(B, T, sizes, seed=302 + Q)
    metas = S.make_img_metas_per_sample(B, T, ih, iw)
    model = model_of(params, T, L, nc, pc, 1)
    cls, box = model(bbox.to(DEV), feat.to(DEV), [f.to(DEV) for f in feats], None, copy.deepcopy(metas))
    assert model.decoder._runtime.launches_per_layer(B, Q) == 6                           # the row chains
    ref = fp64_oracle(params, bbox, feat, feats, metas, pc)
    assert_close('B=3 x Q=%d vs fp64 oracle' % Q, [('cls', cls, ref[0]), ('box', box, ref[1])], TOL)


# ---- class counts ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def class_case(nc, Q):
    """inputs and the fp64 oracle's outputs for a class count, B = 3 -- computed once per (nc, Q), never written to"""
    B, T, pc = 3, 2, S.PC_RANGE_ASYM
    ih, iw, sizes = S.PYRAMIDS['tiny']
    params = S.make_params(400 + nc, embed_dims=256, num_frames=T, num_points=4, num_levels=len(sizes), num_classes=nc)
    bbox, feat = S.make_queries(B, Q, seed=401 + nc)
    feats = S.make_features(B, T, sizes, seed=402 + nc)
    metas = S.make_img_metas_per_sample(B, T, ih, iw)
    ref = fp64_oracle(params, bbox, feat, feats, metas, pc)
    return params, bbox, feat, feats, metas, pc, ref


@gpu
@pytest.mark.parametrize('how', ['default', 'op_by_op'])
@pytest.mark.parametrize('Q', [9, 36])
@pytest.mark.parametrize('nc', list(S.CLASS_COUNTS) + [65])
def test_class_counts_other_than_the_box_width_vs_fp64_oracle(nc, Q, how):
    """num_classes 1, 7, 23, 64 (the row chains' range ends at 64) and 65 (the step must fall back to the op-by-op launches and be right),
    at B = 3 x 9 (27 rows: an odd number of cls values for one class) and 3 x 36, one layer, asymmetric everything, against the fp64
    oracle at 1e-4; shapes; and what nan_to_num makes of non-finite outputs lands in the caller's tensors: with NaN / Inf in the biases
    of the two output Linears (no ReLU behind them -- the runtime's ReLUs turn a NaN into 0 where torch.relu keeps it,
    DESIGN_HISTORY.md) the last class column and box column 9 -- the last element of either tensor, where sbev_finish_outputs'
    two lengths show if swapped -- come back 0, class column 0 +FLT_MAX and box column 4 -FLT_MAX, every other column as before.  Measured worst 2.1e-6 cls, 9.7e-7 box."""
    import contextlib
    B, T = 3, 2
    params, bbox, feat, feats, metas, pc, ref = class_case(nc, Q)
    L = len(feats)
    ctxm = op_by_op_runtime if how == 'op_by_op' else contextlib.nullcontext
    fd = [f.to(DEV) for f in feats]
    bad = dict(params)
    bad['cls_branch.6.bias'], bad['reg_branch.4.bias'] = params['cls_branch.6.bias'].clone(), params['reg_branch.4.bias'].clone()
    bad['cls_branch.6.bias'][nc - 1] = float('nan')
    if nc > 1:
        bad['cls_branch.6.bias'][0] = float('inf')
    bad['reg_branch.4.bias'][9] = float('nan')
    bad['reg_branch.4.bias'][4] = float('-inf')
    with ctxm():
        model = model_of(params, T, L, nc, pc, 1)
        cls, box = model(bbox.to(DEV), feat.to(DEV), list(fd), None, copy.deepcopy(metas))
        per_layer = model.decoder._runtime.launches_per_layer(B, Q)
        # 6 launches a layer: the row chains; they take 1 .. 64 classes, past that the step must plan the op-by-op launches (17 or more)
        assert per_layer == 6 if how == 'default' and nc <= 64 else per_layer >= 17, (nc, how, per_layer)
        assert cls.shape == (1, B, Q, nc) and box.shape == (1, B, Q, 10) and cls.is_contiguous() and box.is_contiguous()
        assert_close('%d classes, Q=%d, %s' % (nc, Q, how), [('cls', cls, ref[0]), ('box', box, ref[1])], TOL)
        cls_n, box_n = model_of(bad, T, L, nc, pc, 1)(bbox.to(DEV), feat.to(DEV), list(fd), None, copy.deepcopy(metas))
    assert bool(torch.isfinite(cls_n).all()) and bool(torch.isfinite(box_n).all()), 'a NaN / Inf got past nan_to_num'
    big = torch.finfo(torch.float32).max
    want_cls, want_box = ref[0].float(), ref[1].float()
    want_cls[..., nc - 1] = 0.0
    if nc > 1:
        want_cls[..., 0] = big
    want_box[..., 9] = 0.0
    want_box[..., 4] = -big
    cls_n, box_n = cls_n.cpu(), box_n.cpu()
    for name, got, want, cols in (('cls', cls_n, want_cls, [0, nc - 1]), ('box', box_n, want_box, [4, 9])):
        for c in cols:
            assert torch.equal(got[..., c], want[..., c]), '%s column %d after nan_to_num: per sample %s' % (name, c, got[0, :, :, c].abs().amax(1).tolist())
            got[..., c] = 0.0
            want[..., c] = 0.0
    assert_close('%d classes, Q=%d, %s, non-finite biases' % (nc, Q, how), [('cls', cls_n, want_cls), ('box', box_n, want_box)], TOL)


# ---- the other ways of running a step, on the G14 inputs --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def g14_eager():
    """(cls, box) of the default eager step on the G14 inputs, 2 layers: what every other way of running the step must reproduce"""
    g, params, feats, metas, pc, nc = g14()
    B, Q, T, L = [int(v) for v in g['cfg']]
    qb, qf, fd = on_device(g, feats)
    out = model_of(params, T, L, nc, pc, 2)(qb, qf, list(fd), None, copy.deepcopy(metas))
    return tuple(t.clone() for t in out)


def rolled(metas, feats_dev, qb, qf, k=1):
    """the batch with its samples rotated by k: every per-sample input moves together, so the outputs must rotate with them"""
    return (qb.roll(k, 0).contiguous(), qf.roll(k, 0).contiguous(), [f.roll(k, 0).contiguous() for f in feats_dev],
            [copy.deepcopy(metas[(b - k) % len(metas)]) for b in range(len(metas))])


@gpu
def test_g14_replayed_step_with_fresh_tensors_and_rotated_samples():
    """tests/test_gpu_lazy.py's claim: lists of new tensors replay ONE captured step, bit-identical to the eager step -- here with the
    samples rotated between replays, so that a replay that kept a sample's constants from the capture gives another sample's."""
    from sparsebev_amd import runtime
    g, params, feats, metas, pc, nc = g14()
    B, Q, T, L = [int(v) for v in g['cfg']]
    qb, qf, fd = on_device(g, feats)
    want = g14_eager()
    m = model_of(params, T, L, nc, pc, 2, graph=True)
    for step in range(5):
        k = step % B
        b_in, f_in, feats_in, metas_in = rolled(metas, fd, qb, qf, k)
        got = m(b_in, f_in, feats_in, None, metas_in)
        assert_same('step %d (samples rotated by %d)' % (step, k), (got[0].roll(-k, 1), got[1].roll(-k, 1)), want)
    sg = m.decoder._runtime.step_graphs
    assert sg.captures == 1 and sg.replays == 4, (sg.captures, sg.replays)      # the first sighting runs eager, the second call captures and launches
    assert len([e for e in sg.entries.values() if isinstance(e, runtime.CapturedStep)]) == 1


@gpu
def test_g14_rotated_samples_rotate_the_eager_outputs():
    """the property the replay test leans on, on the eager step: per-sample inputs rotated together rotate the outputs bit for bit"""
    g, params, feats, metas, pc, nc = g14()
    B, Q, T, L = [int(v) for v in g['cfg']]
    qb, qf, fd = on_device(g, feats)
    want = g14_eager()
    m = model_of(params, T, L, nc, pc, 2)
    for k in (1, 2):
        b_in, f_in, feats_in, metas_in = rolled(metas, fd, qb, qf, k)
        got = m(b_in, f_in, feats_in, None, metas_in)
        assert_same('samples rotated by %d' % k, (got[0].roll(-k, 1), got[1].roll(-k, 1)), want)


@gpu
@pytest.mark.parametrize('mode', [1, 2])
def test_g14_query_order_modes(mode):
    from sparsebev_amd import runtime
    g, params, feats, metas, pc, nc = g14()
    B, Q, T, L = [int(v) for v in g['cfg']]
    qb, qf, fd = on_device(g, feats)
    want = g14_eager()
    m = model_of(params, T, L, nc, pc, 2)
    prev = runtime.query_order(False)
    try:
        runtime.query_order(True if mode == 1 else 2)
        got = m(qb, qf, list(fd), None, copy.deepcopy(metas))
        assert m.decoder._runtime.launches_per_layer(B, Q) == (7 if mode == 1 else 6)
    finally:
        runtime.query_order(prev)
    assert_same('query order mode %d' % mode, got, want)


@gpu
def test_g14_dense_relayout_instead_of_on_demand():
    from sparsebev_amd import runtime
    g, params, feats, metas, pc, nc = g14()
    B, Q, T, L = [int(v) for v in g['cfg']]
    qb, qf, fd = on_device(g, feats)
    want = g14_eager()
    prev = runtime.lazy_relayout(True)
    try:
        runtime.lazy_relayout(False)
        got = model_of(params, T, L, nc, pc, 2)(qb, qf, list(fd), None, copy.deepcopy(metas))
        got_pyr = model_of(params, T, L, nc, pc, 2)(qb, qf, FeaturePyramid(fd), None, copy.deepcopy(metas))
    finally:
        runtime.lazy_relayout(prev)
    assert_same('dense relayout', got, want)
    assert_same('dense relayout, FeaturePyramid handed over', got_pyr, want)


@gpu
@pytest.mark.parametrize('way', ['ring', 'put', 'step', 'stream'])
def test_g14_frame_ring_and_frame_pool(way):
    """the frame ring (frames pushed oldest first) and the keyed pool -- put(), step() with the newest frame, stream() with both frames --
    hold the same frames as the dense stack: bit-identical outputs (tests/test_gpu_decoder.py, test_gpu_pool*.py)"""
    from sparsebev_amd.cache import FrameFeatureCache, FramePool
    g, params, feats, metas, pc, nc = g14()
    B, Q, T, L = [int(v) for v in g['cfg']]
    qb, qf, fd = on_device(g, feats)
    want = g14_eager()
    frame = lambda t: [f[:, t * 6:(t + 1) * 6].contiguous() for f in fd]                  # list[L] of [B, 6, C, H, W], t = 0 newest
    keys = [[('s%d' % b, t) for t in range(T)] for b in range(B)]
    if way == 'ring':
        ring = FrameFeatureCache(T, n_slots=T + 1)
        for t in reversed(range(T)):
            ring.push(frame(t))
        pyr = ring.pyramid()
    else:
        pool = FramePool(T, n_slots=T + 1)
        held = {t: frame(t) for t in range(T)}
        if way == 'stream':
            pyr = pool.stream(keys, held)
        else:
            for b, k in pool.missing(keys):
                if way == 'put' or k[1] > 0:
                    pool.put(b, k, [f[b] for f in held[k[1]]])
            pyr = pool.pyramid(keys) if way == 'put' else pool.step(keys, held[0])
    got = model_of(params, T, L, nc, pc, 2)(qb, qf, pyr, None, copy.deepcopy(metas))
    assert_same(way, got, want)


@gpu
def test_g14_prefix_cache_hit():
    from sparsebev_amd import runtime
    g, params, feats, metas, pc, nc = g14()
    B, Q, T, L = [int(v) for v in g['cfg']]
    qb, qf, fd = on_device(g, feats)
    m = model_of(params, T, L, nc, pc, 2)
    runtime.prefix_cache(False)
    try:
        off = tuple(t.clone() for t in m(qb, qf, list(fd), None, copy.deepcopy(metas)))
    finally:
        runtime.prefix_cache(True)
    assert_same('cache off vs the default eager step', off, g14_eager())
    m(qb, qf, list(fd), None, copy.deepcopy(metas))
    n0 = m.decoder._runtime.prefix_counters()
    # same queries in new tensors, the samples' cameras and frames rotated under them: a hit must skip only what reads the queries alone
    _, _, feats_in, metas_in = rolled(metas, fd, qb, qf, 1)
    got = tuple(t.clone() for t in m(qb.clone(), qf.clone(), feats_in, None, metas_in))
    n1 = m.decoder._runtime.prefix_counters()
    assert (n1[0] - n0[0], n1[1] - n0[1]) == (1, 0)
    runtime.prefix_cache(False)
    try:
        want = m(qb.clone(), qf.clone(), feats_in, None, metas_in)
    finally:
        runtime.prefix_cache(True)
    assert_same('prefix cache hit under other cameras', got, want)
    assert not torch.equal(got[0], off[0])


@gpu
def test_g14_exact_gemm_mode():
    g, params, feats, metas, pc, nc = g14()
    B, Q, T, L = [int(v) for v in g['cfg']]
    qb, qf, fd = on_device(g, feats)
    m = model_of(params, T, L, nc, pc, 2)
    m.decoder.gemm_mode = 'f32'
    cls, box = m(qb, qf, list(fd), None, copy.deepcopy(metas))
    assert_close('G14 gemm mode f32, layer 0 vs the recording', [('cls', cls[0], g['out_cls'][0]), ('box', box[0], g['out_bbox'][0])], TOL)
    ref = g14_oracle()
    assert_close('G14 gemm mode f32, layer 0 vs the oracle', [('cls', cls[0], ref[0][0]), ('box', box[0], ref[1][0])], TOL)


# ---- head --------------------------------------------------------------------------------------------------------------------------

@gpu
def test_head_seven_classes_asymmetric_range_per_sample_metas_vs_oracle():
    """tests/test_gpu_head.py::test_head_module_end_to_end_vs_oracle with 7 classes, the asymmetric pc_range in transformer and coder
    and per-sample metas at B = 3: scores to 1e-4, boxes in metres to 1e-4 x the largest span of the range (102.4 m: that test's 1e-3 is
    this rule rounded), labels equal, the decode step equal to the oracle's on the device tensors.  Measured 9.5e-7 / 1.5e-5 m."""
    from sparsebev_amd import head as H
    T, L, Q, B, nc, pc = 2, 4, 36, 3, 7, S.PC_RANGE_ASYM
    post = [-50.0, -71.2, -10.0, 72.4, 51.2, 10.0]
    ih, iw, sizes = S.PYRAMIDS['tiny']
    head = H.SparseBEVHead(num_classes=nc, in_channels=256, num_query=Q, code_size=10,
                           transformer=dict(type='SparseBEVTransformer', embed_dims=256, num_frames=T, num_points=4, num_layers=2,
                                            num_levels=L, num_classes=nc, code_size=10, pc_range=pc),
                           bbox_coder=dict(type='NMSFreeCoder', post_center_range=post, max_num=30, score_threshold=None,
                                           num_classes=nc, pc_range=pc))
    assert tuple(head.label_enc.weight.shape) == (nc + 1, 255)
    params = S.make_params(81, embed_dims=256, num_frames=T, num_points=4, num_levels=L, num_classes=nc)
    head.transformer.load_state_dict({PREFIX + k: v for k, v in params.items()}, strict=True)
    with torch.no_grad():
        head.init_query_bbox.weight[:, 2] = 0.5            # lift the grid so that the cameras see it
        head.init_query_bbox.weight[:, 5] = 0.5
        gen = torch.Generator().manual_seed(82)            # every row of the label embedding its own: row num_classes is the one to read
        head.label_enc.weight.copy_(torch.randn(nc + 1, 255, generator=gen))
    head = head.to(DEV).eval()
    feats = S.make_features(B, T, sizes, seed=83)
    metas = S.make_img_metas_per_sample(B, T, ih, iw)
    outs = head([f.to(DEV) for f in feats], copy.deepcopy(metas))
    assert outs['all_cls_scores'].shape == (2, B, Q, nc) and outs['all_bbox_preds'].shape == (2, B, Q, 10)
    qb, qf = O.head_prepare(head.init_query_bbox.weight.cpu(), head.label_enc.weight.cpu(), nc, B)
    cls, box, _ = O.decoder(params, qb, qf, feats, metas, pc, num_layers=2)
    box = O.head_postprocess(box, pc)
    span = max(pc[3] - pc[0], pc[4] - pc[1], pc[5] - pc[2])
    assert_close('head scores, layer 0', [('cls', outs['all_cls_scores'][0], cls[0])], TOL)
    assert_close('head boxes in metres, layer 0', [('box', outs['all_bbox_preds'][0], box[0])], TOL * span)
    res = head.get_bboxes(outs, metas)
    assert len(res) == B and all(r[0].shape[1] == 9 and r[0].shape[0] == r[1].shape[0] == r[2].shape[0] for r in res)
    ref = O.get_bboxes(O.nms_free_decode(outs['all_cls_scores'].cpu(), outs['all_bbox_preds'].cpu(), nc, 30, None, post))
    assert sum(r[0].shape[0] for r in ref) > 0
    for b, ((rb, rs, rl), (bb, ss, ll)) in enumerate(zip(ref, res)):
        assert torch.equal(ll.cpu(), rl), 'labels of sample %d' % b
        assert int(rl.max()) < nc
        if rl.numel():
            assert (ss.cpu() - rs).abs().max() < 1e-6 and (bb.cpu() - rb).abs().max() < 2e-5, 'decode of sample %d' % b


# ---- training ------------------------------------------------------------------------------------------------------------------------

@gpu
@torch.enable_grad()
@pytest.mark.parametrize('mode', ['f16x3', 'f32'])
def test_one_layer_trained_with_per_sample_metas_seven_classes_vs_oracle_autograd(mode):
    """One layer, forward + backward, B = 3 x 36, T = 2, 7 classes, per-sample metas, asymmetric range, against the fp64 oracle under
    autograd with the recipe and the bounds of test_one_layer_trained_at_the_trainval_shapes_vs_oracle_autograd; then once per sample
    with the cotangents of the other samples zeroed: the gradient of reg_branch.4's rows 8 - 9 (the velocity columns, divided by
    vel_div[b]) to the recipe's 1e-5 for tensors downstream of every decision, and the gradient of sample b's feature maps (reached
    through lidar2img[b]) norm-wise to 5e-3 and max-abs to 5e-2 -- 1e-4 when no mixing ReLU input lies within fp32 reach of zero -- with
    the other samples' feature-map gradients exactly zero.  Measured (63 mixing ReLU inputs within 1e-5 of zero): outputs 5.4e-7, downstream
    6.8e-7, worst l2 2.9e-3, worst max-abs 2.7e-2; per sample rows 8 - 9 8.3e-7, feature maps 2.7e-2 max-abs."""
    from test_gpu_backward import rel
    from test_gpu_backward_shapes import TrainedLayer, _one_layer_trained_vs_oracle, rel_l2
    B, Q, T, nc = 3, 36, 2, 7
    ih, iw, _ = S.PYRAMIDS['tiny']
    case = TrainedLayer(B, Q, T, 'tiny', 4, mode, False, 700, metas=S.make_img_metas_per_sample(B, T, ih, iw), num_classes=nc,
                        pc_range=S.PC_RANGE_ASYM)
    mix_near = _one_layer_trained_vs_oracle(case, 'asym')
    worst = []
    for b in range(B):
        keep = torch.zeros(1, B, 1, 1)
        keep[0, b] = 1.0
        _, _, got = case.device(case.cc * keep, case.cb * keep)
        _, _, want = case.oracle(case.cc * keep, case.cb * keep)
        got, want = dict(got), dict(want)
        for name in ('reg_branch.4.weight', 'reg_branch.4.bias'):
            e = rel(got[name][8:10], want[name][8:10])
            worst.append((e, b, name + '[8:10]'))
            assert e < 1e-5, 'sample %d: gradient of %s rows 8-9 off by %.2e (relative)' % (b, name, e)
        for l in range(case.L):
            a, r = got['feat%d' % l], want['feat%d' % l]
            others = [i for i in range(B) if i != b]
            assert float(a[others].abs().max()) == 0.0 and float(r[others].abs().max()) == 0.0, 'sample %d reached another sample\'s feature maps (level %d)' % (b, l)
            e2, em = rel_l2(a[b], r[b]), rel(a[b], r[b])
            worst.append((em, b, 'feat%d' % l))
            assert e2 < 5e-3 and em < (1e-4 if mix_near == 0 else 5e-2), 'sample %d: feature-map gradient, level %d: l2 %.2e max-abs %.2e' % (b, l, e2, em)
    print('per-sample gradients (%s): %s' % (mode, ' '.join('%d:%s=%.1e' % (b, n, e) for e, b, n in worst)))
