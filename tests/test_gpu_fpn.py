"""FPNNeck on the device against the fp64 restatement of its definition (fpn_cases.py).  Every case runs with fp16 and fp32 inputs and
fp16 and fp32 outputs, into NaN-filled destinations.  Integers make the structural test exact (torch.equal); real-valued data is held
stage by stage against fp64 on the device's own previous stage, inside the worst-case fp32 accumulation bound; then the operands'
rounding, the weight pack's version key, capture, and the hand-over to FeaturePyramid, FramePool.stream and a decoder step."""
import ctypes
import functools

import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

import fpn_cases as FC  # noqa: E402
from sparsebev_amd import _lib  # noqa: E402

DEV = 'cuda:0'
F16, F32 = torch.float16, torch.float32
DTYPES = [(F16, F16), (F16, F32), (F32, F16), (F32, F32)]
DTYPE_IDS = ['in16_out16', 'in16_out32', 'in32_out16', 'in32_out32']
CASE_IDS = [c.name for c in FC.CASES]


@functools.lru_cache(maxsize=None)
def integer_case(name):
    """integer data and its fp64 restatement, computed once per case and never written to"""
    case = FC.BY_NAME[name]
    xs, params = FC.integer_data(case, seed=11)
    M, P = FC.reference(xs, params, case.num_outs)
    return xs, params, M, P


@functools.lru_cache(maxsize=None)
def real_case(name):
    case = FC.BY_NAME[name]
    return FC.real_data(case, seed=5)


def device_inputs(xs, dtype):
    return [FC.channels_last(x.to(device=DEV, dtype=dtype)) for x in xs]


def assert_layout(case, got, out):
    for g, o, (h, w) in zip(got, out, FC.out_planes(case)):
        assert g.data_ptr() == o.data_ptr() and tuple(g.shape) == (case.n, 256, h, w)
        assert g.permute(0, 2, 3, 1).is_contiguous()


# ---- 1. exact on integers ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('in_dtype,out_dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('name', CASE_IDS)
def test_exact_on_integers(name, in_dtype, out_dtype):
    case = FC.BY_NAME[name]
    xs, params, M, P = integer_case(name)
    # the premises of exactness, on the CPU first: every merged lateral is an fp16 integer, every output an fp32 integer
    assert max(float(m.abs().max()) for m in M) < 2 ** 11 and max(float(p.abs().max()) for p in P) < 2 ** 24
    assert all(torch.equal(m, m.round()) for m in M) and max(float(p.abs().max()) for p in P) > 2 ** 11
    neck = FC.make_neck(case, params, DEV)
    out = FC.nan_outputs(case, out_dtype, DEV)
    got = neck(device_inputs(xs, in_dtype), out=out)
    assert_layout(case, got, out)
    assert len(neck.merged) == len(xs) and len(got) == case.num_outs
    for l, (m, want) in enumerate(zip(neck.merged, M)):
        assert m.dtype == F16 and torch.equal(m.cpu().double(), want), 'M%d' % l
    for o, (g, want) in enumerate(zip(got, P)):
        assert g.dtype == out_dtype
        want = want.half() if out_dtype == F16 else want.float()
        assert torch.equal(g.cpu(), want), 'P%d' % o


# ---- 2. real-valued data, stage by stage ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('in_dtype,out_dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('name', CASE_IDS)
def test_real_data_stage_by_stage(name, in_dtype, out_dtype):
    """Bounds (fpn_cases.stage_errors): |got - s| <= 2^-11 |s| + 2^-25 + (K + 4) 2^-23 A for a merged lateral and an fp16 output, the last
    term alone for an fp32 output; s = fp64 on the device's own previous stage, A = sum of absolute products + |bias| (+ |parent|).  The
    worst case of fp32 accumulation, with a factor 2 for additions inside the matrix core that do not round to nearest: loose by
    construction, it guards scale, bias and rounding; structure is test 1's."""
    case = FC.BY_NAME[name]
    xs, params = real_case(name)
    neck = FC.make_neck(case, params, DEV)
    rows = FC.stage_errors(neck, case, xs, params, in_dtype, out_dtype, DEV)
    for r in rows:
        print('%-6s %s -> %s  %-3s max %.3e rms %.3e  error / bound %.4f' % (name, in_dtype, out_dtype, r['stage'], r['max'], r['rms'], r['ratio']))
    for r in rows:
        assert r['finite'] and r['ratio'] <= 1.0, r


# ---- 3. fp32 operands are rounded to nearest even ------------------------------------------------------------------------------------

@pytest.mark.parametrize('out_dtype', [F16, F32], ids=['out16', 'out32'])
@pytest.mark.parametrize('name', ['tiny', 'edges'])
def test_fp32_inputs_round_to_nearest_even(name, out_dtype):
    case = FC.BY_NAME[name]
    xs, params = real_case(name)
    xs = [x.clone() for x in xs]
    ties = torch.tensor([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2.0 ** -25, 3 * 2.0 ** -25, 65519.0, 2.0 ** -14 + 2.0 ** -25])
    for x in xs:                                  # exact ties, the smallest subnormal's, and the last value below the overflow threshold
        x.view(-1)[:len(ties)] = ties
    assert not torch.equal(xs[0].half().float(), xs[0])
    neck = FC.make_neck(case, params, DEV)
    a = [t.clone() for t in neck(device_inputs(xs, F32), out=FC.nan_outputs(case, out_dtype, DEV))]
    ma = [m.clone() for m in neck.merged]
    b = neck(device_inputs([x.half() for x in xs], F16), out=FC.nan_outputs(case, out_dtype, DEV))
    for l, (p, q) in enumerate(zip(ma, neck.merged)):
        assert torch.equal(p, q) and bool(torch.isfinite(p).all()), 'M%d' % l
    for o, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(p, q) and bool(torch.isfinite(p).all()), 'P%d' % o


# ---- 4. the pack follows the weights -------------------------------------------------------------------------------------------------

def test_weights_move():
    case = FC.BY_NAME['tiny']
    xs, params, M, P = integer_case('tiny')
    neck = FC.make_neck(case, params, DEV)
    inputs = device_inputs(xs, F16)
    got = neck(inputs, out_dtype=F32)
    assert all(torch.equal(g.cpu(), p.float()) for g, p in zip(got, P))
    image = neck.pack()
    assert neck.pack() is image                                   # nothing changed: no repack
    before = image.clone()
    # an optimizer's kind of write (in place) ...
    neck.fpn_convs[0].conv.weight.mul_(2)
    neck.lateral_convs[3].conv.weight.neg_()
    neck.fpn_convs[1].conv.bias.add_(1)                           # (biases are read where they are)
    moved = {k: v.clone() for k, v in params.items()}
    moved['fpn_convs.0.conv.weight'] *= 2
    moved['lateral_convs.3.conv.weight'] *= -1
    moved['fpn_convs.1.conv.bias'] += 1
    M2, P2 = FC.reference(xs, moved, case.num_outs)
    assert max(float(m.abs().max()) for m in M2) < 2 ** 11 and max(float(p.abs().max()) for p in P2) < 2 ** 24
    got = neck(inputs, out_dtype=F32)
    assert not torch.equal(neck.pack(), before)
    assert neck.pack().data_ptr() == image.data_ptr()             # repacked in place: an already captured forward reads the new image
    assert all(torch.equal(m.cpu().double(), w) for m, w in zip(neck.merged, M2))
    assert all(torch.equal(g.cpu(), p.float()) for g, p in zip(got, P2))
    assert not torch.equal(P2[0], P[0]) and not torch.equal(M2[0], M[0])
    # ... and load_state_dict
    neck.load_state_dict(params, strict=True)
    got = neck(inputs, out_dtype=F32)
    assert all(torch.equal(g.cpu(), p.float()) for g, p in zip(got, P))


# ---- 5. capture ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['tiny', 'five'])
def test_capture_and_replay(name):
    """one forward captured with out=: L + 1 kernel nodes (the extra level rides in the convolution launch), no allocation in the call;
    a replay after the inputs were overwritten in place equals the eager call bit for bit"""
    case = FC.BY_NAME[name]
    xs, params = real_case(name)
    xs2, _ = FC.real_data(case, seed=6)
    lib = _lib.load()
    neck = FC.make_neck(case, params, DEV)
    inputs = device_inputs(xs, F32)
    out = FC.nan_outputs(case, F16, DEV)
    neck(inputs, out=out)                                         # packs, allocates the workspace
    torch.cuda.synchronize()
    allocs = torch.cuda.memory_stats(DEV)['allocation.all.allocated']
    neck(inputs, out=out)
    assert torch.cuda.memory_stats(DEV)['allocation.all.allocated'] == allocs
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    handle = ctypes.c_void_p()
    with torch.cuda.stream(side):
        sp = ctypes.c_void_p(side.cuda_stream)
        _lib.check(lib.sbev_capture_begin(sp), 'sbev_capture_begin')
        try:
            neck(inputs, out=out)
        finally:
            st = lib.sbev_capture_end(sp, ctypes.byref(handle))
        _lib.check(st, 'sbev_capture_end')
    torch.cuda.current_stream().wait_stream(side)
    try:
        assert lib.sbev_graph_num_nodes(handle) == len(xs) + 1
        for x, new in zip(inputs, xs2):                           # new values at the captured addresses
            x.copy_(new.to(DEV))
        for o in out:
            o.fill_(float('nan'))
        _lib.check(lib.sbev_graph_launch(handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'sbev_graph_launch')
        torch.cuda.synchronize()
        replayed = [o.clone() for o in out]
        merged = [m.clone() for m in neck.merged]
    finally:
        lib.sbev_graph_destroy(handle)
    eager = neck(device_inputs(xs2, F32), out=FC.nan_outputs(case, F16, DEV))
    assert all(torch.equal(a, b) and bool(torch.isfinite(a).all()) for a, b in zip(replayed, eager))
    assert all(torch.equal(a, b) for a, b in zip(merged, neck.merged))
    with pytest.raises(RuntimeError, match='not packed'):         # a capture may not pack: stale weights are refused there
        neck.lateral_convs[0].conv.weight.mul_(2)
        with torch.cuda.stream(side):
            _lib.check(lib.sbev_capture_begin(ctypes.c_void_p(side.cuda_stream)), 'sbev_capture_begin')
            try:
                neck(inputs, out=out)
            finally:
                lib.sbev_capture_end(ctypes.c_void_p(side.cuda_stream), None)


# ---- 6. hand-over --------------------------------------------------------------------------------------------------------------------

def tiny_pyramid_neck(n, seed, out_dtype):
    """the neck over the smallest pyramid sparsebev_amd.synthetic offers, n images: outputs [n, 256, H, W]"""
    from sparsebev_amd import synthetic as S
    sizes = S.PYRAMIDS['tiny'][2]
    case = FC.Case('pyr', n, list(sizes), [32, 64, 96, 128], len(sizes), '')
    xs, params = FC.real_data(case, seed)
    neck = FC.make_neck(case, params, DEV)
    return neck(device_inputs(xs, F16), out_dtype=out_dtype), sizes


def test_feature_pyramid_takes_the_outputs_in_place():
    from sparsebev_amd.transformer import FeaturePyramid
    B, T = 2, 2
    outs, sizes = tiny_pyramid_neck(B * T * 6, 31, F32)
    feats = [o.view(B, T * 6, 256, h, w) for o, (h, w) in zip(outs, sizes)]
    pyr = FeaturePyramid(feats)
    assert pyr.copied == 0
    assert all(level.data_ptr() == o.data_ptr() for level, o in zip(pyr.levels, outs))


def test_frame_pool_stream_lets_the_outputs_travel():
    from sparsebev_amd.cache import FramePool
    from sparsebev_amd.utils import FrameInsert
    B, T = 2, 2
    for dtype in (F16, F32):
        outs, sizes = tiny_pyramid_neck(B * 6, 32, dtype)
        frames = [o.view(B, 6, 256, h, w) for o, (h, w) in zip(outs, sizes)]
        pool = FramePool(T, n_slots=4)
        keys = [[(b, 0)] * T for b in range(B)]
        pyr = pool.stream(keys, {0: frames})
        assert isinstance(pyr.insert, FrameInsert) and pyr.insert.nhwc is True          # no eager store: the frames travel
        assert all(f.data_ptr() == o.data_ptr() for f, o in zip(pyr.insert.frames, outs))
        pyr.materialise()
        for buf, o in zip(pool.buffers, outs):
            for b in range(B):
                slot = int(pool.slot_table[b, 0])
                assert torch.equal(buf[b, slot], o.view(B, 6, 256, *o.shape[2:])[b].permute(0, 2, 3, 1).float())


def test_decoder_step_on_the_outputs_equals_nchw_copies():
    from sparsebev_amd import synthetic as S
    from sparsebev_amd.transformer import SparseBEVTransformer
    B, T, Q = 1, 2, 49
    ih, iw, sizes = S.PYRAMIDS['tiny']
    outs, _ = tiny_pyramid_neck(B * T * 6, 33, F32)
    params = S.make_params(3, embed_dims=256, num_frames=T, num_points=4, num_levels=len(sizes))
    m = SparseBEVTransformer(256, num_frames=T, num_points=4, num_layers=2, num_levels=len(sizes), num_classes=10, code_size=10, pc_range=S.PC_RANGE)
    m.load_state_dict({'decoder.decoder_layer.' + k: v for k, v in params.items()}, strict=True)
    m = m.to(DEV).eval()
    m.decoder.static_graph = False
    bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=4)]
    metas = S.make_img_metas(B, T, ih, iw)
    views = [o.view(B, T * 6, 256, h, w) for o, (h, w) in zip(outs, sizes)]
    copies = [v.contiguous() for v in views]
    assert all(c.is_contiguous() and not v.is_contiguous() for c, v in zip(copies[:1], views[:1]))
    got = m(bbox, feat, views, None, metas)
    want = m(bbox, feat, copies, None, metas)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool(torch.isfinite(got[0]).all()) and float(got[0].abs().max()) > 0
