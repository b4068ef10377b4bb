"""The FPN neck's backward on the device against the fp64 restatement of its definition (fpn_bwd_cases.py).  Integers make the structural
test exact (torch.equal) for every case, input dtype and gradient dtype, through the C entry into NaN-filled destinations; then the
scale's invariance, zero and non-finite gradients, real-valued data stage by stage against fp64 on the device's own previous stage,
autograd (accumulation, two forwards in flight, the repack after an optimizer step), capture, and a decoder step behind the neck."""
import ctypes
import functools

import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

import fpn_bwd_cases as BC  # noqa: E402
import fpn_cases as FC  # noqa: E402
from sparsebev_amd import _lib  # noqa: E402

DEV = 'cuda:0'
F16, F32 = torch.float16, torch.float32
DTYPES = [(F16, F16), (F16, F32), (F32, F16), (F32, F32)]
DTYPE_IDS = ['in16_g16', 'in16_g32', 'in32_g16', 'in32_g32']
CASE_IDS = [c.name for c in FC.CASES]


@functools.lru_cache(maxsize=None)
def integer_case(name):
    """integer data, integer output gradients and both restatements, computed once per case and never written to"""
    case = FC.BY_NAME[name]
    xs, params = FC.integer_data(case, seed=11)
    M, _ = FC.reference(xs, params, case.num_outs)
    gP = BC.integer_grads(case, seed=12)
    return xs, params, M, gP, BC.backward_reference(xs, params, M, gP)


@functools.lru_cache(maxsize=None)
def real_case(name):
    case = FC.BY_NAME[name]
    xs, params = FC.real_data(case, seed=5)
    return xs, params, BC.real_grads(case, seed=8)


def assert_premises(case, xs, M, ref):
    """what makes the integer test exact, on the restatement: scaled lateral gradients are integers of magnitude <= 2^11, and every
    weight-gradient sum -- any partial of it included: the sum of the absolute products -- stays below 2^24 in the scaled domain"""
    assert ref['e'] == 2
    for l, (g, gm) in enumerate(zip(ref['g'], ref['gM'])):
        assert torch.equal(gm, gm.round()) and float(gm.abs().max()) <= 2 ** 11 and float(gm.abs().max()) > 0, l
        assert float(BC.weight_grad3(g, M[l])[1].max()) < 2 ** 24, l
        assert float(torch.einsum('nohw,nchw->oc', gm.abs(), xs[l].double().abs()).max()) < 2 ** 24, l
        assert float(gm.abs().sum((0, 2, 3)).max()) < 2 ** 24 and float(g.abs().sum((0, 2, 3)).max()) < 2 ** 24, l


def assert_equal_to_reference(run, ref, in_dtype, factor=1.0):
    want = BC.param_grads(ref)
    for k, g in run.grads.items():
        assert g.dtype == F32 and torch.equal(g.cpu().view(want[k].shape), (want[k] * factor).float()), k
    if run.gC is not None:
        for l, g in enumerate(run.gC):
            assert g.dtype == in_dtype and g.permute(0, 2, 3, 1).is_contiguous()
            assert torch.equal(g.cpu(), (ref['gC'][l] * factor).to(in_dtype)), 'gC%d' % l


# ---- 1. exact on integers ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('in_dtype,g_dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('name', CASE_IDS)
def test_exact_on_integers(name, in_dtype, g_dtype):
    case = FC.BY_NAME[name]
    xs, params, M, gP, ref = integer_case(name)
    assert_premises(case, xs, M, ref)
    neck = BC.make_trainable_neck(case, params, DEV)
    run = BC.DeviceBackward(neck, case, xs, gP, in_dtype, g_dtype, DEV)
    assert run.scale() == (2.0 ** ref['e'], 2.0 ** -ref['e'])
    for l in range(len(xs)):
        assert torch.equal(run.stage('gM', l).double(), ref['gM'][l]), 'gM%d' % l
        if l > 0:
            assert torch.equal(run.stage('D', l).double(), ref['D'][l]), 'D%d' % l
    assert_equal_to_reference(run, ref, in_dtype)
    # without input gradients: the same parameter gradients
    lean = BC.DeviceBackward(neck, case, xs, gP, in_dtype, g_dtype, DEV, input_grads=False)
    assert all(torch.equal(a, b) for a, b in zip(lean.grads.values(), run.grads.values()))


# ---- 2. the scale ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('g_dtype', [F16, F32], ids=['g16', 'g32'])
@pytest.mark.parametrize('name', ['tiny', 'five'])
def test_scale_invariance(name, g_dtype):
    """the output gradients times 2^-20 and 2^10: e moves by 20 and -10, every scaled operand is the same, the fp32 parameter gradients
    are exactly the power of two times the unscaled run's"""
    case = FC.BY_NAME[name]
    xs, params, M, gP, ref = integer_case(name)
    neck = BC.make_trainable_neck(case, params, DEV)
    for k in (-20, 10):
        run = BC.DeviceBackward(neck, case, xs, [g * 2.0 ** k for g in gP], F32, g_dtype, DEV)
        assert run.scale() == (2.0 ** (ref['e'] - k), 2.0 ** (k - ref['e']))
        assert_equal_to_reference(run, ref, F32, factor=2.0 ** k)
        assert float(run.grads['fpn_convs.0.conv.weight'].abs().max()) > 0


def test_zero_and_non_finite_gradients():
    case = FC.BY_NAME['tiny']
    xs, params, M, gP, ref = integer_case('tiny')
    neck = BC.make_trainable_neck(case, params, DEV)
    run = BC.DeviceBackward(neck, case, xs, [torch.zeros_like(g) for g in gP], F16, F32, DEV)
    assert run.scale() == (1.0, 1.0)
    assert all(bool((g == 0).all()) for g in list(run.grads.values()) + run.gC)
    bad = [g.clone() for g in gP]
    bad[0][1, 7, 2, 3] = float('inf')
    run = BC.DeviceBackward(neck, case, xs, bad, F16, F32, DEV)
    assert run.scale() == (1.0, 1.0)
    assert not bool(torch.isfinite(run.grads['fpn_convs.0.conv.bias']).all())
    assert not bool(torch.isfinite(run.grads['fpn_convs.0.conv.weight']).all())
    assert not bool(torch.isfinite(run.grads['lateral_convs.0.conv.bias']).all())


# ---- 3. real-valued data, stage by stage -----------------------------------------------------------------------------------------------

def stage_rows(run, case, xs, params, gP, in_dtype, g_dtype):
    """Every stage against fp64 on the DEVICE's own previous stage, operands rounded as the definition says.  Bounds, in the scaled
    domain (K = reduction length, A = sum of absolute products): fp16 results 2^-11 |s| + 2^-25 + (K + 4) 2^-23 A, fp32 results the
    last term alone.  Returns (stage, error / bound) pairs."""
    L = len(xs)
    up, down = run.scale()
    e = BC.scale_exponent([g.to(g_dtype).float() for g in gP])
    assert up == 2.0 ** e and down == 2.0 ** -e
    g = BC.staged_grads([t.to(g_dtype).float() for t in gP], L, e)
    rows = []

    def row(name, got, s, A, K, rounding):
        bound = (K + 4) * 2.0 ** -23 * A
        if rounding:
            bound = bound + 2.0 ** -11 * s.abs() + 2.0 ** -25
        assert bool(torch.isfinite(got).all()), name
        rows.append((name, float(((got.double() - s).abs() / bound.clamp_min(1e-300)).max())))

    merged = [m.cpu() for m in run.merged]
    x16 = [x.to(in_dtype).half().double() for x in xs]
    for l in range(L):
        s, A = BC.data_grad3(g[l], params['fpn_convs.%d.conv.weight' % l])
        gm = run.stage('gM', l)
        if l == 0:
            row('gM0', gm, s, A, 9 * 256, True)
        else:
            d = run.stage('D', l)
            row('D%d' % l, d, s, A, 9 * 256, False)
            cs, ca, most = BC.children_sum(run.stage('gM', l - 1), d.shape[2], d.shape[3])
            row('gM%d' % l, gm, d.double() + cs, d.double().abs() + ca, most + 1, True)
        gm = gm.double()
        wl = params['lateral_convs.%d.conv.weight' % l].half().double()[:, :, 0, 0]
        # the data gradient is rounded to the inputs' dtype AFTER the multiplication by 2^-e: the bound is taken in the unscaled domain
        row('gC%d' % l, run.gC[l].cpu(), down * torch.einsum('nohw,oc->nchw', gm, wl), down * torch.einsum('nohw,oc->nchw', gm.abs(), wl.abs()),
            256, in_dtype == F16)
        pixels = case.n * case.planes[l][0] * case.planes[l][1]
        s, A = BC.weight_grad3(g[l], merged[l])
        row('gW3_%d' % l, run.gw3[l].cpu() * up, s, A, pixels, False)
        row('gWlat%d' % l, run.gwl[l].cpu()[:, :, 0, 0] * up, torch.einsum('nohw,nchw->oc', gm, x16[l]),
            torch.einsum('nohw,nchw->oc', gm.abs(), x16[l].abs()), pixels, False)
        row('gc%d' % l, run.gb3[l].cpu() * up, g[l].sum((0, 2, 3)), g[l].abs().sum((0, 2, 3)), pixels, False)
        row('gblat%d' % l, run.gbl[l].cpu() * up, gm.sum((0, 2, 3)), gm.abs().sum((0, 2, 3)), pixels, False)
    return rows


@pytest.mark.parametrize('in_dtype,g_dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('name', CASE_IDS)
def test_real_data_stage_by_stage(name, in_dtype, g_dtype):
    """The forward tests' worst-case bound, |got - s| <= 2^-11 |s| + 2^-25 + (K + 4) 2^-23 A (the first two terms dropped for fp32
    results), K = 9 x 256, 256, the pixel count of the level, or the child count + 1: loose by construction, it guards the scale, the
    operand roundings and the slab fold; structure is test 1's."""
    case = FC.BY_NAME[name]
    xs, params, gP = real_case(name)
    neck = BC.make_trainable_neck(case, params, DEV)
    run = BC.DeviceBackward(neck, case, xs, gP, in_dtype, g_dtype, DEV)
    rows = stage_rows(run, case, xs, params, gP, in_dtype, g_dtype)
    worst = {}
    for stage, ratio in rows:
        key = stage.rstrip('0123456789_')
        worst[key] = max(worst.get(key, 0.0), ratio)
    print('STAGES %s %s %s' % (name, DTYPE_IDS[DTYPES.index((in_dtype, g_dtype))], ' '.join('%s=%.4f' % kv for kv in sorted(worst.items()))))
    for stage, ratio in rows:
        assert ratio <= 1.0, (stage, ratio)


# ---- 4. through autograd ---------------------------------------------------------------------------------------------------------------

def autograd_run(neck, xs, R, in_dtype, out_dtype, input_grads):
    inputs = [FC.channels_last(x.to(device=DEV, dtype=in_dtype)).requires_grad_(input_grads) for x in xs]
    outs = neck(inputs, out_dtype=out_dtype)
    loss = sum((o.float() * r.float()).sum() for o, r in zip(outs, R))
    return inputs, outs, loss


@torch.enable_grad()
@pytest.mark.parametrize('in_dtype,out_dtype', [(F16, F16), (F32, F32)], ids=['f16', 'f32'])
@pytest.mark.parametrize('name', ['tiny', 'five'])
def test_through_autograd(name, in_dtype, out_dtype):
    case = FC.BY_NAME[name]
    xs, params, gP = real_case(name)
    neck = BC.make_trainable_neck(case, params, DEV)
    R = [FC.channels_last(g.to(device=DEV, dtype=out_dtype)) for g in gP]
    direct = BC.DeviceBackward(neck, case, xs, gP, in_dtype, out_dtype, DEV)
    inputs, outs, loss = autograd_run(neck, xs, R, in_dtype, out_dtype, True)
    with torch.no_grad():
        plain = neck([x.detach() for x in inputs], out_dtype=out_dtype)
    assert all(o.dtype == out_dtype and o.permute(0, 2, 3, 1).is_contiguous() and torch.equal(o, p) for o, p in zip(outs, plain))
    loss.backward()
    named = dict(neck.named_parameters())
    assert len(named) == 4 * len(xs)
    for k, g in direct.grads.items():
        assert named[k].grad is not None and named[k].grad.dtype == F32 and torch.equal(named[k].grad, g), k
    for x, g in zip(inputs, direct.gC):
        assert x.grad.dtype == in_dtype and torch.equal(x.grad, g)
    # a second backward accumulates, as autograd does
    inputs2, _, loss2 = autograd_run(neck, xs, R, in_dtype, out_dtype, False)
    loss2.backward()
    assert all(x.grad is None for x in inputs2)
    for k, g in direct.grads.items():
        assert torch.equal(named[k].grad, g + g), k


@torch.enable_grad()
def test_two_forwards_then_two_backwards():
    case = FC.BY_NAME['edges']
    xs, params, gP = real_case('edges')
    xs2, _ = FC.real_data(case, seed=6)
    neck = BC.make_trainable_neck(case, params, DEV)
    R = [FC.channels_last(g.to(DEV)) for g in gP]
    alone = []
    for data in (xs, xs2):
        neck.zero_grad(set_to_none=True)
        inputs, _, loss = autograd_run(neck, data, R, F32, F32, True)
        loss.backward()
        alone.append(([x.grad.clone() for x in inputs], {k: p.grad.clone() for k, p in neck.named_parameters()}))
    neck.zero_grad(set_to_none=True)
    in_a, _, loss_a = autograd_run(neck, xs, R, F32, F32, True)
    in_b, _, loss_b = autograd_run(neck, xs2, R, F32, F32, True)         # the second forward must not clobber the first's merged laterals
    loss_a.backward()
    got_a = {k: p.grad.clone() for k, p in neck.named_parameters()}
    neck.zero_grad(set_to_none=True)
    loss_b.backward()
    got_b = {k: p.grad.clone() for k, p in neck.named_parameters()}
    for (gx, gp), ins, got in ((alone[0], in_a, got_a), (alone[1], in_b, got_b)):
        assert all(torch.equal(x.grad, g) for x, g in zip(ins, gx))
        assert all(torch.equal(got[k], gp[k]) for k in gp)
    assert not torch.equal(got_a['fpn_convs.0.conv.weight'], got_b['fpn_convs.0.conv.weight'])


@torch.enable_grad()
def test_optimizer_step_repacks_both_images():
    from sparsebev_amd import optim
    case = FC.BY_NAME['tiny']
    xs, params, gP = real_case('tiny')
    neck = BC.make_trainable_neck(case, params, DEV)
    R = [FC.channels_last(g.to(DEV)) for g in gP]
    opt = optim.FusedAdamW(list(neck.parameters()), lr=1e-2)
    _, outs, loss = autograd_run(neck, xs, R, F32, F32, False)
    before = [o.detach().clone() for o in outs]
    images = neck.pack().clone(), neck.pack_bwd().clone()
    at = neck.pack().data_ptr(), neck.pack_bwd().data_ptr()
    loss.backward()
    opt.step()
    neck.zero_grad(set_to_none=True)
    _, outs, loss = autograd_run(neck, xs, R, F32, F32, False)
    assert not torch.equal(neck.pack(), images[0]) and not torch.equal(neck.pack_bwd(), images[1])
    assert (neck.pack().data_ptr(), neck.pack_bwd().data_ptr()) == at          # both repacked in place
    assert not any(torch.equal(o, b) for o, b in zip(outs, before))
    loss.backward()
    moved = {k: v.detach().cpu() for k, v in neck.state_dict().items()}
    assert not torch.equal(moved['fpn_convs.1.conv.weight'], params['fpn_convs.1.conv.weight'])
    # the gradients on the new weights: bit-equal to the C entry's, which is held stage by stage against the restatement on them
    direct = BC.DeviceBackward(neck, case, xs, gP, F32, F32, DEV)
    for k, p in neck.named_parameters():
        assert torch.equal(p.grad, direct.grads[k]), k
    for stage, ratio in stage_rows(direct, case, xs, moved, gP, F32, F32):
        assert ratio <= 1.0, (stage, ratio)


# ---- 5. capture ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['tiny', 'five'])
def test_capture_and_replay(name):
    """sbev_fpn_backward captured into preallocated buffers: 5 L + 1 kernel nodes and the memset node; a replay after inputs, merged
    laterals and output gradients were overwritten in place equals the eager call bit for bit (the scale is read on the device)"""
    case = FC.BY_NAME[name]
    xs, params, gP = real_case(name)
    xs2, _ = FC.real_data(case, seed=6)
    gP2 = BC.real_grads(case, seed=9, scale=2.0 ** -9)
    lib = _lib.load()
    neck = BC.make_trainable_neck(case, params, DEV)
    run = BC.DeviceBackward(neck, case, xs, gP, F32, F32, DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    handle = ctypes.c_void_p()
    with torch.cuda.stream(side):
        sp = ctypes.c_void_p(side.cuda_stream)
        _lib.check(lib.sbev_capture_begin(sp), 'sbev_capture_begin')
        try:
            run.run(sp)
        finally:
            st = lib.sbev_capture_end(sp, ctypes.byref(handle))
        _lib.check(st, 'sbev_capture_end')
    torch.cuda.current_stream().wait_stream(side)
    try:
        assert lib.sbev_graph_num_nodes(handle) == run.plan['launches'] + 1 == 5 * len(xs) + 2
        eager = BC.DeviceBackward(neck, case, xs2, gP2, F32, F32, DEV)          # (its forward rewrites the shared merged laterals)
        for x, new in zip(run.inputs, eager.inputs):
            x.copy_(new)
        for g, new in zip(run.gouts, eager.gouts):
            g.copy_(new)
        for t in list(run.grads.values()) + run.gC:
            t.fill_(float('nan'))
        _lib.check(lib.sbev_graph_launch(handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'sbev_graph_launch')
        torch.cuda.synchronize()
    finally:
        lib.sbev_graph_destroy(handle)
    assert run.scale() == eager.scale() and run.scale()[0] > 2.0 ** 8
    for k, g in eager.grads.items():
        assert torch.equal(run.grads[k], g) and bool(torch.isfinite(g).all()), k
    assert all(torch.equal(a, b) for a, b in zip(run.gC, eager.gC))


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------------

@torch.enable_grad()
def test_decoder_trains_through_the_neck():
    from sparsebev_amd import synthetic as S
    from sparsebev_amd.transformer import SparseBEVTransformer
    B, T, Q = 1, 2, 49
    ih, iw, sizes = S.PYRAMIDS['tiny']
    case = FC.Case('pyr', B * T * 6, list(sizes), [32, 64, 96, 128], len(sizes), '')
    xs, nparams = FC.real_data(case, 33)
    neck = BC.make_trainable_neck(case, nparams, DEV)
    params = S.make_params(3, embed_dims=256, num_frames=T, num_points=4, num_levels=len(sizes))
    m = SparseBEVTransformer(256, num_frames=T, num_points=4, num_layers=2, num_levels=len(sizes), num_classes=10, code_size=10, pc_range=S.PC_RANGE)
    m.load_state_dict({'decoder.decoder_layer.' + k: v for k, v in params.items()}, strict=True)
    m = m.to(DEV).train()
    m.decoder.static_graph = False
    bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=4)]
    metas = S.make_img_metas(B, T, ih, iw)
    inputs = [FC.channels_last(x.to(device=DEV, dtype=F16)) for x in xs]
    outs = neck(inputs, out_dtype=F32)
    for o in outs:
        o.retain_grad()
    merged_ws = [mm.clone() for mm in neck.merged]
    cls, box = m(bbox, feat, [o.view(B, T * 6, 256, h, w) for o, (h, w) in zip(outs, sizes)], None, metas)
    g = torch.Generator().manual_seed(2)
    loss = (cls * torch.randn(cls.shape, generator=g).to(DEV)).sum() + (box * torch.randn(box.shape, generator=g).to(DEV)).sum()
    loss.backward()
    tapped = [o.grad for o in outs]                                      # what the decoder's FeatureTap handed back
    assert all(t is not None and t.dtype == F32 and float(t.abs().max()) > 0 for t in tapped)
    by_hand = BC.DeviceBackward(neck, case, xs, [t.cpu() for t in tapped], F16, F32, DEV, input_grads=False)
    assert all(torch.equal(a, b) for a, b in zip(by_hand.merged, merged_ws))
    for k, p in neck.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
        assert torch.equal(p.grad, by_hand.grads[k]), k
