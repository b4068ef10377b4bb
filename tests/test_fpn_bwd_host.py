"""The FPN neck's backward without a GPU: the fp64 restatement (fpn_bwd_cases.py) against torch.autograd with the roundings off, the
children table against nearest_index, sbev_fpn_backward_plan as a literal table with its refusals, the C entry's argument validation
(which returns before any HIP call), and FPNNeck's refusals with and without ``trainable``."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_bwd_cases as BC
import fpn_cases as FC
from sparsebev_amd import _lib
from sparsebev_amd import fpn
from sparsebev_amd._lib import SbevError


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


@pytest.mark.parametrize('case', FC.CASES, ids=[c.name for c in FC.CASES])
def test_restatement_equals_autograd_in_fp64(case):
    xs, params = FC.real_data(case, seed=3)
    gP = BC.real_grads(case, seed=4)
    M, _ = FC.reference(xs, params, case.num_outs, rounded=False)
    ref = BC.backward_reference(xs, params, M, gP, rounded=False)
    assert ref['e'] == 0
    L = len(xs)
    with torch.enable_grad():
        leaves = [x.double().requires_grad_(True) for x in xs]
        p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
        lat = [F.conv2d(leaves[l], p64['lateral_convs.%d.conv.weight' % l], p64['lateral_convs.%d.conv.bias' % l]) for l in range(L)]
        for l in range(L - 1, 0, -1):
            lat[l - 1] = lat[l - 1] + F.interpolate(lat[l], size=lat[l - 1].shape[2:], mode='nearest')
        outs = [F.conv2d(lat[l], p64['fpn_convs.%d.conv.weight' % l], p64['fpn_convs.%d.conv.bias' % l], padding=1) for l in range(L)]
        while len(outs) < case.num_outs:
            outs.append(outs[-1][:, :, ::2, ::2])
        sum((o * g.double()).sum() for o, g in zip(outs, gP)).backward()
    named = BC.param_grads(ref)
    pairs = [('gC%d' % l, ref['gC'][l], leaves[l].grad) for l in range(L)] + [(k, named[k], p64[k].grad) for k in sorted(named)]
    for name, got, want in pairs:
        assert got.dtype == torch.float64 and got.shape == want.shape, name
        assert (got - want).abs().max() <= 1e-12 * max(1.0, float(want.abs().max())), name
    # with the roundings on, the staged gradients and the lateral gradients hold fp16 values in the scaled window
    Mr, _ = FC.reference(xs, params, case.num_outs)
    refr = BC.backward_reference(xs, params, Mr, gP)
    amax = max(float(g.abs().max()) for g in gP)
    assert 2.0 ** BC.WINDOW <= 2.0 ** refr['e'] * amax < 2.0 ** (BC.WINDOW + 1)
    assert all(torch.equal(t, t.half().double()) for t in refr['g'] + refr['gM'])


def test_scale_exponent():
    t = lambda v: [torch.tensor([v, -v / 2])]
    assert BC.WINDOW == 3
    assert BC.scale_exponent(t(8.0)) == 0 and BC.scale_exponent(t(15.99)) == 0 and BC.scale_exponent(t(16.0)) == -1
    assert BC.scale_exponent(t(1.0)) == 3 and BC.scale_exponent(t(2.0 ** -20)) == 23 and BC.scale_exponent(t(2.0 ** -140)) == 126
    assert BC.scale_exponent(t(0.0)) == 0 and BC.scale_exponent(t(float('inf'))) == 0 and BC.scale_exponent(t(float('nan'))) == 0


def test_children_are_the_preimage_of_nearest_index():
    for n_in in range(1, 41):
        for n_out in range(1, 65):
            idx = fpn.nearest_index(n_in, n_out)
            start, stop = fpn.children(n_in, n_out)
            assert start.dtype == np.int64 and start.shape == (n_in,) and stop.shape == (n_in,)
            seen = np.zeros(n_out, dtype=np.int64)
            for s in range(n_in):
                assert 0 <= start[s] <= stop[s] <= n_out
                assert np.array_equal(np.nonzero(idx == s)[0], np.arange(start[s], stop[s])), (n_in, n_out, s)
                seen[start[s]:stop[s]] += 1
            assert np.array_equal(seen, np.ones(n_out, dtype=np.int64)), (n_in, n_out)         # every destination has exactly one parent


R50 = [(256, 64, 176), (512, 32, 88), (1024, 16, 44), (2048, 8, 22)]
W3 = 9 * 256 * 256


def expect_plan(chw, n, num_outs, input_grads):
    """the header's workspace and slab arithmetic, restated"""
    L = len(chw)
    pix = [n * h * w for _, h, w in chw]
    up = lambda v, m: (v + m - 1) // m * m
    slab_len = [max(512, up((p + 15) // 16, 256)) for p in pix]
    slabs = [(p + s - 1) // s for p, s in zip(pix, slab_len)]
    part = max(k * (W3 + 256 * c + 512) for k, (c, _, _) in zip(slabs, chw))
    gm, d = 256, 256 + up(sum(pix) * 512, 256)
    po = d + up(sum(pix[1:]) * 1024, 256)
    return dict(launches=((5 if input_grads else 4) * L + 1) if n else 0, workspace_bytes=(po + 4 * part) if n else 0,
                pack_bytes=sum(c for c, _, _ in chw) * 512 + L * W3 * 2, slabs=slabs if n else [0] * L, slab_len=slab_len, gm_offset=gm, d_offset=d,
                part_offset=po)


def test_backward_plan_literal_table():
    tiny = BC.chw_of(FC.BY_NAME['tiny'])
    five = BC.chw_of(FC.BY_NAME['five'])
    got = fpn.backward_plan(five, 1, 5, True)
    assert got['launches'] == 21 and got['slabs'] == [2, 1, 1, 1] and got['slab_len'] == [512, 512, 512, 512]        # 960 = 512 + 448: a partial last slab
    assert got['pack_bytes'] == fpn.plan(five, 1, 5)['pack_bytes']
    assert got['gm_offset'] == 256 and got['d_offset'] == 256 + 1275 * 512 and got['part_offset'] == got['d_offset'] + 315 * 1024
    assert got['workspace_bytes'] == got['part_offset'] + 4 * 2 * (W3 + 256 * 32 + 512)
    got = fpn.backward_plan(R50, 48, 4)
    assert got['launches'] == 17 and got['slabs'] == [16, 16, 15, 11] and got['slab_len'] == [33792, 8448, 2304, 768]
    got = fpn.backward_plan(R50, 6, 4, True)
    assert got['launches'] == 21 and got['slabs'] == [16, 14, 9, 3] and got['slab_len'] == [4352, 1280, 512, 512]
    for args in [(tiny, 2, 4, False), (tiny, 2, 4, True), (five, 1, 5, True), (five, 0, 5, False), (R50, 6, 4, True), (R50, 48, 4, False),
                 ([(32, 9, 9)], 3, 5, True), ([(64, 1, 513)], 1, 1, False), ([(32, 100, 100)], 1, 2, True)]:
        assert fpn.backward_plan(*args) == expect_plan(*args), (args, fpn.backward_plan(*args))
    many = fpn.backward_plan([(32, 100, 100)], 1, 1)                     # 10000 pixels: 13 slabs of 768 and one of 16
    assert many['slabs'] == [14] and many['slab_len'] == [768] and 10000 - 13 * 768 == 16


def test_backward_plan_refusals(lib):
    one = [(32, 4, 4)]
    table = [
        (([], 1, 1), 'sbev_fpn_backward_plan: 0 input levels (1 .. 4 are built)'),
        ((one * 5, 1, 5), 'sbev_fpn_backward_plan: 5 input levels (1 .. 4 are built)'),
        ((one * 2, 1, 1), 'sbev_fpn_backward_plan: num_outs=1 not in 2 .. 5 (add_extra_convs is not built)'),
        ((one, 1, 6), 'sbev_fpn_backward_plan: num_outs=6 not in 1 .. 5 (add_extra_convs is not built)'),
        ((one, -1, 1), 'sbev_fpn_backward_plan: n=-1 images'),
        (([(48, 4, 4)], 1, 1), 'sbev_fpn_backward_plan: level 0 has 48 input channels (a multiple of 32, at most 65536)'),
        (([(32, 0, 4)], 1, 1), 'sbev_fpn_backward_plan: level 0 has an empty plane (0 x 4)'),
        (([(32, 4, 32768)], 1, 1), 'sbev_fpn_backward_plan: level 0 plane 4 x 32768: a side above 32767'),
        (([(32, 1, 1)], 1 << 31, 1), 'sbev_fpn_backward_plan: 2147483648 pixels: pixel indices are 32-bit'),
    ]
    for args, text in table:
        with pytest.raises(SbevError) as e:
            fpn.backward_plan(*args)
        assert text in str(e.value), (args, str(e.value))
    out = (ctypes.c_int64 * fpn.BWD_PLAN_WORDS)()
    chw = (ctypes.c_int32 * 3)(32, 4, 4)
    assert lib.sbev_fpn_backward_plan(1, None, 1, 1, 0, out) == -1 and b'null level list' in lib.sbev_last_error()
    assert lib.sbev_fpn_backward_plan(1, chw, 1, 1, 0, None) == -1 and b'null out' in lib.sbev_last_error()
    assert lib.sbev_fpn_backward_plan(1, chw, 1, 1, 2, out) == -1 and b'want_input_grads=2 (0 or 1)' in lib.sbev_last_error()
    # the forward's plan is what it was
    assert fpn.PLAN_WORDS == 18 and fpn.plan(one, 1, 1)['launches'] == 2


def test_capi_validation_returns_before_any_gpu_call(lib):
    L = 2
    chw = (ctypes.c_int32 * 6)(32, 4, 4, 64, 2, 2)
    VP = ctypes.c_void_p
    good = dict(inputs=[0x1000, 0x2000], merged=0x3000, gouts=[0x4000, 0x5000], pack=0x6000, ws=0x7000, gx=[0x8000, 0x9000],
                gwl=[0xa000, 0xa400], gbl=[0xb000, 0xb400], gw3=[0xc000, 0xc400], gb3=[0xd000, 0xd400], n=3, num_outs=2, in_dtype=0, g_dtype=2)

    def arr(v):
        return None if v is None else (VP * len(v))(*v)

    def bwd(**o):
        d = dict(good, **o)
        one = lambda k: VP(d[k]) if d[k] else None
        return lib.sbev_fpn_backward(L, chw, d['n'], d['num_outs'], arr(d['inputs']), d['in_dtype'], one('merged'), arr(d['gouts']), d['g_dtype'],
                                     one('pack'), one('ws'), arr(d['gx']), arr(d['gwl']), arr(d['gbl']), arr(d['gw3']), arr(d['gb3']), None)

    nothing = dict(inputs=None, merged=None, gouts=None, pack=None, ws=None, gx=None, gwl=None, gbl=None, gw3=None, gb3=None)
    table = [
        (dict(n=0, **nothing), 0, ''),
        (dict(n=0, num_outs=6, **nothing), -1, 'sbev_fpn_backward: num_outs=6 not in 2 .. 5'),
        (dict(n=0, in_dtype=1, **nothing), -1, 'sbev_fpn_backward: in_dtype 1 (SBEV_F32 or SBEV_F16)'),
        (dict(g_dtype=3), -1, 'sbev_fpn_backward: g_dtype 3 (SBEV_F32 or SBEV_F16)'),
        (nothing, -1, 'sbev_fpn_backward: null pointer'),
        (dict(merged=None), -1, 'sbev_fpn_backward: null pointer'),
        (dict(gw3=None), -1, 'sbev_fpn_backward: null pointer'),
        (dict(inputs=[0x1000, None]), -1, 'sbev_fpn_backward: level 1: null pointer'),
        (dict(gbl=[None, 0xb400]), -1, 'sbev_fpn_backward: level 0: null pointer'),
        (dict(gouts=[0x4000, None]), -1, 'sbev_fpn_backward: output gradient 1: null pointer'),
        (dict(gouts=[0x4008, 0x5000]), -1, 'sbev_fpn_backward: 16-byte alignment'),
        (dict(gx=[0x8000, 0x9008]), -1, 'sbev_fpn_backward: 16-byte alignment'),
        (dict(ws=0x7008), -1, 'sbev_fpn_backward: 16-byte alignment'),
        (dict(merged=0x3004), -1, 'sbev_fpn_backward: 16-byte alignment'),
        (dict(gb3=[0xd002, 0xd400]), -1, 'sbev_fpn_backward: 16-byte alignment'),
    ]
    for overrides, status, text in table:
        got = bwd(**overrides)
        err = lib.sbev_last_error().decode() if got != 0 else ''
        assert got == status and text in err, (overrides, got, err)

    def pack(lat=(0x1000, 0x2000), out=(0x3000, 0x4000), dtype=0, dst=0x5000, levels=L):
        return lib.sbev_fpn_pack_weights_bwd(levels, chw, arr(lat), arr(out), dtype, VP(dst) if dst else None, None)

    assert pack(dst=None) == -1 and b'sbev_fpn_pack_weights_bwd: null pointer' in lib.sbev_last_error()
    assert pack(out=(0x3000, None)) == -1 and b'sbev_fpn_pack_weights_bwd: level 1: null weight' in lib.sbev_last_error()
    assert pack(dtype=1) == -1 and b'sbev_fpn_pack_weights_bwd: w_dtype 1' in lib.sbev_last_error()
    assert pack(dst=0x5004) == -1 and b'sbev_fpn_pack_weights_bwd: 16-byte alignment' in lib.sbev_last_error()


def test_python_refusals():
    from sparsebev_amd import FPNNeck
    cl = lambda *s, dtype=torch.float16: FC.channels_last(torch.zeros(*s, dtype=dtype))
    with pytest.raises(ValueError, match='add_extra_convs'):
        FPNNeck([32, 64], trainable=True, add_extra_convs='on_input')
    with pytest.raises(ValueError, match='hi \\+ lo'):
        FPNNeck([32, 64], trainable=True, grad_mode='f16x2')
    neck = FPNNeck([32, 64])                                                # the default is what it was
    assert neck.trainable is False
    with torch.enable_grad(), pytest.raises(RuntimeError, match='inference only'):
        neck([cl(1, 32, 4, 4), cl(1, 64, 2, 2)])
    neck = FPNNeck([32, 64], 256, 2, trainable=True)
    assert neck.trainable is True and sorted(neck.state_dict()) == sorted(FPNNeck([32, 64]).state_dict())
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match='device tensors'):          # no CPU path, trainable or not
            neck([cl(1, 32, 4, 4), cl(1, 64, 2, 2)])
        with pytest.raises(ValueError, match=r'input 0 is not channels-last'):          # NCHW inputs stay refused
            neck([torch.zeros(1, 32, 4, 4, dtype=torch.float16), cl(1, 64, 2, 2)])
    with torch.no_grad(), pytest.raises(RuntimeError, match='device tensors'):
        neck([cl(1, 32, 4, 4), cl(1, 64, 2, 2)])
