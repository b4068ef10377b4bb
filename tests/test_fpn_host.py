"""The FPN neck without a GPU: the fp64 restatement (fpn_cases.py) against plain torch with the roundings off, the nearest-index rule
against F.interpolate, sbev_fpn_plan as a literal table with its refusals, the C entries' argument validation (which returns before any
HIP call), mmdet's parameter names, and FPNNeck's own refusals."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_cases as FC
from sparsebev_amd import _lib
from sparsebev_amd import fpn
from sparsebev_amd._lib import SbevError


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


@pytest.mark.parametrize('case', FC.CASES, ids=[c.name for c in FC.CASES])
def test_restatement_equals_plain_torch_in_fp64(case):
    xs, params = FC.real_data(case, seed=3)
    M, P = FC.reference(xs, params, case.num_outs, rounded=False)
    L = len(xs)
    lat = [F.conv2d(xs[l].double(), params['lateral_convs.%d.conv.weight' % l].double(), params['lateral_convs.%d.conv.bias' % l].double())
           for l in range(L)]
    for l in range(L - 1, 0, -1):
        lat[l - 1] = lat[l - 1] + F.interpolate(lat[l], size=lat[l - 1].shape[2:], mode='nearest')
    outs = [F.conv2d(lat[l], params['fpn_convs.%d.conv.weight' % l].double(), params['fpn_convs.%d.conv.bias' % l].double(), padding=1)
            for l in range(L)]
    while len(outs) < case.num_outs:
        outs.append(F.max_pool2d(outs[-1], 1, stride=2))
    assert len(P) == case.num_outs and [tuple(p.shape[2:]) for p in P] == FC.out_planes(case)
    for got, want in zip(M + P, lat + outs):
        assert got.dtype == torch.float64 and got.shape == want.shape
        # two orders of summing the same fp64 products: a few ulps of the largest partial sum
        assert (got - want).abs().max() <= 1e-12 * max(1.0, float(want.abs().max()))
    # and with the roundings on the merged laterals hold fp16 values, the operands were rounded
    Mr, _ = FC.reference(xs, params, case.num_outs)
    assert all(torch.equal(m, m.half().double()) for m in Mr)
    assert not torch.equal(Mr[0], M[0])


def test_nearest_index_equals_interpolate():
    for n_in in range(1, 65):
        src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
        for n_out in range(1, 65):
            want = F.interpolate(src, size=(n_out, 1), mode='nearest').view(-1).long().numpy()
            got = fpn.nearest_index(n_in, n_out)
            assert got.dtype == np.int64 and np.array_equal(got, want), (n_in, n_out)
            want_w = F.interpolate(src.view(1, 1, 1, n_in), size=(1, n_out), mode='nearest').view(-1).long().numpy()
            assert np.array_equal(got, want_w), (n_in, n_out)


R50 = [(256, 64, 176), (512, 32, 88), (1024, 16, 44), (2048, 8, 22)]


def test_plan_literal_table():
    tiny = [(c, h, w) for c, (h, w) in zip(FC.BY_NAME['tiny'].cin, FC.BY_NAME['tiny'].planes)]
    five = [(c, h, w) for c, (h, w) in zip(FC.BY_NAME['five'].cin, FC.BY_NAME['five'].planes)]
    conv_bytes = 9 * 256 * 256 * 2
    table = [
        ((tiny, 2, 4), dict(launches=5, pack_bytes=320 * 512 + 4 * conv_bytes, workspace_bytes=66 * 512, pixels=66, conv_tiles=4,
                            lateral_tiles=[1, 1, 1, 1], extra=[])),
        ((R50, 6, 4), dict(launches=5, pack_bytes=3840 * 512 + 4 * conv_bytes, workspace_bytes=89760 * 512, pixels=89760, conv_tiles=702,
                           lateral_tiles=[528, 132, 33, 9], extra=[])),
        ((R50, 48, 4), dict(launches=5, pack_bytes=3840 * 512 + 4 * conv_bytes, workspace_bytes=718080 * 512, pixels=718080, conv_tiles=5610,
                            lateral_tiles=[4224, 1056, 264, 66], extra=[])),
        ((five, 1, 5), dict(launches=5, pack_bytes=128 * 512 + 4 * conv_bytes, workspace_bytes=1275 * 512, pixels=1275, conv_tiles=12,
                            lateral_tiles=[8, 2, 1, 1], extra=[(2, 3)])),
        ((five, 0, 5), dict(launches=0, pack_bytes=128 * 512 + 4 * conv_bytes, workspace_bytes=0, pixels=0, conv_tiles=0,
                            lateral_tiles=[0, 0, 0, 0], extra=[(2, 3)])),
        (([(32, 9, 9)], 3, 5), dict(launches=2, pack_bytes=32 * 512 + conv_bytes, workspace_bytes=243 * 512, pixels=243, conv_tiles=2,
                                    lateral_tiles=[2], extra=[(5, 5), (3, 3), (2, 2), (1, 1)])),
        (([(32, 1, 128)], 1, 1), dict(launches=2, pack_bytes=32 * 512 + conv_bytes, workspace_bytes=128 * 512, pixels=128, conv_tiles=1,
                                      lateral_tiles=[1], extra=[])),
        (([(32, 1, 129)], 1, 1), dict(launches=2, pack_bytes=32 * 512 + conv_bytes, workspace_bytes=129 * 512, pixels=129, conv_tiles=2,
                                      lateral_tiles=[2], extra=[])),
    ]
    for args, want in table:
        assert fpn.plan(*args) == want, (args, fpn.plan(*args))


def test_plan_refusals(lib):
    one = [(32, 4, 4)]
    table = [
        (([], 1, 1), 'sbev_fpn_plan: 0 input levels (1 .. 4 are built)'),
        ((one * 5, 1, 5), 'sbev_fpn_plan: 5 input levels (1 .. 4 are built)'),
        ((one * 2, 1, 1), 'sbev_fpn_plan: num_outs=1 not in 2 .. 5 (add_extra_convs is not built)'),
        ((one, 1, 6), 'sbev_fpn_plan: num_outs=6 not in 1 .. 5 (add_extra_convs is not built)'),
        ((one, -1, 1), 'sbev_fpn_plan: n=-1 images'),
        (([(48, 4, 4)], 1, 1), 'sbev_fpn_plan: level 0 has 48 input channels (a multiple of 32, at most 65536)'),
        ((one + [(16, 2, 2)], 1, 2), 'sbev_fpn_plan: level 1 has 16 input channels (a multiple of 32, at most 65536)'),
        (([(0, 4, 4)], 1, 1), 'sbev_fpn_plan: level 0 has 0 input channels (a multiple of 32, at most 65536)'),
        (([(32, 0, 4)], 1, 1), 'sbev_fpn_plan: level 0 has an empty plane (0 x 4)'),
        (([(32, 4, 32768)], 1, 1), 'sbev_fpn_plan: level 0 plane 4 x 32768: a side above 32767'),
        (([(32, 1, 1)], 1 << 31, 1), 'sbev_fpn_plan: 2147483648 pixels: pixel indices are 32-bit'),
        (([(32, 1024, 1024), (32, 1024, 1024)], 1024, 2), 'sbev_fpn_plan: 2147483648 pixels: pixel indices are 32-bit'),
    ]
    for args, text in table:
        with pytest.raises(SbevError) as e:
            fpn.plan(*args)
        assert text in str(e.value), (args, str(e.value))
    assert fpn.plan([(32, 1, 1)], (1 << 31) - 1 - 128, 1)['pixels'] == (1 << 31) - 129          # the largest count taken
    out = (ctypes.c_int64 * fpn.PLAN_WORDS)()
    assert lib.sbev_fpn_plan(1, None, 1, 1, out) == -1 and b'null level list' in lib.sbev_last_error()
    assert lib.sbev_fpn_plan(1, (ctypes.c_int32 * 3)(32, 4, 4), 1, 1, None) == -1 and b'null out' in lib.sbev_last_error()


def test_capi_validation_returns_before_any_gpu_call(lib):
    L = 2
    chw = (ctypes.c_int32 * 6)(32, 4, 4, 64, 2, 2)
    VP = ctypes.c_void_p
    good = dict(inputs=[0x1000, 0x2000], pack=0x3000, lb=[0x4000, 0x4400], fb=[0x5000, 0x5400], ws=0x6000, outs=[0x7000, 0x8000],
                n=3, num_outs=2, in_dtype=0, out_dtype=2)

    def arr(v):
        return None if v is None else (VP * len(v))(*v)

    def fwd(**o):
        d = dict(good, **o)
        return lib.sbev_fpn_forward(L, chw, d['n'], d['num_outs'], arr(d['inputs']), d['in_dtype'], VP(d['pack']) if d['pack'] else None,
                                    arr(d['lb']), arr(d['fb']), VP(d['ws']) if d['ws'] else None, arr(d['outs']), d['out_dtype'], None)

    nothing = dict(inputs=None, pack=None, lb=None, fb=None, ws=None, outs=None)
    table = [
        (dict(n=0, **nothing), 0, ''),                                                     # the empty call
        (dict(n=0, num_outs=6, **nothing), -1, 'sbev_fpn_forward: num_outs=6 not in 2 .. 5'),      # the plan's refusals come first
        (dict(n=0, in_dtype=1, **nothing), -1, 'sbev_fpn_forward: in_dtype 1 (SBEV_F32 or SBEV_F16)'),
        (dict(out_dtype=3), -1, 'sbev_fpn_forward: out_dtype 3 (SBEV_F32 or SBEV_F16)'),
        (nothing, -1, 'sbev_fpn_forward: null pointer'),
        (dict(pack=None), -1, 'sbev_fpn_forward: null pointer'),
        (dict(ws=None), -1, 'sbev_fpn_forward: null pointer'),
        (dict(inputs=[0x1000, None]), -1, 'sbev_fpn_forward: level 1: null pointer'),
        (dict(fb=[None, 0x5400]), -1, 'sbev_fpn_forward: level 0: null pointer'),
        (dict(outs=[0x7000, None]), -1, 'sbev_fpn_forward: output 1: null pointer'),
        (dict(inputs=[0x1008, 0x2000]), -1, 'sbev_fpn_forward: 16-byte alignment'),
        (dict(outs=[0x7000, 0x8004]), -1, 'sbev_fpn_forward: 16-byte alignment'),
        (dict(pack=0x3008), -1, 'sbev_fpn_forward: 16-byte alignment'),
        (dict(ws=0x6002), -1, 'sbev_fpn_forward: 16-byte alignment'),
        (dict(lb=[0x4002, 0x4400]), -1, 'sbev_fpn_forward: 16-byte alignment'),
    ]
    for overrides, status, text in table:
        got = fwd(**overrides)
        err = lib.sbev_last_error().decode() if got != 0 else ''
        assert got == status and text in err, (overrides, got, err)

    def pack(lat=(0x1000, 0x2000), out=(0x3000, 0x4000), dtype=0, dst=0x5000, levels=L):
        return lib.sbev_fpn_pack_weights(levels, chw, arr(lat), arr(out), dtype, VP(dst) if dst else None, None)

    assert pack(dst=None) == -1 and b'sbev_fpn_pack_weights: null pointer' in lib.sbev_last_error()
    assert pack(lat=None) == -1 and b'sbev_fpn_pack_weights: null pointer' in lib.sbev_last_error()
    assert pack(out=(0x3000, None)) == -1 and b'sbev_fpn_pack_weights: level 1: null weight' in lib.sbev_last_error()
    assert pack(dtype=1) == -1 and b'sbev_fpn_pack_weights: w_dtype 1' in lib.sbev_last_error()
    assert pack(dst=0x5004) == -1 and b'sbev_fpn_pack_weights: 16-byte alignment' in lib.sbev_last_error()
    assert pack(levels=5) == -1 and b'sbev_fpn_pack_weights: 5 input levels' in lib.sbev_last_error()


MMDET_KEYS = [
    'lateral_convs.0.conv.weight', 'lateral_convs.0.conv.bias', 'lateral_convs.1.conv.weight', 'lateral_convs.1.conv.bias',
    'lateral_convs.2.conv.weight', 'lateral_convs.2.conv.bias', 'lateral_convs.3.conv.weight', 'lateral_convs.3.conv.bias',
    'fpn_convs.0.conv.weight', 'fpn_convs.0.conv.bias', 'fpn_convs.1.conv.weight', 'fpn_convs.1.conv.bias',
    'fpn_convs.2.conv.weight', 'fpn_convs.2.conv.bias', 'fpn_convs.3.conv.weight', 'fpn_convs.3.conv.bias',
]


def test_mmdet_state_dict_loads_strict():
    import sparsebev_amd
    cin = [256, 512, 1024, 2048]
    neck = sparsebev_amd.FPNNeck(cin, 256, 4)
    assert sorted(neck.state_dict()) == sorted(MMDET_KEYS)
    for i, c in enumerate(cin):
        w = neck.lateral_convs[i].conv.weight
        assert tuple(w.shape) == (256, c, 1, 1) and tuple(neck.fpn_convs[i].conv.weight.shape) == (256, 256, 3, 3)
        bound = (6.0 / (c + 256)) ** 0.5                                   # Xavier-uniform, zero bias (mmdet's init_cfg)
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
        assert not neck.lateral_convs[i].conv.bias.any() and not neck.fpn_convs[i].conv.bias.any()
    g = torch.Generator().manual_seed(0)
    ckpt = {'img_neck.' + k: torch.randn(neck.state_dict()[k].shape, generator=g) for k in MMDET_KEYS}
    ckpt['img_backbone.conv1.weight'] = torch.zeros(1)
    state = {k[len('img_neck.'):]: v for k, v in ckpt.items() if k.startswith('img_neck.')}
    assert neck.load_state_dict(state, strict=True).missing_keys == []
    assert torch.equal(neck.fpn_convs[2].conv.weight, ckpt['img_neck.fpn_convs.2.conv.weight'])


def test_python_refusals():
    from sparsebev_amd import FPNNeck
    for bad in (dict(in_channels=[32], out_channels=128), dict(in_channels=[]), dict(in_channels=[32] * 5), dict(in_channels=[48]),
                dict(in_channels=[32, 32], num_outs=1), dict(in_channels=[32], num_outs=6)):
        with pytest.raises(ValueError, match='FPNNeck'):
            FPNNeck(**bad)
    neck = FPNNeck([32, 64]).eval()
    assert neck.num_outs == 2
    cl = lambda *s, dtype=torch.float16: FC.channels_last(torch.zeros(*s, dtype=dtype))
    with pytest.raises(ValueError, match='2 inputs'):
        neck([cl(1, 32, 4, 4)])
    with pytest.raises(TypeError, match='all fp16 or all fp32'):
        neck([cl(1, 32, 4, 4), cl(1, 64, 2, 2, dtype=torch.float32)])
    with pytest.raises(TypeError, match='all fp16 or all fp32'):
        neck([cl(1, 32, 4, 4, dtype=torch.bfloat16), cl(1, 64, 2, 2, dtype=torch.bfloat16)])
    with pytest.raises(ValueError, match=r'input 1 has 32 channels, in_channels\[1\] = 64'):
        neck([cl(1, 32, 4, 4), cl(1, 32, 2, 2)])
    with pytest.raises(ValueError, match='one image count'):
        neck([cl(1, 32, 4, 4), cl(2, 64, 2, 2)])
    with pytest.raises(ValueError, match=r'input 0 is not channels-last.*memory_format=torch\.channels_last'):
        neck([torch.zeros(1, 32, 4, 4, dtype=torch.float16), cl(1, 64, 2, 2)])
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match='inference only'):
            neck([cl(1, 32, 4, 4), cl(1, 64, 2, 2)])                      # the parameters require grad
        for p in neck.parameters():
            p.requires_grad_(False)
        with pytest.raises(RuntimeError, match='inference only'):
            neck([cl(1, 32, 4, 4).requires_grad_(True), cl(1, 64, 2, 2)])
    with pytest.raises(RuntimeError, match='device tensors'):              # everything else in order: still no CPU path
        neck([cl(1, 32, 4, 4), cl(1, 64, 2, 2)])
